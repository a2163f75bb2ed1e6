// hg_consensus.hpp -- batched RANSAC consensus: draw, solve, score and arg-max n hypotheses
// for each of P image pairs without a per-hypothesis byte in HBM and without the host.
//
//   consensus_score_kernel   grid = pairs x blocks-per-pair.  A lane draws and solves two
//                            hypotheses as one packed f32x2 pair (draws4 + solve, the seeded
//                            sampler's arithmetic), scores both over its pair's pool with the
//                            packed scorer body (pool points through wave-uniform loads, as
//                            ransac_score_sgpr_kernel), and keeps the largest key
//                            (count << 32) | (0xFFFFFFFF - i); one key per block goes to the
//                            workspace.
//   consensus_select_kernel  a few blocks per pair: max over the pair's partial keys, the
//                            winner's H recomputed with the same draw and solve code,
//                            best_H / best_count / best_index, and the inlier mask.
//   consensus_mask_kernel    mask[i] = is_inlier(H, point i) on its own.
//
// Keys are unique per hypothesis of a pair (the index is part of the key), so the maximum is
// the same whatever the order of the reduction: ties go to the lowest index, and the result
// is deterministic.  Pool sizes are known only on the device (pair_offsets), so the draws
// reduce with `%` instead of the host-made fastmod constant; the pool is gathered from global
// memory (L2-resident: 16 B per point) and no LDS is used, so a pool of any size takes the
// same path.  Included by hg_consensus.hip.
#pragma once

#include "hg_ransac.hpp"

#pragma clang fp contract(off)

namespace hg {

constexpr int kConsensusHypPerLane = 2;
constexpr int kConsensusTile = kBlock * kConsensusHypPerLane;  // hypotheses per block and step
// Blocks that share one pair's hypotheses, at most: 2048 blocks of 4 waves fill 256 CUs at 8
// waves per SIMD in one go (1 M hypotheses: one step per block, the shipped scorer's grid; at
// 1024 the same launch ran 4 waves per SIMD and 10 % slower, tools/kbench_consensus.py).
constexpr int64_t kConsensusMaxBlocksPerPair = 2048;
constexpr uint32_t kQuietNaN = 0x7FC00000u;

// Blocks that share one pair's n hypotheses (host and device agree on it).
inline int64_t consensus_blocks_per_pair(int64_t n) {
    const int64_t tiles = (n + kConsensusTile - 1) / kConsensusTile;
    return tiles < 1 ? 1 : (tiles < kConsensusMaxBlocksPerPair ? tiles : kConsensusMaxBlocksPerPair);
}

// Rows [lo, lo + m) of the pool that pair j owns: offsets clamped into [0, total], a
// descending step is an empty pair.
__device__ __forceinline__ void consensus_pair_rows(const int64_t* __restrict__ off, int64_t j,
                                                    int64_t total, int64_t& lo, uint32_t& m) {
    int64_t a = off[j], b = off[j + 1];
    a = a < 0 ? 0 : (a > total ? total : a);
    b = b < 0 ? 0 : (b > total ? total : b);
    lo = a;
    m = b > a ? (uint32_t)(b - a) : 0u;
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kWave);
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kWave);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

// The block's maximum, valid in every thread.  `part` holds kWavesPerBlock words of LDS.
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* part) {
    v = wave_max_u64(v);
    __syncthreads();  // part may still be read from an earlier call
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    uint64_t r = part[0];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) r = part[w] > r ? part[w] : r;
    return r;
}

// Hypotheses pa and pb (positions in the stream: pair * n + index) of a pool of m >= 1 points,
// drawn and solved as the two halves of one packed pair -- the seeded sampler's statements.
template <int ALGO>
__device__ __forceinline__ void consensus_solve2(const float2* __restrict__ ps,
                                                 const float2* __restrict__ pt, uint32_t m,
                                                 uint64_t bits_base, bool odd, int64_t pa,
                                                 int64_t pb, f32x2 (&h)[9]) {
    const u32x4 ra = draws4<kDrawsPaired>(nullptr, bits_base, odd, pa);
    const u32x4 rb = draws4<kDrawsPaired>(nullptr, bits_base, odd, pb);
    f32x2 s[8], t[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t ia = ra[k] % m, ib = rb[k] % m;
        const float2 as = ps[ia], at = pt[ia];
        const float2 bs = ps[ib], bt = pt[ib];
        s[2 * k] = f32x2{as.x, bs.x}; s[2 * k + 1] = f32x2{as.y, bs.y};
        t[2 * k] = f32x2{at.x, bt.x}; t[2 * k + 1] = f32x2{at.y, bt.y};
    }
    solve<ALGO, true, true>(s, t, h);
}

// Pass 1.  Block b of pair j walks hypothesis tiles b, b + bpp, ... of the pair.
template <int ALGO, int UNROLL>
__global__ __launch_bounds__(kBlock) void consensus_score_kernel(
    const float2* __restrict__ pool_src, const float2* __restrict__ pool_tar, int64_t total,
    const int64_t* __restrict__ pair_offsets, int64_t n, uint32_t bpp, float t2,
    uint64_t bits_base, uint32_t bits_odd, uint64_t* __restrict__ partial) {
    __shared__ uint64_t part[kWavesPerBlock];
    const int64_t j = blockIdx.x / bpp;
    const uint32_t b = blockIdx.x % bpp;
    int64_t lo;
    uint32_t m;
    consensus_pair_rows(pair_offsets, j, total, lo, m);
    if (m == 0) return;  // an empty pair: pass 2 does not read its partials
    const float2* __restrict__ ps = pool_src + lo;
    const float2* __restrict__ pt = pool_tar + lo;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const f32x2 t2v = {t2, t2};
    uint64_t best = 0;  // below every key of a real hypothesis (their low words are >= 2^31)
    for (int64_t base = (int64_t)b * kConsensusTile; base < n; base += (int64_t)bpp * kConsensusTile) {
        // the wave's 128 hypotheses: lane, and lane + 64 (past n they are solved and dropped)
        const int64_t ia = base + wave * (2 * kWave) + lane, ib = ia + kWave;
        f32x2 h[9];
        consensus_solve2<ALGO>(ps, pt, m, bits_base, bits_odd != 0, j * n + ia, j * n + ib, h);
        i32x2 cnt = {0, 0};
        auto pair = [&](float2 a, float2 q) {
            const f32x2 x = {a.x, a.x}, y = {a.y, a.y}, nu = {-q.x, -q.x}, nv = {-q.y, -q.y};
            const f32x2 xs = __builtin_elementwise_fma(h[0], x, __builtin_elementwise_fma(h[1], y, h[2]));
            const f32x2 ys = __builtin_elementwise_fma(h[3], x, __builtin_elementwise_fma(h[4], y, h[5]));
            const f32x2 ws = __builtin_elementwise_fma(h[6], x, __builtin_elementwise_fma(h[7], y, h[8]));
            const f32x2 ex = __builtin_elementwise_fma(nu, ws, xs);
            const f32x2 ey = __builtin_elementwise_fma(nv, ws, ys);
            const f32x2 e2 = __builtin_elementwise_fma(ex, ex, ey * ey);
            const f32x2 lim = t2v * (ws * ws);
            const f32x2 zero = {0.f, 0.f};
            cnt -= (e2 <= lim) & (ws != zero);  // vector compares yield -1 / 0
        };
        uint32_t i = 0;
        for (; i + UNROLL <= m; i += UNROLL) {
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) pair(ps[i + u], pt[i + u]);
        }
        for (; i < m; ++i) pair(ps[i], pt[i]);
        const uint64_t ka = ia < n ? ((uint64_t)(uint32_t)cnt.x << 32) | (0xFFFFFFFFu - (uint32_t)ia) : 0;
        const uint64_t kb = ib < n ? ((uint64_t)(uint32_t)cnt.y << 32) | (0xFFFFFFFFu - (uint32_t)ib) : 0;
        best = ka > best ? ka : best;
        best = kb > best ? kb : best;
    }
    best = block_max_u64(best, part);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// Pass 2.  mb blocks per pair: each reduces the pair's partial keys and re-solves the winner
// (the same value in all of them), the first writes best_H / best_count / best_index, and
// together they stream the pair's rows once for the mask (block q: rows q * 256 + lane,
// then every mb * 256).  One block per pair leaves a large pair's mask to 256 lanes.
template <int ALGO>
__global__ __launch_bounds__(kBlock) void consensus_select_kernel(
    const float2* __restrict__ pool_src, const float2* __restrict__ pool_tar, int64_t total,
    const int64_t* __restrict__ pair_offsets, int64_t n, uint32_t bpp, uint32_t mb, float t2,
    uint64_t bits_base, uint32_t bits_odd, const uint64_t* __restrict__ partial,
    float* __restrict__ best_H, uint32_t* __restrict__ best_count,
    int64_t* __restrict__ best_index, uint8_t* __restrict__ mask) {
    __shared__ uint64_t part[kWavesPerBlock];
    const int64_t j = blockIdx.x / mb;
    const uint32_t q = blockIdx.x % mb;
    int64_t lo;
    uint32_t m;
    consensus_pair_rows(pair_offsets, j, total, lo, m);
    if (m == 0) {
        if (q != 0) return;
        if (threadIdx.x < 9)
            best_H[j * 9 + threadIdx.x] = __builtin_bit_cast(float, kQuietNaN);
        if (threadIdx.x == 0) { best_count[j] = 0; best_index[j] = 0; }
        return;
    }
    uint64_t key = 0;
    for (uint32_t k = threadIdx.x; k < bpp; k += kBlock) {
        const uint64_t v = partial[j * bpp + k];
        key = v > key ? v : key;
    }
    key = block_max_u64(key, part);
    const uint32_t count = (uint32_t)(key >> 32);
    const int64_t win = (int64_t)(0xFFFFFFFFu - (uint32_t)key);
    // the winner and its even/odd neighbour as one packed pair, both halves kept live
    const int64_t pa = j * n + (win & ~(int64_t)1);
    f32x2 hp[9];
    consensus_solve2<ALGO>(pool_src + lo, pool_tar + lo, m, bits_base, bits_odd != 0, pa, pa + 1, hp);
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = (win & 1) ? hp[k].y : hp[k].x;
    if (q == 0 && threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) best_H[j * 9 + k] = h[k];
        best_count[j] = count;
        best_index[j] = win;
    }
    if (mask) {
        const float2* __restrict__ ps = pool_src + lo;
        const float2* __restrict__ pt = pool_tar + lo;
        for (uint32_t i = q * kBlock + threadIdx.x; i < m; i += mb * kBlock) {
            const float2 a = ps[i], b = pt[i];
            mask[lo + i] = is_inlier(h, make_float4(a.x, a.y, b.x, b.y), t2) ? 1 : 0;
        }
    }
}

// Blocks per pair of pass 2: about one per 1024 rows of the average pair (the sizes
// themselves are on the device), at most 64.
inline uint32_t consensus_mask_blocks(int64_t total, int64_t pairs) {
    const int64_t per = (total / (pairs < 1 ? 1 : pairs) + 1023) / 1024;
    return (uint32_t)(per < 1 ? 1 : (per > 64 ? 64 : per));
}

static __global__ __launch_bounds__(kBlock) void consensus_mask_kernel(
    const float* __restrict__ H, const float2* __restrict__ pool_src,
    const float2* __restrict__ pool_tar, uint32_t npool, float t2, uint8_t* __restrict__ mask) {
    float h[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = H[k];
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < npool; i += stride) {
        const float2 a = pool_src[i], q = pool_tar[i];
        mask[i] = is_inlier(h, make_float4(a.x, a.y, q.x, q.y), t2) ? 1 : 0;
    }
}

}  // namespace hg
