// hg_refit.hpp -- the least-squares step behind the RANSAC consensus: refit H to every row a
// mask selects (the N-point DLT of the reference's runKernel_DLT, C++ Codes/modules/DLT.cpp:
// 53-119, with the 9x9 eigen-decomposition replaced by an 8x8 LDL^T solve), and the batched
// re-mask / accept step of a local-optimisation round.
//
//   refit_kernel    one block of 256 lanes per pair, everything in binary64 from the binary32
//                   pool values, contraction off, only + - * / fabs:
//                     n        rows of the pair whose mask byte is non-zero
//                     c[4]     sum(x, y, u, v) / n
//                     d[4]     sum |. - c|,  s = n / d
//                     LtL[45]  upper triangle of sum Lx Lx^T + Ly Ly^T over the normalised rows
//                     h'       LtL[0:8,0:8] h' = -LtL[0:8,8] by LDL^T (h'8 = 1), no pivoting
//                     H        T2^-1 H' T1, times 1 / H[8]
//   accept_kernel   one block per pair: the inlier count of H_new over the pair's rows
//                   (is_inlier, the scorer's test); when H_new is finite and the count is >= the
//                   count held, H_io / count_io / the pair's mask rows are overwritten.
//
// THE SUMMATION ORDER of the three sums (c, d, LtL) is part of the definition.  It depends only
// on the pair's row count m and a row's index i inside the pair:
//   * lane l = i % 256 owns rows l, l + 256, l + 512, ... and adds them in ascending order into
//     an accumulator that starts at +0.0; a row that is not selected adds +0.0;
//   * the 256 lane sums v[0..255] are then combined by the xor-butterfly
//         for d = 1, 2, 4, ..., 128:  v[l] <- v[l] + v[l xor d]      (all l at once)
//     (steps 1 ... 32 inside a wave through lane exchanges, 64 and 128 through LDS: the four
//     wave sums w0 ... w3 give (w0 + w1) + (w2 + w3)).  IEEE addition commutes, so every lane
//     ends with the same bits.
// Nothing depends on the grid, on `pairs` or on what other pairs hold.  tests/restate_refit.py
// restates all of it in numpy; the GPU results equal it as bit patterns.
// Included by hg_refit.hip.
#pragma once

#include "hg_consensus.hpp"

#pragma clang fp contract(off)

namespace hg {

constexpr uint64_t kQuietNaN64 = 0x7FF8000000000000ull;
constexpr int kLtL = 45;      // the upper triangle of a 9 x 9 matrix
constexpr int kLtLSums = 30;  // its entries that are not a zero or a copy by structure

static_assert(kBlock == 256 && kWavesPerBlock == 4, "the refit's summation order is 256 lanes, 4 waves");

// Entry (j, k), j <= k, of a 9 x 9 upper triangle stored row by row.
__host__ __device__ constexpr int ltl_at(int j, int k) { return j * 9 - j * (j - 1) / 2 + (k - j); }

// The butterfly over the block's 256 values of each of v[0..N): every thread gets the total.
// `part` holds kWavesPerBlock x N doubles of LDS.
template <int N>
__device__ __forceinline__ void block_butterfly_f64(double (&v)[N], double (*part)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) v[k] = v[k] + __shfl_xor(v[k], d, kWave);
    }
    __syncthreads();  // part may still be read from an earlier call
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) part[threadIdx.x / kWave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// The block's sum of an integer, valid in every thread.  `part`: kWavesPerBlock words of LDS.
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* part) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) v += (uint32_t)__shfl_xor((int)v, d, kWave);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// f(selected, src point, tar point) for the calling lane's rows l, l + 256, ... of a pair, in
// ascending order.  The loads of U steps are issued together (one block streams its pair alone:
// with one load in flight per step a 20 000-row pair paid a memory round trip per step and pass,
// tools/kbench_refit.py); f still sees the rows one by one, in order.
template <int U, typename F>
__device__ __forceinline__ void for_lane_rows(const float2* __restrict__ ps,
                                              const float2* __restrict__ pt,
                                              const uint8_t* __restrict__ mk, uint32_t m, F&& f) {
    uint32_t i = threadIdx.x;  // i + U * 256 < 2^32: m < 2^31
    for (; i + (U - 1) * kBlock < m; i += U * kBlock) {
        float2 a[U], b[U];
        uint8_t s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s[u] = mk[i + u * kBlock];
            a[u] = ps[i + u * kBlock];
            b[u] = pt[i + u * kBlock];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) f(s[u] != 0, a[u], b[u]);
    }
    for (; i < m; i += kBlock) f(mk[i] != 0, ps[i], pt[i]);
}

__device__ __forceinline__ bool finite_f64(double v) {
    return (__builtin_bit_cast(uint64_t, v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull;
}
__device__ __forceinline__ bool finite_f32(float v) {
    return (__builtin_bit_cast(uint32_t, v) & 0x7F800000u) != 0x7F800000u;
}

// LtL (upper triangle), c, s -> H (9 doubles).  False when a pivot is not > 0.
//   A = LtL[0:8,0:8], g = -LtL[0:8,8].  For j = 0 ... 7:
//     v[k] = L[j][k] D[k]                                  (k < j)
//     D[j] = A[j][j] - L[j][0] v[0] - ... - L[j][j-1] v[j-1]   (left to right)
//     L[i][j] = (A[j][i] - L[i][0] v[0] - ... - L[i][j-1] v[j-1]) / D[j]   (i > j)
//   z[i] = g[i] - L[i][0] z[0] - ... - L[i][i-1] z[i-1];  w[i] = z[i] / D[i];
//   h[i] = w[i] - L[i+1][i] h[i+1] - ... - L[7][i] h[7]  (i = 7 ... 0);  h[8] = 1.
//   G = T2^-1 H':  G[k] = h[k] (1 / s2) + c2 h[6+k],  G[3+k] = h[3+k] (1 / s3) + c3 h[6+k],
//                  G[6+k] = h[6+k]                                    (k = 0, 1, 2)
//   F = G T1:      F[3r] = G[3r] s0,  F[3r+1] = G[3r+1] s1,
//                  F[3r+2] = (G[3r] (-(c0 s0)) + G[3r+1] (-(c1 s1))) + G[3r+2]
//   H = F (1 / F[8]).
__device__ __forceinline__ bool refit_solve(const double (&A)[kLtL], const double (&c)[4],
                                            const double (&s)[4], double (&H)[9]) {
    double L[8][8], D[8], v[8];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int k = 0; k < j; ++k) v[k] = L[j][k] * D[k];
        double dj = A[ltl_at(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) dj = dj - L[j][k] * v[k];
        ok = ok && (dj > 0.0);
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 8; ++i) {
            double t = A[ltl_at(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k) t = t - L[i][k] * v[k];
            L[i][j] = t / dj;
        }
    }
    double h[9];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        double z = -A[ltl_at(i, 8)];
#pragma unroll
        for (int k = 0; k < i; ++k) z = z - L[i][k] * h[k];
        h[i] = z;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) h[i] = h[i] / D[i];
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double w = h[i];
#pragma unroll
        for (int k = i + 1; k < 8; ++k) w = w - L[k][i] * h[k];
        h[i] = w;
    }
    h[8] = 1.0;
    const double i2 = 1.0 / s[2], i3 = 1.0 / s[3];
    const double t0 = -(c[0] * s[0]), t1 = -(c[1] * s[1]);
    double G[9], F[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        G[k] = h[k] * i2 + c[2] * h[6 + k];
        G[3 + k] = h[3 + k] * i3 + c[3] * h[6 + k];
        G[6 + k] = h[6 + k];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        F[3 * r] = G[3 * r] * s[0];
        F[3 * r + 1] = G[3 * r + 1] * s[1];
        F[3 * r + 2] = (G[3 * r] * t0 + G[3 * r + 1] * t1) + G[3 * r + 2];
    }
    const double r8 = 1.0 / F[8];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = F[k] * r8;
    return ok;
}

static __global__ __launch_bounds__(kBlock) void refit_kernel(
    const float2* __restrict__ pool_src, const float2* __restrict__ pool_tar, int64_t total,
    const int64_t* __restrict__ pair_offsets, const uint8_t* __restrict__ mask,
    float* __restrict__ H, double* __restrict__ H64, int32_t* __restrict__ used) {
    __shared__ double part[kWavesPerBlock][kLtLSums];
    __shared__ uint32_t cpart[kWavesPerBlock];
    const int64_t j = blockIdx.x;
    int64_t lo;
    uint32_t m;
    consensus_pair_rows(pair_offsets, j, total, lo, m);
    const float2* __restrict__ ps = pool_src + lo;
    const float2* __restrict__ pt = pool_tar + lo;
    const uint8_t* __restrict__ mk = mask + lo;

    // n and the centroid sums
    uint32_t cnt = 0;
    double c[4] = {0.0, 0.0, 0.0, 0.0};
    for_lane_rows<8>(ps, pt, mk, m, [&](bool sel, float2 a, float2 b) {
        cnt += sel ? 1u : 0u;
        c[0] = c[0] + (sel ? (double)a.x : 0.0);
        c[1] = c[1] + (sel ? (double)a.y : 0.0);
        c[2] = c[2] + (sel ? (double)b.x : 0.0);
        c[3] = c[3] + (sel ? (double)b.y : 0.0);
    });
    const uint32_t n = block_sum_u32(cnt, cpart);
    bool ok = n >= 4;  // the same in every thread
    double h[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (ok) {
        block_butterfly_f64(c, reinterpret_cast<double(*)[4]>(&part[0][0]));
        const double nd = (double)n;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = c[k] / nd;

        // the mean absolute deviations
        double d[4] = {0.0, 0.0, 0.0, 0.0};
        for_lane_rows<8>(ps, pt, mk, m, [&](bool sel, float2 a, float2 b) {
            d[0] = d[0] + (sel ? __builtin_fabs((double)a.x - c[0]) : 0.0);
            d[1] = d[1] + (sel ? __builtin_fabs((double)a.y - c[1]) : 0.0);
            d[2] = d[2] + (sel ? __builtin_fabs((double)b.x - c[2]) : 0.0);
            d[3] = d[3] + (sel ? __builtin_fabs((double)b.y - c[3]) : 0.0);
        });
        block_butterfly_f64(d, reinterpret_cast<double(*)[4]>(&part[0][0]));
        double s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok = ok && !(d[k] == 0.0);
            s[k] = nd / d[k];
        }

        // LtL.  The definition adds Lx[j] Lx[k] + Ly[j] Ly[k] for all 45 (j, k); with Lx =
        // [X, Y, 1, 0, 0, 0, ...] and Ly = [0, 0, 0, X, Y, 1, ...] one of the two products, or
        // both, is a zero by structure in 39 of them, so 30 sums are accumulated (kLtLSums):
        //   q[0..5]    X X, X Y, X, Y Y, Y, 1        = LtL[0:3,0:3] and, the same bits, LtL[3:6,3:6]
        //   q[6..14]   Lx[r] Lx[6+k]                 = LtL[0:3,6:9]
        //   q[15..23]  Ly[3+r] Ly[6+k]               = LtL[3:6,6:9]
        //   q[24..29]  Lx[6+p] Lx[6+k] + Ly[6+p] Ly[6+k] = LtL[6:9,6:9]
        // and LtL[0:3,3:6] is +0.0.  For finite X, Y, a, b these are the definition's bits: the
        // product left out is a zero, p + (+-0) is p or a zero of another sign, and a zero of
        // either sign leaves an accumulator that started at +0.0 unchanged (it is never -0.0).
        // When one of them is not finite the literal sums hold NaNs these do not, but then the
        // pair fails either way: X or Y not finite makes pivot 0 or 1 NaN (X X, or inf - inf), a
        // or b not finite makes the sum of -a or -b (q[14], q[23]: the right-hand side) and with
        // it h'[2] or h'[5] and H not finite.  An unselected row enters as X = Y = a = b = +0.0
        // with a 0 for the 1: every product is a zero, as the definition's +0.0.
        double q[kLtLSums];
#pragma unroll
        for (int k = 0; k < kLtLSums; ++k) q[k] = 0.0;
        for_lane_rows<4>(ps, pt, mk, m, [&](bool sel, float2 p, float2 t) {
            const double X = sel ? ((double)p.x - c[0]) * s[0] : 0.0;
            const double Y = sel ? ((double)p.y - c[1]) * s[1] : 0.0;
            const double a = sel ? ((double)t.x - c[2]) * s[2] : 0.0;
            const double b = sel ? ((double)t.y - c[3]) * s[3] : 0.0;
            const double lx[3] = {-a * X, -a * Y, -a}, ly[3] = {-b * X, -b * Y, -b};
            q[0] = q[0] + X * X;
            q[1] = q[1] + X * Y;
            q[2] = q[2] + X;
            q[3] = q[3] + Y * Y;
            q[4] = q[4] + Y;
            q[5] = q[5] + (sel ? 1.0 : 0.0);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q[6 + k] = q[6 + k] + X * lx[k];
                q[9 + k] = q[9 + k] + Y * lx[k];
                q[12 + k] = q[12 + k] + lx[k];
                q[15 + k] = q[15 + k] + X * ly[k];
                q[18 + k] = q[18 + k] + Y * ly[k];
                q[21 + k] = q[21 + k] + ly[k];
            }
            q[24] = q[24] + (lx[0] * lx[0] + ly[0] * ly[0]);
            q[25] = q[25] + (lx[0] * lx[1] + ly[0] * ly[1]);
            q[26] = q[26] + (lx[0] * lx[2] + ly[0] * ly[2]);
            q[27] = q[27] + (lx[1] * lx[1] + ly[1] * ly[1]);
            q[28] = q[28] + (lx[1] * lx[2] + ly[1] * ly[2]);
            q[29] = q[29] + (lx[2] * lx[2] + ly[2] * ly[2]);
        });
        block_butterfly_f64(q, part);
        if (threadIdx.x != 0) return;
        double A[kLtL];
        constexpr int kHead[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
        constexpr int kTail[3][3] = {{24, 25, 26}, {25, 27, 28}, {26, 28, 29}};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k >= r) {
                    A[ltl_at(r, k)] = q[kHead[r][k]];
                    A[ltl_at(3 + r, 3 + k)] = q[kHead[r][k]];
                    A[ltl_at(6 + r, 6 + k)] = q[kTail[r][k]];
                }
                A[ltl_at(r, 3 + k)] = 0.0;
                A[ltl_at(r, 6 + k)] = q[6 + 3 * r + k];
                A[ltl_at(3 + r, 6 + k)] = q[15 + 3 * r + k];
            }
        }
        ok = refit_solve(A, c, s, h) && ok;
#pragma unroll
        for (int k = 0; k < 9; ++k) ok = ok && finite_f64(h[k]) && finite_f32((float)h[k]);
    }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        H[j * 9 + k] = ok ? (float)h[k] : __builtin_bit_cast(float, kQuietNaN);
        if (H64) H64[j * 9 + k] = ok ? h[k] : __builtin_bit_cast(double, kQuietNaN64);
    }
    used[j] = (int32_t)n;
}

// The accept step.  count_io is read by every thread before the block's reduction (two
// barriers) and written by thread 0 after it.
static __global__ __launch_bounds__(kBlock) void accept_kernel(
    const float* __restrict__ H_new, const float2* __restrict__ pool_src,
    const float2* __restrict__ pool_tar, int64_t total, const int64_t* __restrict__ pair_offsets,
    float t2, float* __restrict__ H_io, uint32_t* __restrict__ count_io,
    uint8_t* __restrict__ mask_io) {
    __shared__ uint32_t cpart[kWavesPerBlock];
    const int64_t j = blockIdx.x;
    int64_t lo;
    uint32_t m;
    consensus_pair_rows(pair_offsets, j, total, lo, m);
    const float2* __restrict__ ps = pool_src + lo;
    const float2* __restrict__ pt = pool_tar + lo;
    float h[9];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        h[k] = H_new[j * 9 + k];
        finite = finite && finite_f32(h[k]);
    }
    const uint32_t held = count_io[j];
    if (!finite) return;  // the same in every thread
    uint32_t cnt = 0;
    for (uint32_t i = threadIdx.x; i < m; i += kBlock) {
        const float2 a = ps[i], b = pt[i];
        cnt += is_inlier(h, make_float4(a.x, a.y, b.x, b.y), t2) ? 1u : 0u;
    }
    const uint32_t count = block_sum_u32(cnt, cpart);
    if (count < held) return;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) H_io[j * 9 + k] = h[k];
        count_io[j] = count;
    }
    uint8_t* __restrict__ mk = mask_io + lo;
    for (uint32_t i = threadIdx.x; i < m; i += kBlock) {
        const float2 a = ps[i], b = pt[i];
        mk[i] = is_inlier(h, make_float4(a.x, a.y, b.x, b.y), t2) ? 1 : 0;
    }
}

}  // namespace hg
