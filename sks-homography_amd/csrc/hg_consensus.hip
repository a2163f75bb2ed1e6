// hg_consensus.hip -- the C ABI of the batched RANSAC consensus (added after 0.3):
//
//   hg_ransac_consensus_workspace   bytes of device scratch a call needs (host computation)
//   hg_ransac_consensus_f32         P pairs x n hypotheses -> best H, count, index, inlier mask
//   hg_ransac_inlier_mask_f32       mask[i] = is_inlier(H, point i)
//
// Per pair the result is, bit for bit, hg_sample_solve_seeded_f32 (normalised) +
// hg_ransac_score_f32 + the first arg-max, with the pair's slice of the stream; two launches
// in a chain on `stream`, nothing allocated, no synchronisation.  Kernels: hg_consensus.hpp.
#include "hg_consensus.hpp"

namespace {

constexpr int64_t kMaxHyp = int64_t(1) << 31;

bool consensus_shape_ok(int64_t pairs, int64_t n) {
    if (pairs < 0 || n > kMaxHyp) return false;
    // one grid holds every pair's blocks
    return pairs * hg::kConsensusMaxBlocksPerPair <= 0x7fffffffLL;
}

}  // namespace

extern "C" {

int64_t hg_ransac_consensus_workspace(int64_t pairs, int64_t n) {
    if (!consensus_shape_ok(pairs, n) || n < 1) return 0;
    const int64_t p = pairs < 1 ? 1 : pairs;
    return p * hg::consensus_blocks_per_pair(n) * (int64_t)sizeof(uint64_t);
}

int hg_ransac_consensus_f32(const float* pool_src, const float* pool_tar, int64_t total,
                            const int64_t* pair_offsets, int64_t pairs, int64_t n, float thresh,
                            uint64_t seed, uint64_t offset, int algo, float* best_H,
                            uint32_t* best_count, int64_t* best_index, uint8_t* mask,
                            void* workspace, void* stream) {
    if (!consensus_shape_ok(pairs, n) || total < 0 || total >= kMaxHyp || (algo != 0 && algo != 1))
        return (int)hipErrorInvalidValue;
    if (pairs == 0) return 0;
    if (n < 1) return (int)hipErrorInvalidValue;
    if (!pair_offsets || !best_H || !best_count || !best_index || !workspace ||
        (total && (!pool_src || !pool_tar)))
        return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(pool_src) & 7u) || (reinterpret_cast<uintptr_t>(pool_tar) & 7u) ||
        (reinterpret_cast<uintptr_t>(pair_offsets) & 7u) || (reinterpret_cast<uintptr_t>(best_index) & 7u) ||
        (reinterpret_cast<uintptr_t>(workspace) & 7u) || (reinterpret_cast<uintptr_t>(best_H) & 3u) ||
        (reinterpret_cast<uintptr_t>(best_count) & 3u))
        return (int)hipErrorInvalidValue;
    const uint32_t bpp = (uint32_t)hg::consensus_blocks_per_pair(n);
    const unsigned grid = (unsigned)(pairs * bpp);
    const float t2 = thresh * thresh;
    const uint64_t bits_base = seed * hg::kBitsMul + (offset >> 1);
    const uint32_t odd = (uint32_t)(offset & 1);
    const auto* ps = reinterpret_cast<const float2*>(pool_src);
    const auto* pt = reinterpret_cast<const float2*>(pool_tar);
    auto* partial = reinterpret_cast<uint64_t*>(workspace);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // pool points through wave-uniform loads, unroll 8: the shipped scorer's shape
    int rc = algo == 0
        ? hg::launch(hg::consensus_score_kernel<hg::kACA, 8>, grid, hg::kBlock, 0, s, ps, pt, total,
                     pair_offsets, n, bpp, t2, bits_base, odd, partial)
        : hg::launch(hg::consensus_score_kernel<hg::kSKS, 8>, grid, hg::kBlock, 0, s, ps, pt, total,
                     pair_offsets, n, bpp, t2, bits_base, odd, partial);
    if (rc != 0) return rc;
    const uint32_t mb = mask ? hg::consensus_mask_blocks(total, pairs) : 1u;
    const unsigned grid2 = (unsigned)(pairs * mb);
    return algo == 0
        ? hg::launch(hg::consensus_select_kernel<hg::kACA>, grid2, hg::kBlock, 0, s, ps, pt, total,
                     pair_offsets, n, bpp, mb, t2, bits_base, odd, partial, best_H, best_count,
                     best_index, mask)
        : hg::launch(hg::consensus_select_kernel<hg::kSKS>, grid2, hg::kBlock, 0, s, ps, pt, total,
                     pair_offsets, n, bpp, mb, t2, bits_base, odd, partial, best_H, best_count,
                     best_index, mask);
}

int hg_ransac_inlier_mask_f32(const float* H, const float* pool_src, const float* pool_tar,
                              uint32_t npool, float thresh, uint8_t* mask, void* stream) {
    if (npool == 0) return 0;
    if (!H || !pool_src || !pool_tar || !mask) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(pool_src) & 7u) || (reinterpret_cast<uintptr_t>(pool_tar) & 7u) ||
        (reinterpret_cast<uintptr_t>(H) & 3u))
        return (int)hipErrorInvalidValue;
    const uint32_t want = (npool + hg::kBlock - 1) / hg::kBlock;
    const unsigned grid = want < 4096u ? want : 4096u;
    return hg::launch(hg::consensus_mask_kernel, grid, hg::kBlock, 0,
                      reinterpret_cast<hipStream_t>(stream), H,
                      reinterpret_cast<const float2*>(pool_src),
                      reinterpret_cast<const float2*>(pool_tar), npool, thresh * thresh, mask);
}

}  // extern "C"
