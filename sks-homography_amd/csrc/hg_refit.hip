// hg_refit.hip -- the C ABI of the refinement behind the batched RANSAC consensus (added after
// 0.3):
//
//   hg_ransac_refit_f32    least-squares H (N-point DLT) of the rows a mask selects, per pair
//   hg_ransac_accept_f32   re-mask with a new H per pair, kept where it counts no fewer inliers
//
// One launch each on `stream`, one block per pair, nothing allocated, no workspace, no
// synchronisation.  Kernels and the definition's summation order: hg_refit.hpp.
#include "hg_refit.hpp"

namespace {

constexpr int64_t kMaxRows = int64_t(1) << 31;
constexpr int64_t kMaxPairs = int64_t(1) << 20;

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

}  // namespace

extern "C" {

int hg_ransac_refit_f32(const float* pool_src, const float* pool_tar, int64_t total,
                        const int64_t* pair_offsets, int64_t pairs, const uint8_t* mask,
                        float* H, double* H64, int32_t* used, void* stream) {
    if (pairs < 0 || pairs >= kMaxPairs || total < 0 || total >= kMaxRows)
        return (int)hipErrorInvalidValue;
    if (pairs == 0) return 0;
    if (!pair_offsets || !H || !used || (total && (!pool_src || !pool_tar || !mask)))
        return (int)hipErrorInvalidValue;
    if (misaligned(pool_src, 7u) || misaligned(pool_tar, 7u) || misaligned(pair_offsets, 7u) ||
        misaligned(H64, 7u) || misaligned(H, 3u) || misaligned(used, 3u))
        return (int)hipErrorInvalidValue;
    return hg::launch(hg::refit_kernel, (unsigned)pairs, hg::kBlock, 0,
                      reinterpret_cast<hipStream_t>(stream),
                      reinterpret_cast<const float2*>(pool_src),
                      reinterpret_cast<const float2*>(pool_tar), total, pair_offsets, mask, H, H64,
                      used);
}

int hg_ransac_accept_f32(const float* H_new, const float* pool_src, const float* pool_tar,
                         int64_t total, const int64_t* pair_offsets, int64_t pairs, float thresh,
                         float* H_io, uint32_t* count_io, uint8_t* mask_io, void* stream) {
    if (pairs < 0 || pairs >= kMaxPairs || total < 0 || total >= kMaxRows)
        return (int)hipErrorInvalidValue;
    if (pairs == 0) return 0;
    if (!H_new || !pair_offsets || !H_io || !count_io ||
        (total && (!pool_src || !pool_tar || !mask_io)))
        return (int)hipErrorInvalidValue;
    if (misaligned(pool_src, 7u) || misaligned(pool_tar, 7u) || misaligned(pair_offsets, 7u) ||
        misaligned(H_new, 3u) || misaligned(H_io, 3u) || misaligned(count_io, 3u))
        return (int)hipErrorInvalidValue;
    return hg::launch(hg::accept_kernel, (unsigned)pairs, hg::kBlock, 0,
                      reinterpret_cast<hipStream_t>(stream), H_new,
                      reinterpret_cast<const float2*>(pool_src),
                      reinterpret_cast<const float2*>(pool_tar), total, pair_offsets,
                      thresh * thresh, H_io, count_io, mask_io);
}

}  // extern "C"
