"""RANSAC on the solver: hypothesis sampling, the fused
gather + closed-form solve, and inlier scoring -- all on the device.

The reference stops at timing random 4-point hypotheses: cuRAND indices, the
get_rand_list gather and the solver kernel (GPU_Runtime Test.cu:1443-1451, :52-78,
:81-151), the "sampling number" use case of its Table 8.  This module runs that
pipeline, adds the scoring step it implies, and returns the best hypothesis.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib
from .ops import _gpu_device, _guard, _require_device, _stream


_strtof_fn = None


def _strtof(tokens):
    """Decimal strings -> binary32 the way the reference's sscanf("%f") converts them (C
    strtof: one correct rounding).  numpy's str -> float32 goes through binary64 first, and
    that double rounding gives the other neighbour for a decimal just above a binary32
    midpoint (e.g. 1.00000005960464477539062500000001 -> 1.0 instead of 1 + 2^-23)."""
    global _strtof_fn
    import ctypes
    import ctypes.util

    import numpy as np

    if _strtof_fn is None:
        fn = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6").strtof
        fn.restype = ctypes.c_float
        fn.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
        _strtof_fn = fn
    return np.array([_strtof_fn(t.encode(), None) for t in tokens], dtype=np.float32)


def read_points(filename: str):
    """The reference's correspondence-file reader (CPU_Runtime Test/utils.cpp:6-21; the GPU
    harness's copy at GPU_Runtime Test.cu:31-46): the first line holds the count N, then N
    lines "x1 y1 x2 y2" (source point, target point), each value parsed as sscanf's "%f"
    does.  Returns (pool_src, pool_tar), each an (N,2) float32 numpy array, ready for
    sample_solve / score / ransac (orig_pts_wall.txt is the reference's own file)."""
    import numpy as np

    with open(filename) as f:
        head = f.readline().split()
        if not head:
            raise ValueError(f"{filename}: empty file (expected the point count first)")
        count = int(head[0])
        tokens = []
        for i in range(count):
            vals = f.readline().split()[:4]
            if len(vals) < 4:
                raise ValueError(f"{filename}: line {i + 2} has fewer than 4 values")
            tokens += vals
    a = _strtof(tokens).reshape(count, 4)
    return np.ascontiguousarray(a[:, 0:2]), np.ascontiguousarray(a[:, 2:4])


def fill_bits(count: int, seed: int, offset: int = 0, device="cuda") -> torch.Tensor:
    """Counter-based uint32 draws (held in an int32 tensor), bit-identical to the
    host regeneration."""
    if count < 0:
        raise ValueError(f"count must be >= 0, got {count}")
    dev = _gpu_device(device)
    out = torch.empty(count, dtype=torch.int32, device=dev)
    with _guard(dev):
        _lib.call("hg_fill_bits_u32", out.data_ptr(), count, seed, offset, _stream(dev))
    return out


def _pool(pool: torch.Tensor) -> torch.Tensor:
    if pool.dim() != 2 or pool.shape[1] != 2:
        raise ValueError(f"pool must be (npool,2), got {tuple(pool.shape)}")
    return pool.to(torch.float32).contiguous()


def sample_solve(pool_src: torch.Tensor, pool_tar: torch.Tensor, idx: torch.Tensor,
                 algo: str = "aca", normalize: bool = True) -> torch.Tensor:
    """H of each row of ``idx`` ((n,4) int32/uint32; entries reduced modulo the pool
    size like get_rand_list, .cu:56-59) gathered from (npool,2) pools.  (n,9)."""
    dev = _require_device(pool_src, pool_tar, idx)
    if idx.dim() != 2 or idx.shape[1] != 4 or idx.dtype not in (torch.int32, torch.uint32):
        raise ValueError("idx must be an (n,4) int32/uint32 tensor")
    if algo not in ("aca", "sks"):
        raise ValueError(f"algo must be 'aca' or 'sks', got {algo!r}")
    ps, pt, idx = _pool(pool_src), _pool(pool_tar), idx.contiguous()
    n = idx.shape[0]
    out = torch.empty((n, 9), dtype=torch.float32, device=dev)
    with _guard(dev):
        _lib.call("hg_sample_solve_f32", ps.data_ptr(), pt.data_ptr(), ps.shape[0],
                  idx.data_ptr(), out.data_ptr(), n, 0 if algo == "aca" else 1,
                  1 if normalize else 0, _stream(dev))
    return out


def sample_solve_seeded(pool_src: torch.Tensor, pool_tar: torch.Tensor, n: int, seed: int,
                        offset: int = 0, algo: str = "aca", normalize: bool = True) -> torch.Tensor:
    """``n`` hypotheses drawn AND solved in one launch: bit for bit
    ``sample_solve(pool_src, pool_tar, fill_bits(4 * n, seed, offset).view(n, 4))``, with the
    draws made in the kernel instead of read from an index array.  (n,9)."""
    dev = _require_device(pool_src, pool_tar)
    if algo not in ("aca", "sks"):
        raise ValueError(f"algo must be 'aca' or 'sks', got {algo!r}")
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    ps, pt = _pool(pool_src), _pool(pool_tar)
    out = torch.empty((n, 9), dtype=torch.float32, device=dev)
    with _guard(dev):
        _lib.call("hg_sample_solve_seeded_f32", ps.data_ptr(), pt.data_ptr(), ps.shape[0],
                  seed, offset, out.data_ptr(), n, 0 if algo == "aca" else 1,
                  1 if normalize else 0, _stream(dev))
    return out


def score(H: torch.Tensor, pool_src: torch.Tensor, pool_tar: torch.Tensor,
          thresh: float) -> torch.Tensor:
    """Inlier count of every hypothesis H (n,9) over the pool: points whose
    reprojection error is at most ``thresh`` (division-free test, see
    include/sks_homography.h).  Returns (n,) int32."""
    dev = _require_device(H, pool_src, pool_tar)
    H = H.reshape(-1, 9).to(torch.float32).contiguous()
    ps, pt = _pool(pool_src), _pool(pool_tar)
    counts = torch.empty(H.shape[0], dtype=torch.int32, device=dev)
    with _guard(dev):
        _lib.call("hg_ransac_score_f32", H.data_ptr(), H.shape[0], ps.data_ptr(), pt.data_ptr(),
                  ps.shape[0], float(thresh), counts.data_ptr(), _stream(dev))
    return counts


# ---- the reference's Table-8 pipeline in its own formats (GPU_Runtime Test.cu:1443-1451) ----
_ALGO_IDS = {"aca": 0, "sks": 1, "ge": 2, "gpt": 3}


def rand_mrg32k3a(count: int, seed: int = 11, device="cuda") -> torch.Tensor:
    """``count`` MRG32K3A words, as curandGenerate fills the reference's index list
    (.cu:1443-1446, seed 11): the hand-written generator, uint32 values in an int32 tensor.
    The words equal rocRAND's host-API MRG32K3A words on gfx950 bit for bit (their order is
    rocRAND's gfx950 launch layout, hg_mrg32k3a.hpp kOrderLog2); equality with cuRAND's
    words, which the reference's CUDA harness draws, is unpinned (no cuRAND here).
    Asynchronous on the current stream, like every op here."""
    if count < 0:
        raise ValueError(f"count must be >= 0, got {count}")
    dev = _gpu_device(device)
    out = torch.empty(count, dtype=torch.int32, device=dev)
    with _guard(dev):
        _lib.call("hg_rand_mrg32k3a_u32", out.data_ptr(), count, seed, _stream(dev))
    return out


def _point_pool(pool: torch.Tensor) -> torch.Tensor:
    if pool.dim() != 2 or pool.shape[1] != 2 or pool.dtype != torch.float64:
        raise ValueError(f"pool must be an (npool,2) float64 tensor (Point2d), got "
                         f"{tuple(pool.shape)} {pool.dtype}")
    return pool.contiguous()


def _rand_list(rl: torch.Tensor) -> torch.Tensor:
    if rl.dim() != 2 or rl.shape[0] != 4 or rl.dtype not in (torch.int32, torch.uint32):
        raise ValueError("rand_list must be a (4,n) int32/uint32 tensor (word k of hypothesis "
                         "id at [k, id], as get_rand_list reads it)")
    return rl.contiguous()


def get_rand_list(rand_list: torch.Tensor, pool_src: torch.Tensor, pool_tar: torch.Tensor):
    """The reference's get_rand_list (.cu:52-78): (4,n) words and two (npool,2) float64
    point pools -> (d_src, d_tar), each (8,n) float64 SoA, ready for solve(..., layout="soa")."""
    dev = _require_device(rand_list, pool_src, pool_tar)
    rl, ps, pt = _rand_list(rand_list), _point_pool(pool_src), _point_pool(pool_tar)
    if ps.shape[0] != pt.shape[0] or ps.shape[0] == 0:
        raise ValueError("pool_src and pool_tar must hold the same, non-zero number of points")
    n = rl.shape[1]
    d_src = torch.empty((8, n), dtype=torch.float64, device=dev)
    d_tar = torch.empty((8, n), dtype=torch.float64, device=dev)
    with _guard(dev):
        _lib.call("hg_get_rand_list_f64", rl.data_ptr(), ps.shape[0], ps.data_ptr(), pt.data_ptr(),
                  d_src.data_ptr(), d_tar.data_ptr(), n, _stream(dev))
    return d_src, d_tar


def gather_solve(pool_src: torch.Tensor, pool_tar: torch.Tensor, rand_list: torch.Tensor,
                 algo: str = "aca", normalize: bool = False) -> torch.Tensor:
    """get_rand_list fused with cal_Homo_{ACA,SKS,GE,GPT} (.cu:52-78 + :81-507): (9,n)
    float64 SoA H, bit for bit ``solve(algo, *get_rand_list(...), normalize, layout="soa")``
    without the (8,n) rows in memory.  Unnormalised by default, like the reference kernels."""
    dev = _require_device(rand_list, pool_src, pool_tar)
    if algo not in _ALGO_IDS:
        raise ValueError(f"algo must be one of {sorted(_ALGO_IDS)}, got {algo!r}")
    rl, ps, pt = _rand_list(rand_list), _point_pool(pool_src), _point_pool(pool_tar)
    if ps.shape[0] != pt.shape[0] or ps.shape[0] == 0:
        raise ValueError("pool_src and pool_tar must hold the same, non-zero number of points")
    n = rl.shape[1]
    H = torch.empty((9, n), dtype=torch.float64, device=dev)
    with _guard(dev):
        _lib.call("hg_gather_solve_f64", _ALGO_IDS[algo], ps.data_ptr(), pt.data_ptr(), ps.shape[0],
                  rl.data_ptr(), H.data_ptr(), n, 1 if normalize else 0, _stream(dev))
    return H


def rand_gather_solve(pool_src: torch.Tensor, pool_tar: torch.Tensor, n: int, seed: int = 11,
                      algo: str = "aca", normalize: bool = False) -> torch.Tensor:
    """The whole Table-8 flow in one launch (.cu:1443-1451 + :52-78 + :81-507): (9,n) float64
    SoA H, bit for bit ``gather_solve(pool_src, pool_tar, rand_mrg32k3a(4*n, seed).view(4, n),
    algo, normalize)``, with the MRG32K3A words made in registers."""
    dev = _require_device(pool_src, pool_tar)
    if algo not in _ALGO_IDS:
        raise ValueError(f"algo must be one of {sorted(_ALGO_IDS)}, got {algo!r}")
    if n < 0:
        raise ValueError(f"n must be >= 0, got {n}")
    ps, pt = _point_pool(pool_src), _point_pool(pool_tar)
    if ps.shape[0] != pt.shape[0] or ps.shape[0] == 0:
        raise ValueError("pool_src and pool_tar must hold the same, non-zero number of points")
    H = torch.empty((9, n), dtype=torch.float64, device=dev)
    with _guard(dev):
        _lib.call("hg_rand_gather_solve_f64", _ALGO_IDS[algo], ps.data_ptr(), pt.data_ptr(),
                  ps.shape[0], seed, H.data_ptr(), n, 1 if normalize else 0, _stream(dev))
    return H


def mrg32k3a_state(seed: int, subsequence: int = 0, offset: int = 0) -> tuple:
    """The engine state curand_init / rocrand_init(seed, subsequence, offset) sets up, as
    (x1[n-3], x1[n-2], x1[n-1], x2[n-3], x2[n-2], x2[n-1]) (host computation)."""
    st = (ctypes.c_uint32 * 6)()
    _lib.call("hg_mrg32k3a_state", seed, subsequence, offset, st)
    return tuple(st)


class RansacResult(NamedTuple):
    H: torch.Tensor          # (9,) best hypothesis (normalised)
    inliers: int             # its inlier count
    index: int               # which hypothesis won
    counts: torch.Tensor     # (n,) inlier count of every hypothesis


def ransac(pool_src: torch.Tensor, pool_tar: torch.Tensor, hypotheses: int, thresh: float,
           seed: int = 11, algo: str = "aca") -> RansacResult:
    """Draws ``hypotheses`` random 4-point samples and solves them (one fused launch),
    scores them all and returns the best (ties: lowest index).  The winner is read back
    through the host; ``ransac_consensus`` gives the same H, count and index -- for many
    image pairs in one call, with the inlier mask, without a host round trip -- when the
    per-hypothesis counts are not needed."""
    _require_device(pool_src, pool_tar)
    if hypotheses < 1:
        raise ValueError(f"ransac needs at least one hypothesis, got {hypotheses}")
    H = sample_solve_seeded(pool_src, pool_tar, hypotheses, seed, 0, algo=algo, normalize=True)
    counts = score(H, pool_src, pool_tar, thresh)
    best = int((counts == counts.max()).nonzero()[0].item())
    return RansacResult(H[best].clone(), int(counts[best].item()), best, counts)


class ConsensusResult(NamedTuple):
    H: torch.Tensor          # (pairs,9) float32: best hypothesis of each pair (normalised)
    inliers: torch.Tensor    # (pairs,) int32: its inlier count
    index: torch.Tensor      # (pairs,) int64: which hypothesis won (ties: lowest)
    mask: torch.Tensor       # (total,) uint8: 1 where a pool row is an inlier of its pair's H


def _pair_pools(pool_src: torch.Tensor, pool_tar: torch.Tensor):
    for p in (pool_src, pool_tar):
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError(f"pool must be (npool,2), got {tuple(p.shape)}")
    if pool_src.shape[0] != pool_tar.shape[0]:
        raise ValueError("pool_src and pool_tar must hold the same number of points, got "
                         f"{pool_src.shape[0]} and {pool_tar.shape[0]}")
    if pool_src.shape[0] >= 1 << 31:
        raise ValueError("the pools must hold fewer than 2^31 points")


def _pair_offsets(pair_offsets, total: int):
    """pair_offsets as ransac_consensus takes them (None, a list, a host or a device int64
    tensor), checked but not yet moved: a 1-D int64 tensor."""
    if pair_offsets is None:
        pair_offsets = [0, total]
    if not isinstance(pair_offsets, torch.Tensor):
        pair_offsets = torch.tensor([int(v) for v in pair_offsets], dtype=torch.int64)
    if pair_offsets.dim() != 1 or pair_offsets.numel() < 1 or pair_offsets.dtype != torch.int64:
        raise ValueError("pair_offsets must be a 1-D int64 tensor (or a list) of pairs + 1 "
                         f"offsets, got {tuple(pair_offsets.shape)} {pair_offsets.dtype}")
    return pair_offsets


def _offsets_on(pair_offsets: torch.Tensor, dev) -> torch.Tensor:
    if pair_offsets.device != dev:
        if pair_offsets.is_cuda:
            raise ValueError(f"tensors on different devices: {dev} vs {pair_offsets.device}")
        pair_offsets = pair_offsets.to(dev)
    return pair_offsets.contiguous()


class RefitResult(NamedTuple):
    H: torch.Tensor          # (pairs,9) float32: least-squares H of each pair's selected rows
    used: torch.Tensor       # (pairs,) int32: how many rows the mask selected
    H64: torch.Tensor = None  # (pairs,9) float64: the same before rounding (return_f64=True)


def refit(pool_src: torch.Tensor, pool_tar: torch.Tensor, mask: torch.Tensor, pair_offsets=None,
          return_f64: bool = False) -> RefitResult:
    """Least-squares refit (N-point DLT, hg_ransac_refit_f32) of every pair's selected rows.

    Pools and ``pair_offsets`` as ``ransac_consensus``; ``mask`` is a (total,) uint8 device
    tensor and any non-zero byte selects its row -- a consensus mask as it stands.  In binary64
    and in a fixed summation order (include/sks_homography.h), so the result is deterministic
    and independent of the batch.  A pair that cannot be fitted (fewer than 4 rows selected,
    degenerate points, a non-finite result) gets a NaN H; ``used`` still counts its rows.
    Everything returned is a device tensor; nothing synchronises."""
    _pair_pools(pool_src, pool_tar)
    total = pool_src.shape[0]
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.shape != (total,):
        raise ValueError(f"mask must be a ({total},) uint8 tensor, got "
                         f"{tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask)} "
                         f"{getattr(mask, 'dtype', '')}")
    pair_offsets = _pair_offsets(pair_offsets, total)
    dev = _require_device(pool_src, pool_tar, mask)
    off = _offsets_on(pair_offsets, dev)
    pairs = off.numel() - 1
    ps, pt, mk = _pool(pool_src), _pool(pool_tar), mask.contiguous()
    H = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
    used = torch.empty(pairs, dtype=torch.int32, device=dev)
    H64 = torch.empty((pairs, 9), dtype=torch.float64, device=dev) if return_f64 else None
    with _guard(dev):
        _lib.call("hg_ransac_refit_f32", ps.data_ptr(), pt.data_ptr(), total, off.data_ptr(), pairs,
                  mk.data_ptr(), H.data_ptr(), H64.data_ptr() if return_f64 else None,
                  used.data_ptr(), _stream(dev))
    return RefitResult(H, used, H64)


def ransac_consensus(pool_src: torch.Tensor, pool_tar: torch.Tensor, hypotheses: int,
                     thresh: float, pair_offsets=None, seed: int = 11, offset: int = 0,
                     algo: str = "aca", mask: bool = True, refine: int = 0) -> ConsensusResult:
    """RANSAC consensus of many image pairs in one device pass (hg_ransac_consensus_f32).

    The pools hold every pair's correspondences back to back; pair j owns rows
    ``pair_offsets[j]:pair_offsets[j+1]`` (a list, or an int64 tensor -- a host one is moved to
    the device once; None: one pair, the whole pool).  For each pair, ``hypotheses`` samples
    are drawn, solved, scored and reduced on the device: (H, inliers, index) equal
    ``ransac(pool_j, ..)`` made with stream offset ``offset + 4 * hypotheses * j``, bit for
    bit, and ``mask`` marks the pair's inliers of its H (all zero when ``mask=False``).  An
    empty pair gives NaN H, 0 inliers, index 0.  Everything returned is a device tensor;
    nothing synchronises, so the call can be captured in a graph.

    ``refine=R`` (needs ``mask=True``) then runs R local-optimisation rounds on those outputs,
    still on the device: ``refit`` on each pair's inliers, and hg_ransac_accept_f32, which
    re-masks with the refitted H and keeps it where it counts no fewer inliers.  H, inliers
    and mask are then the accepted ones (inliers never falls from round to round); index is
    still the winning hypothesis.  ``refine=0`` makes exactly the calls made without it."""
    _pair_pools(pool_src, pool_tar)
    if algo not in ("aca", "sks"):
        raise ValueError(f"algo must be 'aca' or 'sks', got {algo!r}")
    if not 1 <= hypotheses <= 1 << 31:
        raise ValueError(f"hypotheses must be in [1, 2^31], got {hypotheses}")
    if not isinstance(refine, int) or isinstance(refine, bool) or refine < 0:
        raise ValueError(f"refine must be an integer >= 0, got {refine!r}")
    if refine and not mask:
        raise ValueError("refine > 0 refits the inliers the mask marks: it requires mask=True")
    total = pool_src.shape[0]
    pair_offsets = _pair_offsets(pair_offsets, total)
    # offsets known on the host that rise from <= 0 to >= total give every row to one pair:
    # the kernel then writes the whole mask, and it need not be cleared first
    tiled = False
    if mask and not pair_offsets.is_cuda:
        v = pair_offsets.tolist()
        tiled = v[0] <= 0 and v[-1] >= total and all(a <= b for a, b in zip(v, v[1:]))
    dev = _require_device(pool_src, pool_tar)
    off = _offsets_on(pair_offsets, dev)
    pairs = off.numel() - 1
    ps, pt = _pool(pool_src), _pool(pool_tar)
    H = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
    inliers = torch.empty(pairs, dtype=torch.int32, device=dev)
    index = torch.empty(pairs, dtype=torch.int64, device=dev)
    out_mask = (torch.empty if tiled else torch.zeros)(total, dtype=torch.uint8, device=dev)
    need = _lib.lib().hg_ransac_consensus_workspace(pairs, hypotheses)
    if need <= 0:
        raise ValueError(f"{pairs} pairs x {hypotheses} hypotheses is beyond one call")
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    with _guard(dev):
        _lib.call("hg_ransac_consensus_f32", ps.data_ptr(), pt.data_ptr(), total, off.data_ptr(),
                  pairs, hypotheses, float(thresh), seed, offset, 0 if algo == "aca" else 1,
                  H.data_ptr(), inliers.data_ptr(), index.data_ptr(),
                  out_mask.data_ptr() if mask else None, work.data_ptr(), _stream(dev))
        if refine:
            H_new = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
            used = torch.empty(pairs, dtype=torch.int32, device=dev)
        for _ in range(refine):
            _lib.call("hg_ransac_refit_f32", ps.data_ptr(), pt.data_ptr(), total, off.data_ptr(),
                      pairs, out_mask.data_ptr(), H_new.data_ptr(), None, used.data_ptr(),
                      _stream(dev))
            _lib.call("hg_ransac_accept_f32", H_new.data_ptr(), ps.data_ptr(), pt.data_ptr(), total,
                      off.data_ptr(), pairs, float(thresh), H.data_ptr(), inliers.data_ptr(),
                      out_mask.data_ptr(), _stream(dev))
    return ConsensusResult(H, inliers, index, out_mask)


def inlier_mask(H: torch.Tensor, pool_src: torch.Tensor, pool_tar: torch.Tensor,
                thresh: float) -> torch.Tensor:
    """(npool,) uint8: 1 where a correspondence is an inlier of the one homography ``H``
    (9 elements, on the device) by ``score``'s test -- ``score`` of one-point pools."""
    _pair_pools(pool_src, pool_tar)
    if H.numel() != 9:
        raise ValueError(f"H must hold 9 elements, got {tuple(H.shape)}")
    dev = _require_device(H, pool_src, pool_tar)
    H = H.reshape(9).to(torch.float32).contiguous()
    ps, pt = _pool(pool_src), _pool(pool_tar)
    out = torch.empty(ps.shape[0], dtype=torch.uint8, device=dev)
    with _guard(dev):
        _lib.call("hg_ransac_inlier_mask_f32", H.data_ptr(), ps.data_ptr(), pt.data_ptr(),
                  ps.shape[0], float(thresh), out.data_ptr(), _stream(dev))
    return out
