"""The batched RANSAC consensus at the C-ABI and wrapper level, without a GPU: the three
entry points are declared and exported, every invalid argument is refused before any HIP
call, the workspace size is a host computation, and the Python wrappers refuse host tensors
and bad shapes.  CPU only; what the kernels compute is tests/test_gpu_consensus.py's."""
import os
import re

import pytest

from conftest import ROOT

NAMES = ("hg_ransac_consensus_workspace", "hg_ransac_consensus_f32", "hg_ransac_inlier_mask_f32")
INVALID = 1  # hipErrorInvalidValue


def test_header_declares_and_library_exports_the_consensus_entries(pkg):
    text = open(os.path.join(ROOT, "include", "sks_homography.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = set(re.findall(r"\b(hg_\w+)\s*\(", text))
    lib = pkg.lib()
    for name in NAMES:
        assert name in decls, f"{name} not declared in sks_homography.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES


def _consensus(lib, pool_src=8, pool_tar=8, total=100, offsets=8, pairs=2, n=64, thresh=3.0,
               seed=11, offset=0, algo=0, best_H=4, best_count=4, best_index=8, mask=None,
               workspace=8):
    """hg_ransac_consensus_f32 with small integers for pointers: valid by value and alignment,
    never dereferenced, because every case below is refused (or is a no-op) first."""
    return lib.hg_ransac_consensus_f32(pool_src, pool_tar, total, offsets, pairs, n, thresh, seed,
                                       offset, algo, best_H, best_count, best_index, mask,
                                       workspace, None)


@pytest.mark.parametrize("bad", [
    dict(pairs=-1), dict(n=0), dict(n=-5), dict(n=(1 << 31) + 1), dict(total=-1),
    dict(total=1 << 31), dict(algo=2), dict(algo=-1), dict(offsets=None), dict(best_H=None),
    dict(best_count=None), dict(best_index=None), dict(workspace=None), dict(pool_src=None),
    dict(pool_tar=None), dict(pool_src=12), dict(pool_tar=4),
])
def test_consensus_argument_validation_without_gpu(pkg, bad):
    assert _consensus(pkg.lib(), **bad) == INVALID, bad


def test_consensus_no_pairs_is_a_no_op(pkg):
    lib = pkg.lib()
    assert _consensus(lib, pairs=0) == 0
    assert lib.hg_ransac_consensus_f32(None, None, 0, None, 0, 1, 1.0, 0, 0, 0, None, None, None,
                                       None, None, None) == 0
    assert _consensus(lib, pairs=0, algo=5) == INVALID     # scalars are checked first
    assert _consensus(lib, pairs=0, total=-1) == INVALID


def test_inlier_mask_argument_validation_without_gpu(pkg):
    f = pkg.lib().hg_ransac_inlier_mask_f32
    assert f(None, None, None, 0, 1.0, None, None) == 0        # no points: no-op
    assert f(None, 8, 8, 5, 1.0, 1, None) == INVALID           # NULL H
    assert f(4, None, 8, 5, 1.0, 1, None) == INVALID           # NULL pool
    assert f(4, 8, None, 5, 1.0, 1, None) == INVALID
    assert f(4, 8, 8, 5, 1.0, None, None) == INVALID           # NULL mask
    assert f(4, 12, 8, 5, 1.0, 1, None) == INVALID             # pool not 8-B aligned
    assert f(4, 8, 20, 5, 1.0, 1, None) == INVALID


def test_workspace_is_positive_and_monotone_in_pairs(pkg):
    ws = pkg.lib().hg_ransac_consensus_workspace
    for n in (1, 2, 511, 512, 513, 1024, 65_537, 1 << 20, 1 << 31):
        sizes = [ws(p, n) for p in (1, 2, 3, 33, 256, 257, 1000, 4096)]
        assert all(s > 0 and s % 8 == 0 for s in sizes), (n, sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), (n, sizes)
        assert ws(1, n) <= ws(1, 2 * n if n < 1 << 30 else n)
    assert ws(0, 16) > 0                      # a call with no pairs still gets a valid size
    assert ws(-1, 16) == 0 and ws(4, 0) == 0 and ws(4, (1 << 31) + 1) == 0   # refused shapes


def test_wrappers_refuse_host_tensors_and_bad_shapes(pkg):
    import torch
    ps, pt = torch.zeros(10, 2), torch.zeros(10, 2)
    with pytest.raises(ValueError, match="GPU only"):
        pkg.ransac_consensus(ps, pt, 16, 3.0)
    with pytest.raises(ValueError, match="GPU only"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, pair_offsets=[0, 4, 10])
    with pytest.raises(ValueError, match="GPU only"):
        pkg.inlier_mask(torch.zeros(9), ps, pt, 3.0)
    with pytest.raises(ValueError, match=r"\(npool,2\)"):
        pkg.ransac_consensus(torch.zeros(10, 3), pt, 16, 3.0)
    with pytest.raises(ValueError, match=r"\(npool,2\)"):
        pkg.ransac_consensus(ps, torch.zeros(20), 16, 3.0)
    with pytest.raises(ValueError, match="same number"):
        pkg.ransac_consensus(ps, torch.zeros(9, 2), 16, 3.0)
    with pytest.raises(ValueError, match="hypotheses"):
        pkg.ransac_consensus(ps, pt, 0, 3.0)
    with pytest.raises(ValueError, match="hypotheses"):
        pkg.ransac_consensus(ps, pt, (1 << 31) + 1, 3.0)
    with pytest.raises(ValueError, match="algo"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, algo="ge")
    with pytest.raises(ValueError, match="pair_offsets"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, pair_offsets=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="pair_offsets"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, pair_offsets=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="9 elements"):
        pkg.inlier_mask(torch.zeros(8), ps, pt, 3.0)
    with pytest.raises(ValueError, match=r"\(npool,2\)"):
        pkg.inlier_mask(torch.zeros(9), torch.zeros(10, 4), pt, 3.0)
    assert pkg.ConsensusResult._fields == ("H", "inliers", "index", "mask")
