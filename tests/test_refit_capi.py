"""The least-squares refit and the accept step at the C-ABI and wrapper level, without a GPU:
both entry points are declared and exported, every invalid argument is refused before any HIP
call, no pairs is a no-op, and the Python wrappers refuse host tensors and bad shapes.  CPU
only; what the kernels compute is tests/test_gpu_refit.py's, what the definition means
tests/test_refit_restatement.py's."""
import os
import re

import pytest

from conftest import ROOT

NAMES = ("hg_ransac_refit_f32", "hg_ransac_accept_f32")
INVALID = 1  # hipErrorInvalidValue


def test_header_declares_and_library_exports_the_refit_entries(pkg):
    text = open(os.path.join(ROOT, "include", "sks_homography.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = set(re.findall(r"\b(hg_\w+)\s*\(", text))
    lib = pkg.lib()
    for name in NAMES:
        assert name in decls, f"{name} not declared in sks_homography.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in pkg._lib.SIGNATURES
    assert len(pkg._lib.SIGNATURES["hg_ransac_refit_f32"][0]) == 10
    assert len(pkg._lib.SIGNATURES["hg_ransac_accept_f32"][0]) == 11


def test_refit_sits_in_its_own_translation_unit():
    """The existing kernels' machine code is pinned by digest (tests/test_capi.py): the new
    kernels are built from their own source file."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "sks-homography_amd"))
    try:
        import build_lib as bl
    finally:
        sys.path.pop(0)
    assert "hg_refit.hip" in bl.SOURCES
    for f in ("hg_refit.hip", "hg_refit.hpp"):
        assert os.path.exists(os.path.join(bl.CSRC, f))
    codes = bl.demangle(bl.device_code_digests())
    assert any("hg::refit_kernel" in d for d in codes.values())
    assert any("hg::accept_kernel" in d for d in codes.values())


def _refit(lib, pool_src=8, pool_tar=8, total=100, offsets=8, pairs=2, mask=1, H=4, H64=8, used=4):
    """hg_ransac_refit_f32 with small integers for pointers: valid by value and alignment,
    never dereferenced, because every case below is refused (or is a no-op) first."""
    return lib.hg_ransac_refit_f32(pool_src, pool_tar, total, offsets, pairs, mask, H, H64, used, None)


def _accept(lib, H_new=4, pool_src=8, pool_tar=8, total=100, offsets=8, pairs=2, thresh=3.0,
            H_io=4, count_io=4, mask_io=1):
    return lib.hg_ransac_accept_f32(H_new, pool_src, pool_tar, total, offsets, pairs, thresh, H_io,
                                    count_io, mask_io, None)


@pytest.mark.parametrize("bad", [
    dict(pairs=-1), dict(pairs=1 << 20), dict(total=-1), dict(total=1 << 31), dict(offsets=None),
    dict(H=None), dict(used=None), dict(pool_src=None), dict(pool_tar=None), dict(mask=None),
    dict(pool_src=12), dict(pool_tar=4), dict(offsets=4), dict(H64=4), dict(H64=12), dict(H=2),
    dict(used=6),
])
def test_refit_argument_validation_without_gpu(pkg, bad):
    assert _refit(pkg.lib(), **bad) == INVALID, bad


@pytest.mark.parametrize("bad", [
    dict(pairs=-1), dict(pairs=1 << 20), dict(total=-1), dict(total=1 << 31), dict(offsets=None),
    dict(H_new=None), dict(H_io=None), dict(count_io=None), dict(pool_src=None),
    dict(pool_tar=None), dict(mask_io=None), dict(pool_src=12), dict(pool_tar=4), dict(offsets=4),
    dict(H_new=2), dict(H_io=6), dict(count_io=1),
])
def test_accept_argument_validation_without_gpu(pkg, bad):
    assert _accept(pkg.lib(), **bad) == INVALID, bad


def test_no_pairs_is_a_no_op(pkg):
    lib = pkg.lib()
    assert _refit(lib, pairs=0) == 0 and _accept(lib, pairs=0) == 0
    assert lib.hg_ransac_refit_f32(None, None, 0, None, 0, None, None, None, None, None) == 0
    assert lib.hg_ransac_accept_f32(None, None, None, 0, None, 0, 1.0, None, None, None, None) == 0
    assert _refit(lib, pairs=0, total=-1) == INVALID       # scalars are checked first
    assert _accept(lib, pairs=0, total=1 << 31) == INVALID


def test_wrappers_refuse_host_tensors_and_bad_shapes(pkg):
    import torch
    ps, pt, mk = torch.zeros(10, 2), torch.zeros(10, 2), torch.ones(10, dtype=torch.uint8)
    with pytest.raises(ValueError, match="GPU only"):
        pkg.refit(ps, pt, mk)
    with pytest.raises(ValueError, match="GPU only"):
        pkg.refit(ps, pt, mk, pair_offsets=[0, 4, 10], return_f64=True)
    with pytest.raises(ValueError, match=r"\(npool,2\)"):
        pkg.refit(torch.zeros(10, 3), pt, mk)
    with pytest.raises(ValueError, match="same number"):
        pkg.refit(ps, torch.zeros(9, 2), mk)
    with pytest.raises(ValueError, match="mask"):
        pkg.refit(ps, pt, torch.ones(9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        pkg.refit(ps, pt, torch.ones(10, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask"):
        pkg.refit(ps, pt, torch.ones((10, 1), dtype=torch.uint8))
    with pytest.raises(ValueError, match="mask"):
        pkg.refit(ps, pt, [1] * 10)
    with pytest.raises(ValueError, match="pair_offsets"):
        pkg.refit(ps, pt, mk, pair_offsets=torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError, match="pair_offsets"):
        pkg.refit(ps, pt, mk, pair_offsets=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="refine"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, refine=-1)
    with pytest.raises(ValueError, match="refine"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, refine=1.5)
    with pytest.raises(ValueError, match="mask=True"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, mask=False, refine=1)
    with pytest.raises(ValueError, match="GPU only"):
        pkg.ransac_consensus(ps, pt, 16, 3.0, refine=2)
    assert pkg.RefitResult._fields == ("H", "used", "H64")
    assert pkg.ConsensusResult._fields == ("H", "inliers", "index", "mask")
