"""The least-squares refit and the accept step (hg_ransac_refit_f32, hg_ransac_accept_f32,
pkg.refit, pkg.ransac_consensus(refine=R)) on the GPU.

The refit is defined operation by operation, summation order included
(include/sks_homography.h), so there is no tolerance: H64, H and `used` equal the numpy
restatement (tests/restate_refit.py, tied to exact arithmetic by
tests/test_refit_restatement.py) as integer bit patterns; a failed pair is nine canonical quiet
NaNs on both sides.  The accept step equals its composition from ransac_score, inlier_mask and
the >= rule, byte for byte.

Sizes (csrc/hg_refit.hpp): one block of 256 lanes per pair, a lane owns rows l, l + 256, ...;
pools of 0 ... 5 rows (fewer than four, exactly four, one more), 63 / 64 / 65 (a wave), 255 / 256
/ 257 (one step of the block and its first wrap), 1000, the wall file and 20 000 (79 steps).
"""
import functools

import numpy as np
import pytest
import torch

import restate_refit as rr
from conftest import load_golden
from test_gpu_extents import F32, F64, I32, Arena, Checks, fresh_vs_arena
from test_refit_restatement import failure_cases

pytestmark = pytest.mark.gpu

QNAN = 0x7FC00000
H_TRUE = np.array([[0.92, -0.11, 31.0], [0.08, 1.05, -12.0], [1.1e-4, -6.0e-5, 1.0]])


# ---------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def _model_pool(npool, seed=0):
    """Correspondences of one homography with 0.7 px noise, three rows in ten replaced by
    uniform outliers: a consensus finds the model, so its mask selects most rows."""
    g = np.random.default_rng(100 * seed + npool)
    ps = g.random((npool, 2)) * 1000
    q = np.concatenate([ps, np.ones((npool, 1))], axis=1) @ H_TRUE.T
    pt = q[:, :2] / q[:, 2:] + g.normal(0, 0.7, (npool, 2))
    out = g.random(npool) < 0.3
    pt[out] = g.random((int(out.sum()), 2)) * 1000
    return ps.astype(np.float32), pt.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _wall():
    g = load_golden("cpp_wall.npz")
    return g["pool_src"], g["pool_tar"]


def _pool(npool):
    return _wall() if npool == 2540 else _model_pool(npool)


def _dev(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _i32(x):
    return x.contiguous().view(torch.int32)


def _same(res, want, label):
    """RefitResult (device) against the restatement's (H, H64, used) as bit patterns."""
    H, H64, used = want
    got_h = res.H.cpu().numpy().reshape(-1, 9).view(np.uint32)
    got_h64 = res.H64.cpu().numpy().reshape(-1, 9).view(np.uint64)
    got_used = res.used.cpu().numpy()
    assert np.array_equal(got_used, np.asarray(used, np.int32).reshape(-1)), f"{label}: used"
    want_h64 = np.asarray(H64, np.float64).reshape(-1, 9).view(np.uint64)
    assert np.array_equal(got_h64, want_h64), (
        f"{label}: {(got_h64 != want_h64).sum()} H64 elements differ from the restatement")
    assert np.array_equal(got_h, np.asarray(H, np.float32).reshape(-1, 9).view(np.uint32)), f"{label}: H"


# ------------------------------------------------------------------ one pair, every mask kind
@pytest.mark.parametrize("npool", [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000, 2540, 20_000])
def test_one_pair_equals_the_restatement(pkg, dev, npool):
    ps, pt = _pool(npool)
    dps, dpt = _dev(dev, ps, pt)
    g = np.random.default_rng(npool)
    four = np.zeros(npool, np.uint8)
    four[g.choice(npool, min(4, npool), replace=False)] = 1
    masks = {
        "all ones": np.ones(npool, np.uint8),
        "all zero": np.zeros(npool, np.uint8),
        "exactly 4": four,
        "every other row": (np.arange(npool) % 2 == 0).astype(np.uint8),
        "bytes 1, 2, 255": g.choice(np.array([1, 2, 255], np.uint8), npool),
    }
    if npool:
        cons = pkg.ransac_consensus(dps, dpt, 500, 3.0, seed=11)
        masks["consensus"] = cons.mask.cpu().numpy()
        if npool >= 63:
            assert int(cons.inliers[0].item()) > npool // 3, "the consensus found no model"
    fitted = 0
    for name, mask in masks.items():
        (dm,) = _dev(dev, mask)
        res = pkg.refit(dps, dpt, dm, return_f64=True)
        assert res.H.shape == (1, 9) and res.H.dtype == torch.float32
        assert res.H64.shape == (1, 9) and res.H64.dtype == torch.float64
        assert res.used.shape == (1,) and res.used.dtype == torch.int32
        want = rr.refit(ps, pt, mask)
        _same(res, want, f"npool {npool}, {name}")
        assert int(want[2]) == int(np.count_nonzero(mask))
        fitted += int(np.isfinite(want[0]).all())
        no64 = pkg.refit(dps, dpt, dm)
        assert no64.H64 is None and torch.equal(_i32(no64.H), _i32(res.H))
    if npool >= 63:  # the cases are not all failures: every mask but the empty one fits
        assert fitted == len(masks) - 1, (npool, fitted)


def test_failure_cases_give_nans(pkg, dev):
    for name, (ps, pt, mask, n) in failure_cases().items():
        dps, dpt, dm = _dev(dev, ps, pt, mask)
        res = pkg.refit(dps, dpt, dm, return_f64=True)
        assert _i32(res.H).tolist() == [[QNAN] * 9], name
        assert res.H64.view(torch.int64).tolist() == [[rr.QNAN64] * 9], name
        assert int(res.used[0].item()) == n, name
        _same(res, rr.refit(ps, pt, mask), name)


def test_unselected_rows_do_not_matter(pkg, dev):
    """NaN and Inf in rows the mask leaves out change no bit (a row is selected, not weighted)."""
    ps, pt = _model_pool(1000)
    mask = (np.random.default_rng(3).random(1000) < 0.6).astype(np.uint8)
    js, jt = ps.copy(), pt.copy()
    js[mask == 0] = np.nan
    jt[mask == 0] = np.inf
    a = pkg.refit(*_dev(dev, ps, pt, mask), return_f64=True)
    b = pkg.refit(*_dev(dev, js, jt, mask), return_f64=True)
    assert torch.isfinite(a.H64).all()
    assert torch.equal(a.H64.view(torch.int64), b.H64.view(torch.int64))


# ------------------------------------------------------------------------------ batched pairs
SIZES = {1: [2540], 3: [65, 0, 700],
         33: [700, 1, 4, 65, 3000, 257, 0, 4, 700, 65, 1, 256, 5, 65, 700, 1,
              0,  # the empty pair in the middle
              3000, 65, 4, 3, 700, 255, 65, 0, 1, 4, 700, 65, 1000, 1, 4, 3000]}


@functools.lru_cache(maxsize=None)
def _batch(pairs):
    """Ragged pairs back to back, each its own model pool; a random mask of bytes 0 / 1 / 7."""
    sizes = SIZES[pairs]
    assert len(sizes) == pairs
    pools = [_model_pool(m, seed=j + 1) for j, m in enumerate(sizes)]
    ps = np.concatenate([p[0] for p in pools]).astype(np.float32).reshape(-1, 2)
    pt = np.concatenate([p[1] for p in pools]).astype(np.float32).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    g = np.random.default_rng(pairs)
    mask = g.choice(np.array([0, 1, 1, 7], np.uint8), ps.shape[0])
    return ps, pt, off, mask


@pytest.mark.parametrize("pairs", [1, 3, 33])
def test_batched_pairs_equal_single_pair_calls(pkg, dev, pairs):
    """A pair's result does not depend on its neighbours, on `pairs` or on the grid: each pair
    of one batched call equals the single-pair call on its slice, and the restatement."""
    ps, pt, off, mask = _batch(pairs)
    dps, dpt, dm = _dev(dev, ps, pt, mask)
    res = pkg.refit(dps, dpt, dm, pair_offsets=off.tolist(), return_f64=True)
    on_dev = pkg.refit(dps, dpt, dm, pair_offsets=torch.from_numpy(off).to(dev), return_f64=True)
    for a, b in zip(res, on_dev):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    _same(res, rr.refit_pairs(ps, pt, mask, off), f"{pairs} pairs")
    for j in range(pairs):
        lo, hi = int(off[j]), int(off[j + 1])
        one = pkg.refit(dps[lo:hi], dpt[lo:hi], dm[lo:hi], return_f64=True)
        assert torch.equal(one.H64.view(torch.int64)[0], res.H64.view(torch.int64)[j]), j
        assert torch.equal(_i32(one.H)[0], _i32(res.H)[j]) and int(one.used[0]) == int(res.used[j]), j
        if hi == lo:
            assert _i32(res.H)[j].tolist() == [QNAN] * 9 and int(res.used[j]) == 0
    assert torch.isfinite(res.H).all(dim=1).sum().item() >= sum(m >= 65 for m in SIZES[pairs])


def _refit_call(pkg, dev, dps, dpt, off_dev, pairs, dm, H, H64, used):
    pkg._lib.call("hg_ransac_refit_f32", dps.data_ptr(), dpt.data_ptr(), dps.shape[0],
                  off_dev.data_ptr(), pairs, dm.data_ptr(), H, H64, used,
                  torch.cuda.current_stream(dev).cuda_stream)


def _accept_call(pkg, dev, H_new, dps, dpt, off_dev, pairs, thresh, H, count, mask):
    pkg._lib.call("hg_ransac_accept_f32", H_new.data_ptr(), dps.data_ptr(), dpt.data_ptr(),
                  dps.shape[0], off_dev.data_ptr(), pairs, thresh, H, count, mask,
                  torch.cuda.current_stream(dev).cuda_stream)


def test_offsets_are_clamped(pkg, dev):
    """Offsets below 0, a descending step and a last entry beyond total are clamped on the
    device as the consensus clamps them (the descending step is an empty pair); nothing is
    written outside the outputs and the inputs are untouched."""
    total = 1000
    ps, pt = _model_pool(total)
    mask = np.random.default_rng(4).choice(np.array([0, 1, 255], np.uint8), total)
    dps, dpt, dm = _dev(dev, ps, pt, mask)
    raw = [-7, 400, 900, 600, 5000]
    pairs = len(raw) - 1
    off_dev = torch.tensor(raw, dtype=torch.int64, device=dev)
    aH, a64, au = Arena(dev, pairs * 36, 4), Arena(dev, pairs * 72, 8), Arena(dev, pairs * 4, 4)
    keep = [dps.clone(), dpt.clone(), dm.clone(), off_dev.clone()]
    _refit_call(pkg, dev, dps, dpt, off_dev, pairs, dm, aH.ptr(), a64.ptr(), au.ptr())
    H, H64, used = rr.refit_pairs(ps, pt, mask, raw)
    assert used.tolist() == [int(np.count_nonzero(mask[a:a + m])) for a, m in
                             [(0, 400), (400, 500), (900, 0), (600, 400)]]
    ck = Checks()
    ck.outputs("clamped H", aH, _dev(dev, H))
    ck.outputs("clamped H64", a64, _dev(dev, H64))
    ck.outputs("clamped used", au, _dev(dev, used))
    ck.inputs("clamped", [dps, dpt, dm, off_dev], keep)
    ck.verify()


# ---------------------------------------------------------------- four points against solve()
def test_four_rows_agree_with_the_closed_form_solver(pkg, dev):
    """A 4-row pool has one homography: the refit and solve("aca") on the same four points
    both lie within one binary32 ulp of it, element by element, the exact value computed in
    Fractions.  The four points have small integer coordinates (at most 5 bits), because the
    closed-form solver works in binary32 throughout and a one-ulp bound on its result holds
    only where its products and differences are exact or nearly so (on four wall-file rows it
    is 117 ulp away; the refit, in binary64, is within half an ulp there too), and they are in
    general position, so no element of the exact H is zero (a zero has no ulp to be within)."""
    from fractions import Fraction
    ps = np.array([[1, 2], [9, 1], [10, 9], [2, 10]], np.float32)
    pt = np.array([[3, 1], [20, 4], [17, 15], [4, 12]], np.float32)
    ones = np.ones(4, np.uint8)
    _, _, _, (c, s) = rr.refit(ps, pt, ones, detail=True)
    want = rr.exact_refit(ps, pt, ones, c, s)
    assert all(w != 0 for w in want) and want[8] == 1
    dps, dpt, dm = _dev(dev, ps, pt, ones)
    fit = pkg.refit(dps, dpt, dm).H[0].cpu().numpy()
    aca = pkg.solve("aca", dps.reshape(1, 8), dpt.reshape(1, 8), normalize=True)[0].cpu().numpy()
    for name, got in (("refit", fit), ("aca", aca)):
        for k in range(9):
            err = abs(Fraction(float(got[k])) - want[k]) / rr.ulp32(want[k])
            print(f"{name} H[{k}] {float(err):.3f} ulp")
            assert err <= 1, f"{name} H[{k}] = {got[k]!r}: {float(err):.3g} ulp from {float(want[k])!r}"


# ---------------------------------------------------------------------------------- accept
def _compose_accept(pkg, dps, dpt, off, thresh, H_new, H, count, mask):
    """hg_ransac_accept_f32 from existing pieces, pair by pair, the >= rule on the host.
    Returns (H, count, mask, accepted) as new tensors / a list."""
    H, count, mask = H.clone(), count.clone(), mask.clone()
    accepted = []
    new_host = H_new.cpu().numpy()
    for j, (lo, m) in enumerate(rr.pair_rows(off, dps.shape[0])):
        c = int(pkg.ransac_score(H_new[j], dps[lo:lo + m], dpt[lo:lo + m], thresh)[0].item()) if m else 0
        ok = bool(np.isfinite(new_host[j]).all()) and c >= int(count[j].item())
        accepted.append(ok)
        if ok:
            H[j] = H_new[j]
            count[j] = c
            if m:
                mask[lo:lo + m] = pkg.inlier_mask(H_new[j], dps[lo:lo + m], dpt[lo:lo + m], thresh)
    return H, count, mask, accepted


def test_accept_equals_its_composition(pkg, dev):
    """Pairs with the refitted H, a pair where the new H loses (the held one moved by 50 px:
    its outputs stay byte for byte), NaN and Inf in H_new, an empty pair, and a tie (H_new =
    the held H: count equal, accepted)."""
    sizes = [700, 65, 0, 3000, 257, 700, 1000]
    pools = [_model_pool(m, seed=40 + j) for j, m in enumerate(sizes)]
    ps = np.concatenate([p[0] for p in pools]).reshape(-1, 2)
    pt = np.concatenate([p[1] for p in pools]).reshape(-1, 2)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    dps, dpt = _dev(dev, ps, pt)
    off_dev = torch.from_numpy(off).to(dev)
    thresh, pairs = 3.0, len(sizes)
    base = pkg.ransac_consensus(dps, dpt, 500, thresh, pair_offsets=off_dev, seed=3)
    H_new = pkg.refit(dps, dpt, base.mask, pair_offsets=off_dev).H.clone()
    H_new[1] = base.H[1]
    H_new[1, 2] += 50.0                   # loses: every inlier moves 50 px
    H_new[3, 4] = float("nan")
    H_new[4, 0] = float("inf")
    H_new[5] = base.H[5]                  # a tie
    want_H, want_c, want_m, accepted = _compose_accept(pkg, dps, dpt, off, thresh, H_new, base.H,
                                                       base.inliers, base.mask)
    assert accepted[1:6] == [False, False, False, False, True], accepted
    assert accepted[0] or accepted[6], "no refitted H was accepted: the winning branch is not run"
    H, count, mask = base.H.clone(), base.inliers.clone(), base.mask.clone()
    _accept_call(pkg, dev, H_new, dps, dpt, off_dev, pairs, thresh, H.data_ptr(), count.data_ptr(),
                 mask.data_ptr())
    assert torch.equal(_i32(H), _i32(want_H))
    assert torch.equal(count, want_c) and torch.equal(mask, want_m)
    for j in (1, 2, 3, 4):                # untouched, byte for byte
        lo, hi = int(off[j]), int(off[j + 1])
        assert torch.equal(_i32(H[j]), _i32(base.H[j])) and int(count[j]) == int(base.inliers[j])
        assert torch.equal(mask[lo:hi], base.mask[lo:hi])
    for j in (0, 5, 6):
        if accepted[j]:
            assert int(count[j]) >= int(base.inliers[j]) and torch.equal(_i32(H[j]), _i32(H_new[j]))
    for j in range(pairs):
        lo, hi = int(off[j]), int(off[j + 1])
        assert int(mask[lo:hi].sum().item()) == int(count[j].item()), j


# ------------------------------------------------------------------- ransac_consensus(refine)
def _check_refine(pkg, dps, dpt, off, thresh, kw):
    off_list = [int(v) for v in off]
    plain = pkg.ransac_consensus(dps, dpt, 1000, thresh, pair_offsets=off_list, **kw)
    r = [pkg.ransac_consensus(dps, dpt, 1000, thresh, pair_offsets=off_list, refine=R, **kw)
         for R in (0, 1, 2)]
    for a, b in zip(plain, r[0]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "refine=0 differs"
    rose = 0
    for prev, cur in zip(r, r[1:]):
        assert torch.equal(cur.index, plain.index)
        assert (cur.inliers >= prev.inliers).all(), "a round lowered an inlier count"
        fit = pkg.refit(dps, dpt, prev.mask, pair_offsets=off_list)
        want_H, want_c, want_m, accepted = _compose_accept(pkg, dps, dpt, off_list, thresh, fit.H,
                                                           prev.H, prev.inliers, prev.mask)
        assert torch.equal(_i32(cur.H), _i32(want_H)) and torch.equal(cur.inliers, want_c)
        assert torch.equal(cur.mask, want_m)
        for j, (lo, m) in enumerate(rr.pair_rows(off_list, dps.shape[0])):
            assert torch.equal(_i32(cur.H[j]), _i32(fit.H[j] if accepted[j] else prev.H[j])), j
            assert int(cur.mask[lo:lo + m].sum().item()) == int(cur.inliers[j].item()), j
        rose += int((cur.inliers > prev.inliers).sum().item())
    return r, rose


def test_refine_on_the_wall_file(pkg, dev):
    ps, pt = _wall()
    dps, dpt = _dev(dev, ps, pt)
    for algo in ("aca", "sks"):
        r, rose = _check_refine(pkg, dps, dpt, [0, ps.shape[0]], 3.0, dict(seed=11, algo=algo))
        print(algo, "inliers by round:", [int(x.inliers[0].item()) for x in r])
        assert rose >= 1, "no round raised the wall file's inlier count"


def test_refine_on_ragged_pairs(pkg, dev):
    ps, pt, off, _ = _batch(33)
    dps, dpt = _dev(dev, ps, pt)
    r, rose = _check_refine(pkg, dps, dpt, off, 3.0, dict(seed=11, offset=6))
    assert rose >= 1
    on_dev = pkg.ransac_consensus(dps, dpt, 1000, 3.0, pair_offsets=torch.from_numpy(off).to(dev),
                                  seed=11, offset=6, refine=2)
    for a, b in zip(r[2], on_dev):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("offs", [(0, 0, 0, 0), (4, 8, 4, 1), (8, 0, 8, 4), (4, 8, 8, 8)])
def test_outputs_under_guard_bands(pkg, dev, offs):
    """H, H64, used of the refit and H_io, count_io, mask_io of the accept step as arena
    payloads at byte offsets 0, +4 and +8 (H64: 0 and +8; the mask also +1): the guards keep
    0xA5, the payloads equal the plain call's, the inputs are untouched."""
    oH, o64, ou, om = offs
    ps, pt, off, mask = _batch(33)
    pairs, total = len(off) - 1, ps.shape[0]
    dps, dpt, dm = _dev(dev, ps, pt, mask)
    off_dev = torch.from_numpy(off).to(dev)
    ck = Checks()
    for with64 in (True, False):
        fresh_vs_arena(
            ck, f"refit {offs} H64 {with64}", pkg, dev, "hg_ransac_refit_f32",
            lambda p: (dps.data_ptr(), dpt.data_ptr(), total, off_dev.data_ptr(), pairs,
                       dm.data_ptr(), p["H"], p["H64"], p["used"]),
            outs={"H": (pairs * 9, F32), "H64": (pairs * 9, F64) if with64 else None,
                  "used": (pairs, I32)},
            offsets={"H": oH, "H64": o64, "used": ou}, inputs=(dps, dpt, dm, off_dev))
    base = pkg.ransac_consensus(dps, dpt, 500, 3.0, pair_offsets=off_dev, seed=3)
    H_new = pkg.refit(dps, dpt, base.mask, pair_offsets=off_dev).H.clone()
    H_new[3] = base.H[3]
    H_new[3, 2] += 50.0                                      # a pair that keeps what it holds
    H, count, m = base.H.clone(), base.inliers.clone(), base.mask.clone()
    _accept_call(pkg, dev, H_new, dps, dpt, off_dev, pairs, 3.0, H.data_ptr(), count.data_ptr(),
                 m.data_ptr())
    assert not torch.equal(count, base.inliers)              # the call changes something
    aH = Arena(dev, pairs * 36, oH).put(base.H)
    ac = Arena(dev, pairs * 4, ou).put(base.inliers)
    am = Arena(dev, total, om).put(base.mask)
    keep = [H_new.clone(), dps.clone(), dpt.clone(), off_dev.clone()]
    _accept_call(pkg, dev, H_new, dps, dpt, off_dev, pairs, 3.0, aH.ptr(), ac.ptr(), am.ptr())
    ck.outputs(f"accept {offs} H_io", aH, [H])
    ck.outputs(f"accept {offs} count_io", ac, [count])
    ck.outputs(f"accept {offs} mask_io", am, [m])
    ck.inputs(f"accept {offs}", [H_new, dps, dpt, off_dev], keep)
    ck.verify()


# ------------------------------------------------------------------- graph capture, determinism
def test_refit_and_accept_in_a_graph(pkg, dev):
    """The two C calls of a round, and then the whole pkg.ransac_consensus(refine=2), captured
    on a side stream (nothing allocated by the entries, no synchronisation) and replayed twice
    give the eager call's bytes both times."""
    ps, pt, off, _ = _batch(33)
    pairs, total = len(off) - 1, ps.shape[0]
    dps, dpt = _dev(dev, ps, pt)
    off_dev = torch.from_numpy(off).to(dev)
    base = pkg.ransac_consensus(dps, dpt, 1000, 3.0, pair_offsets=off_dev, seed=11, offset=6)
    want = pkg.ransac_consensus(dps, dpt, 1000, 3.0, pair_offsets=off_dev, seed=11, offset=6, refine=1)
    want2 = pkg.ransac_consensus(dps, dpt, 1000, 3.0, pair_offsets=off_dev, seed=11, offset=6, refine=2)
    H, count, mask = base.H.clone(), base.inliers.clone(), base.mask.clone()
    H_new = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
    H64 = torch.empty((pairs, 9), dtype=torch.float64, device=dev)
    used = torch.empty(pairs, dtype=torch.int32, device=dev)

    def run():
        _refit_call(pkg, dev, dps, dpt, off_dev, pairs, mask, H_new.data_ptr(), H64.data_ptr(),
                    used.data_ptr())
        _accept_call(pkg, dev, H_new, dps, dpt, off_dev, pairs, 3.0, H.data_ptr(), count.data_ptr(),
                     mask.data_ptr())

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run()
        whole = torch.cuda.CUDAGraph()
        with torch.cuda.graph(whole, stream=s):
            res = pkg.ransac_consensus(dps, dpt, 1000, 3.0, pair_offsets=off_dev, seed=11, offset=6,
                                       refine=2)
    torch.cuda.current_stream(dev).wait_stream(s)
    fit = pkg.refit(dps, dpt, base.mask, pair_offsets=off_dev, return_f64=True)
    for _ in range(2):
        H.copy_(base.H), count.copy_(base.inliers), mask.copy_(base.mask)
        H_new.fill_(7), H64.fill_(7), used.fill_(7)
        g.replay()
        torch.cuda.synchronize(dev)
        for got, w in ((H, want.H), (count, want.inliers), (mask, want.mask), (H_new, fit.H),
                       (H64, fit.H64), (used, fit.used)):
            assert torch.equal(got.view(torch.uint8), w.view(torch.uint8))
        for t in res:
            t.fill_(9)
        whole.replay()
        torch.cuda.synchronize(dev)
        for got, w in zip(res, want2):
            assert torch.equal(got.view(torch.uint8), w.view(torch.uint8))


def test_two_calls_give_identical_bytes(pkg, dev):
    ps, pt, off, mask = _batch(33)
    dps, dpt, dm = _dev(dev, ps, pt, mask)
    a = pkg.refit(dps, dpt, dm, pair_offsets=off.tolist(), return_f64=True)
    b = pkg.refit(dps, dpt, dm, pair_offsets=off.tolist(), return_f64=True)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    big_s, big_t = _model_pool(20_000)
    dbs, dbt = _dev(dev, big_s, big_t)
    for algo in ("aca", "sks"):
        x = pkg.ransac_consensus(dbs, dbt, 2000, 3.0, algo=algo, refine=2)
        y = pkg.ransac_consensus(dbs, dbt, 2000, 3.0, algo=algo, refine=2)
        for p, q in zip(x, y):
            assert torch.equal(p.view(torch.uint8), q.view(torch.uint8))
