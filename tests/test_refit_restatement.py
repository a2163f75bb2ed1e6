"""The numpy restatement of the least-squares refit (tests/restate_refit.py) against exact
rational arithmetic.  CPU only; tests/test_gpu_refit.py then pins the kernel to the restatement
bit for bit, so this file is what ties the kernel's bits to the mathematics.

For wall-file rows selected by a seeded mask (4, 5, 16, 64 and 300 of the 2540), the
restatement's own binary64 c and s are taken as exact rationals; the normal equations are built
and solved, and H denormalised and scaled, in ``fractions.Fraction``.  Then
  * c and s agree with the exact centroid and the exact n / sum |. - c| to 2^-44 relative (each
    is a sum of at most 300 binary64 terms and one division: a few hundred roundings of 2^-53);
  * every element of the binary32 H lies within one binary32 ulp of the exact value.
Three mutations of the restatement (a / b swapped in Ly, s = d / n, the final 1 / H[8] left
out) must each fail that check, and the failure cases of the definition return NaNs.

Measured here (x86-64, numpy binary64), largest |H64 - exact| / |exact| over the nine elements:
    4 rows 5.1e-12,  5 rows 5.2e-15,  16 rows 1.3e-14,  64 rows 4.7e-16,  300 rows 6.2e-16
(half a binary32 ulp is 3e-8 to 6e-8 relative: four decades above).
"""
from fractions import Fraction

import numpy as np
import pytest

import restate_refit as rr
from conftest import load_golden

COUNTS = (4, 5, 16, 64, 300)
REL_CS = Fraction(1, 2 ** 44)


def _wall():
    g = load_golden("cpp_wall.npz")
    return g["pool_src"], g["pool_tar"]


def _seeded_mask(total, count, seed=2024):
    mask = np.zeros(total, np.uint8)
    mask[np.random.default_rng(seed + count).choice(total, count, replace=False)] = 1
    return mask


def check_against_exact(ps, pt, mask, H, H64, c, s):
    """Raises AssertionError unless (c, s) are the definition's and H is within one binary32 ulp
    of the exact minimiser for them.  Returns the largest relative error of H64."""
    ce, se = rr.exact_normalisation(ps, pt, mask, c)
    for k in range(4):
        assert abs(Fraction(float(c[k])) - ce[k]) <= REL_CS * abs(ce[k]), f"c[{k}]"
        assert abs(Fraction(float(s[k])) - se[k]) <= REL_CS * abs(se[k]), f"s[{k}]"
    want = rr.exact_refit(ps, pt, mask, c, s)
    assert want is not None, "the exact normal equations are singular"
    assert np.isfinite(H).all() and np.isfinite(H64).all()
    worst = 0.0
    for k in range(9):
        err = abs(Fraction(float(H[k])) - want[k])
        assert err <= rr.ulp32(want[k]), (f"H[{k}] = {H[k]!r} is {float(err / rr.ulp32(want[k])):.3g} "
                                          f"binary32 ulp from {float(want[k])!r}")
        if want[k] != 0:
            worst = max(worst, float(abs(Fraction(float(H64[k])) - want[k]) / abs(want[k])))
    return worst


@pytest.mark.parametrize("count", COUNTS)
def test_restatement_within_one_ulp_of_exact(count):
    ps, pt = _wall()
    mask = _seeded_mask(ps.shape[0], count)
    H, H64, used, (c, s) = rr.refit(ps, pt, mask, detail=True)
    assert int(used) == count and H.dtype == np.float32 and H64.dtype == np.float64
    assert H[8] == np.float32(1.0)
    assert np.array_equal(H.view(np.uint32), H64.astype(np.float32).view(np.uint32))
    worst = check_against_exact(ps, pt, mask, H, H64, c, s)
    print(f"{count} rows: largest relative error of H64 {worst:.3g}")
    assert worst < 1e-9


@pytest.mark.parametrize("mutate", ["swap_ab", "s_inverted", "no_scale"])
@pytest.mark.parametrize("count", [5, 64])
def test_mutations_fail_the_exact_check(mutate, count):
    ps, pt = _wall()
    mask = _seeded_mask(ps.shape[0], count)
    H, H64, _, (c, s) = rr.refit(ps, pt, mask, mutate=mutate, detail=True)
    with pytest.raises(AssertionError):
        check_against_exact(ps, pt, mask, H, H64, c, s)


def test_any_non_zero_byte_selects_and_unselected_rows_do_not_matter():
    ps, pt = _wall()
    mask = _seeded_mask(ps.shape[0], 64)
    want = rr.refit(ps, pt, mask)
    other = mask.copy()
    other[other != 0] = np.resize(np.array([2, 255, 1, 128], np.uint8), 64)
    got = rr.refit(ps, pt, other)
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
    junk_s, junk_t = ps.copy(), pt.copy()
    junk_s[mask == 0] = np.nan                      # an unselected row adds +0.0, whatever it holds
    junk_t[mask == 0] = np.inf
    got = rr.refit(junk_s, junk_t, mask)
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


def _is_nan_result(res, n):
    H, H64, used = res
    return (H.view(np.uint32).tolist() == [rr.QNAN32] * 9
            and H64.view(np.uint64).tolist() == [rr.QNAN64] * 9 and int(used) == n)


def failure_cases():
    """{name: (pool_src, pool_tar, mask, n)}: every way the definition fails (also run on the
    GPU by tests/test_gpu_refit.py)."""
    ps, pt = _wall()
    ps, pt = ps[:40].copy(), pt[:40].copy()
    ones = np.ones(40, np.uint8)
    three = np.zeros(40, np.uint8)
    three[[3, 17, 30]] = 1
    same_s, same_t = np.repeat(ps[:1], 40, axis=0), np.repeat(pt[:1], 40, axis=0)
    col_s = ps.copy()
    col_s[:, 0] = 321.5                              # every selected x equal: d0 = 0
    line_s = ps.copy()
    line_s[:, 1] = 2.0 * line_s[:, 0] + 1.0          # collinear source points: a pivot is not > 0
    nan_s = ps.copy()
    nan_s[7, 0] = np.nan                             # a selected NaN: a non-finite output
    inf_s, inf_t, nan_t = ps.copy(), pt.copy(), pt.copy()
    inf_s[11, 1], inf_t[9, 1], nan_t[39, 0] = np.inf, -np.inf, np.nan
    return {
        "selected Inf in src": (inf_s, pt, ones, 40),
        "selected Inf in tar": (ps, inf_t, ones, 40),
        "selected NaN in tar": (ps, nan_t, ones, 40),
        "empty": (ps[:0], pt[:0], ones[:0], 0),
        "none selected": (ps, pt, np.zeros(40, np.uint8), 0),
        "n = 3": (ps, pt, three, 3),
        "identical rows": (same_s, same_t, ones, 40),
        "equal x": (col_s, pt, ones, 40),
        "collinear source": (line_s, pt, ones, 40),
        "selected NaN": (nan_s, pt, ones, 40),
    }


@pytest.mark.parametrize("name", list(failure_cases()))
def test_failure_cases_return_nans(name):
    ps, pt, mask, n = failure_cases()[name]
    assert _is_nan_result(rr.refit(ps, pt, mask), n), name


def test_the_failure_cases_fail_for_the_stated_reason():
    cases = failure_cases()
    ps, pt, mask, _ = cases["equal x"]
    _, _, d = rr.normalisation(ps, pt, mask != 0)
    assert d[0] == 0.0 and (d[1:] > 0).all()
    ps, pt, mask, _ = cases["identical rows"]
    assert (rr.normalisation(ps, pt, mask != 0)[2] == 0.0).all()
    ps, pt, mask, _ = cases["collinear source"]
    _, c, d = rr.normalisation(ps, pt, mask != 0)
    assert (d > 0).all()                             # the normalisation is fine: the solve fails
    ok_s = ps.copy()
    ok_s[:, 1] += np.linspace(0, 50, 40, dtype=np.float32) ** 2
    assert not _is_nan_result(rr.refit(ok_s, pt, mask), 40)


def test_summation_order_is_the_lane_butterfly():
    """ordered_sum against the order read literally: 256 lane sums in Python floats, rows in
    ascending order, then the xor-butterfly."""
    rng = np.random.default_rng(5)
    for m in (1, 255, 256, 257, 1000):
        t = (rng.standard_normal((m, 2)) * 10.0 ** rng.integers(-8, 8, (m, 2)))
        lanes = [[0.0, 0.0] for _ in range(256)]
        for i in range(m):
            for k in range(2):
                lanes[i % 256][k] = lanes[i % 256][k] + float(t[i, k])
        d = 1
        while d < 256:
            lanes = [[lanes[q][k] + lanes[q ^ d][k] for k in range(2)] for q in range(256)]
            d *= 2
        assert all(row == lanes[0] for row in lanes)          # every lane ends with the same bits
        assert rr.ordered_sum(t).tolist() == lanes[0]


def test_batched_restatement_clamps_offsets():
    assert rr.pair_rows([-7, 400, 900, 600, 5000], 1000) == [(0, 400), (400, 500), (900, 0), (600, 400)]
