"""An independent restatement of the least-squares refit (hg_ransac_refit_f32), for the tests only.

The definition (include/sks_homography.h, "Least-squares refit of the consensus inliers"), in
numpy binary64, every operation rounded on its own, in the definition's fixed summation order:

    row i of the pair belongs to lane i % 256; a lane adds its rows in ascending order into
    +0.0, an unselected row adds +0.0; the 256 lane sums v are then combined by
        for d = 1, 2, 4, ..., 128:   v[l] <- v[l] + v[l xor d]

numpy's float64 array operations round each + - * / once (IEEE 754) and never fuse a multiply
with an add, as the HIP code does with contraction off, so the GPU's H64, H and `used` equal
``refit`` as bit patterns.  No code is shared with the implementation.

``refit(..., mutate=...)`` restates three deliberate mistakes (tests/test_refit_restatement.py
checks that the exact-arithmetic check catches each): "swap_ab" (a and b exchanged in Ly),
"s_inverted" (s = d / n), "no_scale" (the final 1 / H[8] left out).
"""
from __future__ import annotations

import numpy as np

LANES = 256
QNAN32 = 0x7FC00000
QNAN64 = 0x7FF8000000000000


def nan_result(n):
    H64 = np.full(9, QNAN64, np.uint64).view(np.float64)
    H = np.full(9, QNAN32, np.uint32).view(np.float32)
    return H, H64, np.int32(n)


def ordered_sum(terms: np.ndarray) -> np.ndarray:
    """terms: (m, K) binary64, unselected rows already +0.0 -> (K,) in the definition's order.
    Rows past m that pad the last step add +0.0 to an accumulator that is never -0.0 (it
    starts at +0.0, and a sum is -0.0 only when both operands are), so they change no bit."""
    m, K = terms.shape
    steps = -(-m // LANES)
    padded = np.zeros((max(steps, 1) * LANES, K), np.float64)
    padded[:m] = terms
    padded = padded.reshape(-1, LANES, K)
    v = np.zeros((LANES, K), np.float64)
    for step in range(padded.shape[0]):
        v = v + padded[step]
    lane = np.arange(LANES)
    d = 1
    while d < LANES:
        v = v + v[lane ^ d]
        d *= 2
    return v[0]


def ldlt_solve(A: np.ndarray, g: np.ndarray):
    """A h = g for the symmetric 8 x 8 A (its upper triangle is read) by LDL^T without pivoting,
    the recurrences of csrc/hg_refit.hpp operation by operation.  Returns (h, ok)."""
    L = np.zeros((8, 8), np.float64)
    D = np.zeros(8, np.float64)
    ok = True
    for j in range(8):
        v = [L[j, k] * D[k] for k in range(j)]
        dj = A[j, j]
        for k in range(j):
            dj = dj - L[j, k] * v[k]
        ok = ok and bool(dj > 0.0)
        D[j] = dj
        for i in range(j + 1, 8):
            t = A[j, i]
            for k in range(j):
                t = t - L[i, k] * v[k]
            L[i, j] = t / dj
    h = np.zeros(8, np.float64)
    for i in range(8):
        z = g[i]
        for k in range(i):
            z = z - L[i, k] * h[k]
        h[i] = z
    for i in range(8):
        h[i] = h[i] / D[i]
    for i in range(7, -1, -1):
        w = h[i]
        for k in range(i + 1, 8):
            w = w - L[k, i] * h[k]
        h[i] = w
    return h, ok


def normalisation(ps, pt, sel):
    """(n, c (4,), d (4,)) of the selected rows; c and d are None when n < 4."""
    pts = np.concatenate([ps, pt], axis=1).astype(np.float64)  # (m, 4): x, y, u, v
    n = int(np.count_nonzero(sel))
    if n < 4:
        return n, None, None
    zero = np.float64(0.0)
    c = ordered_sum(np.where(sel[:, None], pts, zero)) / np.float64(n)
    d = ordered_sum(np.where(sel[:, None], np.abs(pts - c), zero))
    return n, c, d


def refit(pool_src, pool_tar, mask, mutate=None, detail=False):
    """One pair: (H (9,) float32, H64 (9,) float64, used int32) of its (m,2) float32 pools and
    (m,) uint8 mask.  detail=True also returns (c, s) -- None for a pair that failed early."""
    ps = np.asarray(pool_src, np.float32).reshape(-1, 2)
    pt = np.asarray(pool_tar, np.float32).reshape(-1, 2)
    sel = np.asarray(mask).reshape(-1) != 0
    assert ps.shape == pt.shape and sel.shape[0] == ps.shape[0]

    def out(res, c=None, s=None):
        return res + ((c, s),) if detail else res

    with np.errstate(all="ignore"):
        n, c, d = normalisation(ps, pt, sel)
        if n < 4:
            return out(nan_result(n))
        nd = np.float64(n)
        s = d / nd if mutate == "s_inverted" else nd / d
        ok = not bool((d == 0.0).any())
        pts = np.concatenate([ps, pt], axis=1).astype(np.float64)
        q = (pts - c) * s
        X, Y, a, b = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, zero = np.ones_like(X), np.zeros_like(X)
        Lx = np.stack([X, Y, one, zero, zero, zero, -a * X, -a * Y, -a], axis=1)
        if mutate == "swap_ab":
            b = a
        Ly = np.stack([zero, zero, zero, X, Y, one, -b * X, -b * Y, -b], axis=1)
        jj, kk = np.triu_indices(9)
        terms = Lx[:, jj] * Lx[:, kk] + Ly[:, jj] * Ly[:, kk]
        tri = ordered_sum(np.where(sel[:, None], terms, np.float64(0.0)))
        LtL = np.zeros((9, 9), np.float64)
        LtL[jj, kk] = tri
        h8, piv = ldlt_solve(LtL[:8, :8], -LtL[:8, 8])
        ok = ok and piv
        h = np.concatenate([h8, [1.0]])
        i2, i3 = np.float64(1.0) / s[2], np.float64(1.0) / s[3]
        t0, t1 = -(c[0] * s[0]), -(c[1] * s[1])
        G = np.zeros(9, np.float64)
        F = np.zeros(9, np.float64)
        for k in range(3):
            G[k] = h[k] * i2 + c[2] * h[6 + k]
            G[3 + k] = h[3 + k] * i3 + c[3] * h[6 + k]
            G[6 + k] = h[6 + k]
        for r in range(3):
            F[3 * r] = G[3 * r] * s[0]
            F[3 * r + 1] = G[3 * r + 1] * s[1]
            F[3 * r + 2] = (G[3 * r] * t0 + G[3 * r + 1] * t1) + G[3 * r + 2]
        H64 = F.copy() if mutate == "no_scale" else F * (np.float64(1.0) / F[8])
        H = H64.astype(np.float32)
        if not (ok and np.isfinite(H64).all() and np.isfinite(H).all()):
            return out(nan_result(n), c, s)
        return out((H, H64, np.int32(n)), c, s)


def pair_rows(offsets, total):
    """[(lo, m)] of every pair: offsets clamped into [0, total], a descending step empty."""
    off = [min(max(int(v), 0), total) for v in offsets]
    return [(a, max(b - a, 0)) for a, b in zip(off, off[1:])]


def refit_pairs(pool_src, pool_tar, mask, offsets):
    """Every pair of a batched call: (H (pairs,9) f32, H64 (pairs,9) f64, used (pairs,) i32)."""
    res = [refit(pool_src[lo:lo + m], pool_tar[lo:lo + m], mask[lo:lo + m])
           for lo, m in pair_rows(offsets, pool_src.shape[0])]
    return (np.stack([r[0] for r in res]).reshape(-1, 9), np.stack([r[1] for r in res]).reshape(-1, 9),
            np.array([r[2] for r in res], np.int32))


# ------------------------------------------------------------------ exact rational arithmetic
def exact_solve(A, g):
    """A h = g over the rationals (Gauss-Jordan with any non-zero pivot); None when singular."""
    n = len(g)
    M = [list(A[i]) + [g[i]] for i in range(n)]
    for col in range(n):
        piv = next((r for r in range(col, n) if M[r][col] != 0), None)
        if piv is None:
            return None
        M[col], M[piv] = M[piv], M[col]
        inv = 1 / M[col][col]
        M[col] = [v * inv for v in M[col]]
        for r in range(n):
            if r != col and M[r][col] != 0:
                f = M[r][col]
                M[r] = [a - f * b for a, b in zip(M[r], M[col])]
    return [M[i][n] for i in range(n)]


def exact_refit(pool_src, pool_tar, mask, c, s):
    """The exact minimiser of the definition for the given binary64 c and s (taken as exact
    rationals): nine Fractions, H[8] = 1.  The normal equations are built and solved, and H is
    denormalised and scaled, without a rounding anywhere.  None when they are singular."""
    from fractions import Fraction as Fr
    sel = np.asarray(mask).reshape(-1) != 0
    rows = [[Fr(float(v)) for v in (*pool_src[i], *pool_tar[i])] for i in np.flatnonzero(sel)]
    cf, sf = [Fr(float(v)) for v in c], [Fr(float(v)) for v in s]
    LtL = [[Fr(0)] * 9 for _ in range(9)]
    for r in rows:
        X, Y, a, b = [(r[k] - cf[k]) * sf[k] for k in range(4)]
        Lx = [X, Y, Fr(1), Fr(0), Fr(0), Fr(0), -a * X, -a * Y, -a]
        Ly = [Fr(0), Fr(0), Fr(0), X, Y, Fr(1), -b * X, -b * Y, -b]
        for j in range(9):
            for k in range(9):
                LtL[j][k] += Lx[j] * Lx[k] + Ly[j] * Ly[k]
    h = exact_solve([row[:8] for row in LtL[:8]], [-LtL[i][8] for i in range(8)])
    if h is None:
        return None
    h = h + [Fr(1)]
    T2inv = [[1 / sf[2], 0, cf[2]], [0, 1 / sf[3], cf[3]], [0, 0, 1]]
    T1 = [[sf[0], 0, -cf[0] * sf[0]], [0, sf[1], -cf[1] * sf[1]], [0, 0, 1]]
    Hn = [h[0:3], h[3:6], h[6:9]]
    mul = lambda P, Q: [[sum(P[i][k] * Q[k][j] for k in range(3)) for j in range(3)] for i in range(3)]  # noqa: E731
    F = mul(mul(T2inv, Hn), T1)
    if F[2][2] == 0:
        return None
    return [F[i][j] / F[2][2] for i in range(3) for j in range(3)]


def exact_normalisation(pool_src, pool_tar, mask, c):
    """(c, s) of the definition as Fractions: the exact centroid, and n / sum |. - c| taken about
    the GIVEN binary64 c (the definition's d is a sum about the rounded centroid)."""
    from fractions import Fraction as Fr
    sel = np.asarray(mask).reshape(-1) != 0
    rows = [[Fr(float(v)) for v in (*pool_src[i], *pool_tar[i])] for i in np.flatnonzero(sel)]
    n = len(rows)
    ce = [sum(r[k] for r in rows) / n for k in range(4)]
    se = [Fr(n) / sum(abs(r[k] - Fr(float(c[k]))) for r in rows) for k in range(4)]
    return ce, se


def ulp32(v) -> "Fraction":
    """The spacing of binary32 at the magnitude of the rational v (2^-149 below the normals)."""
    from fractions import Fraction as Fr
    v = abs(Fr(v))
    if v == 0:
        return Fr(1, 2 ** 149)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fr(2) ** e > v:
        e -= 1                                    # 2^e <= v < 2^(e+1)
    e = max(e, -126)
    return Fr(2) ** (e - 23)
