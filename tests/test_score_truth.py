"""The inlier scorer against exact arithmetic.

hg_ransac_score_f32 is the project's own definition (the reference has no scorer), and its
other checks compare it with oracle_ransac_score_f32, a restatement with the same FMA
placement.  Here both meet the definition of include/sks_homography.h stated once more with
no rounding in it: plain numpy in np.longdouble, whose 64-bit significand holds every product
of two binary32 values exactly, so the sums below carry ~2^-63 relative error against the
binary32 rounding (2^-24) they judge.

For hypothesis H and pair (x, y) -> (u, v), all taken as the exact binary32 values given:
    x' = h0 x + h1 y + h2,  y' = h3 x + h4 y + h5,  w' = h6 x + h7 y + h8
    e2 = (x' - u w')^2 + (y' - v w')^2,   lim = fl32(t t) w'^2
    inlier  iff  w' != 0 and e2 <= lim.

The scorer rounds in binary32, so a pair is checked only where the exact margin exceeds the
rounding the kernel is allowed.  With r = 2^-24, Sx = |h0 x| + |h1 y| + |h2| (Sy, Sw alike):
    Ex = 2r (Sx + |u| Sw) + r |x' - u w'|        two nested FMAs per projection, one for ex
    de = 2|ex|Ex + Ex^2 + 2|ey|Ey + Ey^2 + 2r (e2 + 2|ex|Ex + 2|ey|Ey)
    dl = t^2 (4r |w'| Sw + (2r Sw)^2) + 2r (1 + 4r) lim
and a pair is UNDECIDED when |e2 - lim| <= de + dl.  Every decided pair must agree, which per
hypothesis is  decided_inliers <= count <= decided_inliers + undecided.  The share of undecided
pairs is capped at 1e-4 of all pairs: a condition on the inputs (that the test decides nearly
everything), not a tolerance.

Measured undecided shares (1024 ACA hypotheses of seed 11 on cpp_wall.npz's 2540-pair pool; the
oracle's hypotheses on the CPU and the fused sampler's on the MI355X are the same bits, and the
two runs gave the same figures):
    threshold 0.5 px:  32 of 2 588 260 pairs (1.24e-5), 5 hypotheses of 1024 left out
    threshold 3.0 px:   9 of 2 588 260 pairs (3.48e-6), 5 hypotheses of 1024 left out
    planted pool, 3.0 px (MI355X): 1 of 1 531 500 pairs (6.5e-7), 3 hypotheses left out; the
    best hypothesis counts 900 inliers of 900 planted, none of its pairs undecided
Hypotheses that are not finite or have an entry above 1e6 in magnitude (duplicate draws) are
left out (test_score_special_values_vs_oracle covers those); at most 2 % of the batch.
"""
import numpy as np
import pytest

from conftest import load_golden

LD = np.longdouble
R = LD(2.0) ** -24          # binary32 unit roundoff
UNDECIDED_CAP = 1e-4        # share of all pairs
EXCLUDED_CAP = 0.02         # share of the batch
THRESHOLDS = (0.5, 3.0)
N_HYP, SEED = 1024, 11


def _usable(H):
    """Hypotheses this test judges: finite, no entry above 1e6 in magnitude."""
    H = np.asarray(H, np.float32).reshape(-1, 9)
    with np.errstate(invalid="ignore"):
        return np.isfinite(H).all(axis=1) & (np.abs(H) <= 1e6).all(axis=1)


def exact_score(H, ps, pt, thresh, mutation=None):
    """(decided inliers, undecided) per hypothesis, by the header's definition in longdouble.
    `mutation` breaks the definition on purpose (the teeth checks): "swap_uv", "plus_uw",
    "t_for_t2"."""
    assert np.finfo(LD).nmant >= 63, "np.longdouble must carry a 64-bit significand"
    H = np.asarray(H, np.float32).reshape(-1, 9).astype(LD)
    x, y = (np.asarray(ps, np.float32)[:, k].astype(LD)[None, :] for k in (0, 1))
    u, v = (np.asarray(pt, np.float32)[:, k].astype(LD)[None, :] for k in (0, 1))
    if mutation == "swap_uv":
        u, v = v, u
    t32 = np.float32(thresh)
    t2 = LD(t32) if mutation == "t_for_t2" else LD(np.float32(t32 * t32))
    sign = LD(1) if mutation == "plus_uw" else LD(-1)
    inl = np.zeros(H.shape[0], np.int64)
    und = np.zeros(H.shape[0], np.int64)
    for lo in range(0, H.shape[0], 128):
        h = [H[lo:lo + 128, k][:, None] for k in range(9)]
        xs = h[0] * x + h[1] * y + h[2]
        ys = h[3] * x + h[4] * y + h[5]
        ws = h[6] * x + h[7] * y + h[8]
        Sx = np.abs(h[0] * x) + np.abs(h[1] * y) + np.abs(h[2])
        Sy = np.abs(h[3] * x) + np.abs(h[4] * y) + np.abs(h[5])
        Sw = np.abs(h[6] * x) + np.abs(h[7] * y) + np.abs(h[8])
        ex = xs + sign * u * ws
        ey = ys + sign * v * ws
        e2 = ex * ex + ey * ey
        lim = t2 * ws * ws
        Ex = 2 * R * (Sx + np.abs(u) * Sw) + R * np.abs(ex)
        Ey = 2 * R * (Sy + np.abs(v) * Sw) + R * np.abs(ey)
        cross = 2 * np.abs(ex) * Ex + 2 * np.abs(ey) * Ey
        de = cross + Ex * Ex + Ey * Ey + 2 * R * (e2 + cross)
        dl = t2 * (4 * R * np.abs(ws) * Sw + (2 * R * Sw) ** 2) + 2 * R * (1 + 4 * R) * lim
        undecided = np.abs(e2 - lim) <= de + dl
        inlier = (ws != 0) & (e2 <= lim) & ~undecided
        inl[lo:lo + 128] = inlier.sum(axis=1)
        und[lo:lo + 128] = undecided.sum(axis=1)
    return inl, und


def judge(counts, H, ps, pt, thresh, mutation=None):
    """The assertions' facts for one batch: (all decided pairs agree, undecided share of all
    pairs, excluded share of the batch, per-hypothesis undecided, usable mask)."""
    counts = np.asarray(counts).astype(np.int64).ravel()
    H = np.asarray(H, np.float32).reshape(-1, 9)
    use = _usable(H)
    inl, und = exact_score(H[use], ps, pt, thresh, mutation)
    agree = bool(((inl <= counts[use]) & (counts[use] <= inl + und)).all())
    pairs = int(use.sum()) * len(ps)
    und_all = np.zeros(H.shape[0], np.int64)
    und_all[use] = und
    return agree, und.sum() / max(pairs, 1), 1.0 - use.mean(), und_all, use


def check(counts, H, ps, pt, thresh, what):
    agree, share, excluded, und, use = judge(counts, H, ps, pt, thresh)
    print(f"{what} t={thresh}: undecided {int(und.sum())} of {int(use.sum()) * len(ps)} pairs "
          f"({share:.3g}), {int((~use).sum())} of {len(use)} hypotheses left out")
    assert excluded <= EXCLUDED_CAP, f"{what}: {excluded:.3%} of the hypotheses are degenerate"
    assert share <= UNDECIDED_CAP, f"{what}: undecided share {share:.3g}"
    assert agree, f"{what} t={thresh}: a decided pair disagrees with the exact definition"
    return und, use


def _wall():
    g = load_golden("cpp_wall.npz")
    return g["pool_src"], g["pool_tar"]


@pytest.fixture(scope="module")
def wall_cpu(oracle):
    """The wall pool, N_HYP oracle-solved ACA hypotheses of it, and the restatement's counts."""
    ps, pt = _wall()
    idx = oracle.fill_bits(4 * N_HYP, SEED, 0).reshape(N_HYP, 4)
    s, t = oracle.sample_problems(ps, pt, idx)
    H = oracle.solve("aca", s, t)
    return ps, pt, H, {th: oracle.ransac_score(H, ps, pt, th) for th in THRESHOLDS}


@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_oracle_score_means_the_header_definition(wall_cpu, thresh):
    """oracle.ransac_score -- the restatement the GPU tests lean on -- counts what the header
    says, wherever binary32 rounding cannot decide otherwise."""
    ps, pt, H, counts = wall_cpu
    check(counts[thresh], H, ps, pt, thresh, "oracle on the wall pool")


@pytest.mark.parametrize("mutation", ["swap_uv", "plus_uw", "t_for_t2"])
def test_mutated_definition_is_caught(wall_cpu, mutation):
    """Teeth: a reference with u and v swapped, + u w' for - u w', or t for t^2 no longer
    agrees with the restatement on the wall pool, at either threshold."""
    ps, pt, H, counts = wall_cpu
    for thresh in THRESHOLDS:
        agree = judge(counts[thresh], H, ps, pt, thresh, mutation)[0]
        assert not agree, f"{mutation} at t={thresh} went unnoticed"


def test_checker_rejects_a_miscount(wall_cpu):
    """One count off by more than its hypothesis's undecided pairs fails the comparison."""
    ps, pt, H, counts = wall_cpu
    und, use = judge(counts[3.0], H, ps, pt, 3.0)[3:5]
    bad = counts[3.0].astype(np.int64)
    i = int(np.flatnonzero(use)[0])
    bad[i] += und[i] + 1
    assert not judge(bad, H, ps, pt, 3.0)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", THRESHOLDS)
def test_gpu_score_means_the_header_definition(pkg, dev, thresh):
    import torch
    ps, pt = _wall()
    dps, dpt = torch.from_numpy(ps).to(dev), torch.from_numpy(pt).to(dev)
    H = pkg.sample_solve_seeded(dps, dpt, N_HYP, SEED)
    counts = pkg.ransac_score(H, dps, dpt, thresh)
    check(counts.cpu().numpy(), H.cpu().numpy(), ps, pt, thresh, "kernel on the wall pool")


def planted_pool(npool=1500, inlier_share=0.6, seed=2):
    """A pool from a known homography: the first 60 % of the targets are the projected
    sources (rounded to binary32), the rest are displaced by 20-200 px in a random direction."""
    rng = np.random.default_rng(seed)
    Ht = np.array([[0.9, 0.08, 25.0], [-0.06, 1.05, -14.0], [4e-5, -3e-5, 1.0]])
    src = rng.uniform(0, 1000, (npool, 2)).astype(np.float32)
    p = np.concatenate([src.astype(np.float64), np.ones((npool, 1))], 1) @ Ht.T
    tar = p[:, :2] / p[:, 2:3]
    planted = int(round(inlier_share * npool))
    r = rng.uniform(20, 200, npool - planted)
    a = rng.uniform(0, 2 * np.pi, npool - planted)
    tar[planted:] += np.stack([r * np.cos(a), r * np.sin(a)], 1)
    return src, tar.astype(np.float32), planted


@pytest.mark.gpu
def test_gpu_score_finds_the_planted_inliers(pkg, dev):
    """A synthetic pool with 900 exact pairs of a known H and 600 displaced by 20-200 px: the
    kernel's counts obey the exact definition on every hypothesis, and the best hypothesis
    counts the planted pairs, within its own undecided pairs."""
    import torch
    ps, pt, planted = planted_pool()
    dps, dpt = torch.from_numpy(ps).to(dev), torch.from_numpy(pt).to(dev)
    H = pkg.sample_solve_seeded(dps, dpt, N_HYP, SEED)
    counts = pkg.ransac_score(H, dps, dpt, 3.0).cpu().numpy().astype(np.int64)
    und, use = check(counts, H.cpu().numpy(), ps, pt, 3.0, "kernel on the planted pool")
    best = int(np.argmax(np.where(use, counts, -1)))
    print(f"best hypothesis {best}: {counts[best]} inliers, {planted} planted, {und[best]} undecided")
    assert abs(int(counts[best]) - planted) <= und[best], (counts[best], planted, und[best])
