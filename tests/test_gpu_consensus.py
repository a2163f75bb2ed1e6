"""The batched RANSAC consensus (hg_ransac_consensus_f32, pkg.ransac_consensus) on the GPU.

It is defined as the unfused path pair by pair, so there is no tolerance anywhere: the
expected (H, count, index) come from the CPU oracle (fill_bits -> sample_problems -> solve ->
ransac_score -> first arg-max; the mask from ransac_score on one-point pools), and the same
values must equal the existing GPU path (sample_solve_seeded + ransac_score) as integer bit
patterns, NaN bits included.  The oracle's H is compared NaN for NaN (x86 and CDNA propagate
different NaN payloads, oracle.same_bits), everything else exactly.

Sizes (csrc/hg_consensus.hpp): a block takes 512 hypotheses per step (2 per lane, 4 waves), a
pair's hypotheses are shared by at most 2048 blocks, the scorer's pool loop is unrolled 8
times, the pool is gathered and streamed from global memory at every size.
"""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_extents import F32, I32, Arena, Checks, fresh_vs_arena

pytestmark = pytest.mark.gpu

THREADS = 16
_POOL = ThreadPoolExecutor(THREADS)
QNAN = 0x7FC00000
ALGO_ID = {"aca": 0, "sks": 1}


# ------------------------------------------------------------------------------ the oracle
def _oracle_counts(oracle, H, ps, pt, thresh):
    """oracle.ransac_score, the hypotheses split over threads (the C loop holds no lock)."""
    n = H.shape[0]
    if n * ps.shape[0] < 2_000_000:
        return oracle.ransac_score(H, ps, pt, thresh)
    cuts = np.linspace(0, n, THREADS + 1).astype(np.int64)
    parts = _POOL.map(lambda k: oracle.ransac_score(H[cuts[k]:cuts[k + 1]], ps, pt, thresh),
                      [k for k in range(THREADS) if cuts[k] < cuts[k + 1]])
    return np.concatenate(list(parts))


def _oracle_mask(oracle, h, ps, pt, thresh):
    """mask[i] = the oracle's count of h over the one-point pool {i}."""
    def rows(k):
        return [int(oracle.ransac_score(h, ps[i:i + 1], pt[i:i + 1], thresh)[0])
                for i in range(k, ps.shape[0], THREADS)]
    out = np.empty(ps.shape[0], np.uint8)
    for k, r in enumerate(_POOL.map(rows, range(THREADS))):
        out[k::THREADS] = r
    return out


def _oracle_consensus(oracle, ps, pt, n, seed, offset, algo, thresh):
    """(H (9,), count, index, mask, counts) of one pair by the definition."""
    bits = oracle.fill_bits(4 * n, seed, offset).reshape(n, 4)
    s, t = oracle.sample_problems(ps, pt, bits)
    H = oracle.solve(algo, s, t, normalize=True)
    counts = _oracle_counts(oracle, H, ps, pt, thresh)
    idx = int(np.argmax(counts))  # the first maximum
    return H[idx], int(counts[idx]), idx, _oracle_mask(oracle, H[idx], ps, pt, thresh), counts


def _unfused(pkg, dps, dpt, n, seed, offset, algo, thresh):
    """The existing GPU path: (H (9,) device, count, index)."""
    H = pkg.sample_solve_seeded(dps, dpt, n, seed, offset, algo=algo, normalize=True)
    counts = pkg.ransac_score(H, dps, dpt, thresh).cpu().numpy().view(np.uint32)
    idx = int(np.argmax(counts))
    return H[idx], int(counts[idx]), idx


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check_pair(orc, oracle, pkg, res, j, ps, pt, dps, dpt, n, seed, offset, algo, thresh,
                mask_rows=None, label=""):
    """Pair j of `res` against the oracle and against the unfused GPU path."""
    want_h, want_c, want_i, want_m, counts = _oracle_consensus(oracle, ps, pt, n, seed, offset,
                                                               algo, thresh)
    got_h = res.H[j].cpu().numpy()
    got_c, got_i = int(res.inliers[j].item()), int(res.index[j].item())
    assert (got_c, got_i) == (want_c, want_i), f"{label}: got {(got_c, got_i)}, oracle {(want_c, want_i)}"
    assert orc.same_bits(got_h, want_h).all(), f"{label}: H differs from the oracle"
    gh, gc, gi = _unfused(pkg, dps, dpt, n, seed, offset, algo, thresh)
    assert (got_c, got_i) == (gc, gi), f"{label}: got {(got_c, got_i)}, unfused GPU {(gc, gi)}"
    assert torch.equal(_bits(res.H[j]), _bits(gh)), f"{label}: H bits differ from sample_solve_seeded"
    m = res.mask if mask_rows is None else res.mask[mask_rows[0]:mask_rows[1]]
    got_m = m.cpu().numpy()
    assert np.array_equal(got_m, want_m), f"{label}: {(got_m != want_m).sum()} mask bytes differ"
    assert int(got_m.sum()) == got_c, f"{label}: mask holds {int(got_m.sum())}, count {got_c}"
    return counts


@functools.lru_cache(maxsize=None)
def _random_pool(npool, seed=0):
    g = np.random.default_rng(1000 * seed + npool)
    ps = (g.random((npool, 2)) * 1000).astype(np.float32)
    pt = (g.random((npool, 2)) * 1000).astype(np.float32)
    return ps, pt


@functools.lru_cache(maxsize=None)
def _wall():
    g = load_golden("cpp_wall.npz")
    return g["pool_src"], g["pool_tar"]


def _dev(dev, *arrays):
    return [torch.from_numpy(a).to(dev) for a in arrays]


# ------------------------------------------------------------------------ one pair, random pools
@pytest.mark.parametrize("thresh", [0.0, 3.0])
@pytest.mark.parametrize("algo", ["aca", "sks"])
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 1000, 65_537])
@pytest.mark.parametrize("npool", [1, 3, 4, 63, 64, 65, 2540, 20_000])
def test_one_pair_random_pools(orc, oracle, pkg, dev, npool, n, algo, thresh):
    """Odd and even lane packing (n = 1, 2, 3), the ragged last step (127 ... 129, 1000), many
    blocks per pair (65 537: 129 blocks, the cross-block reduction), pools below, at and above
    the unroll and far beyond any LDS staging (20 000)."""
    ps, pt = _random_pool(npool)
    dps, dpt = _dev(dev, ps, pt)
    res = pkg.ransac_consensus(dps, dpt, n, thresh, seed=11, algo=algo)
    assert res.H.shape == (1, 9) and res.inliers.shape == (1,) and res.index.shape == (1,)
    assert res.mask.shape == (npool,) and res.mask.dtype == torch.uint8
    assert res.index.dtype == torch.int64 and res.inliers.dtype == torch.int32
    _check_pair(orc, oracle, pkg, res, 0, ps, pt, dps, dpt, n, 11, 0, algo, thresh,
                label=f"npool {npool} n {n} {algo} thresh {thresh}")


@pytest.mark.parametrize("offset", [0, 3, (1 << 33) + 5])
def test_stream_offsets(orc, oracle, pkg, dev, offset):
    """Even, odd (the four words cross three hashes) and beyond-2^32 stream offsets."""
    ps, pt = _wall()
    dps, dpt = _dev(dev, ps, pt)
    for algo in ("aca", "sks"):
        res = pkg.ransac_consensus(dps, dpt, 1000, 3.0, seed=5, offset=offset, algo=algo)
        _check_pair(orc, oracle, pkg, res, 0, ps, pt, dps, dpt, 1000, 5, offset, algo, 3.0,
                    label=f"offset {offset} {algo}")


# ------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_lowest_index(orc, oracle, pkg, dev):
    """thresh = 1e18 (t2 = 1e36, finite): nearly every finite hypothesis counts the whole pool,
    so hundreds of hypotheses tie at the maximum; thresh = 0 on the wall pool ties at small
    counts.  The winner is the lowest index among them, and the oracle's."""
    for (ps, pt), thresh in ((_random_pool(4), 1e18), (_random_pool(65), 1e18), (_wall(), 1e18),
                             (_wall(), 0.0)):
        dps, dpt = _dev(dev, ps, pt)
        for algo in ("aca", "sks"):
            res = pkg.ransac_consensus(dps, dpt, 1000, thresh, seed=11, algo=algo)
            counts = _check_pair(orc, oracle, pkg, res, 0, ps, pt, dps, dpt, 1000, 11, 0, algo,
                                 thresh, label=f"ties {ps.shape[0]} {thresh} {algo}")
            tied = np.flatnonzero(counts == counts.max())
            assert tied.size > 1, "the case has no tie to break"
            assert int(res.index[0].item()) == int(tied[0])
            if ps.shape[0] == 4:  # most draws repeat a point: the first finite H is not row 0
                assert tied[0] > 0


def test_all_degenerate(orc, oracle, pkg, dev):
    """A pool of identical points: every H is NaN and every count 0, so the winner is index 0
    with row 0's NaN bits exactly as sample_solve_seeded writes them, and an all-zero mask."""
    ps = np.full((37, 2), 5.0, np.float32)
    pt = np.full((37, 2), 7.0, np.float32)
    dps, dpt = _dev(dev, ps, pt)
    for algo in ("aca", "sks"):
        for n in (1, 300, 1025):
            res = pkg.ransac_consensus(dps, dpt, n, 3.0, seed=11, algo=algo)
            counts = _check_pair(orc, oracle, pkg, res, 0, ps, pt, dps, dpt, n, 11, 0, algo, 3.0,
                                 label=f"degenerate {algo} {n}")
            assert counts.max() == 0, "the oracle finds an inlier: the case is not degenerate"
            row0 = pkg.sample_solve_seeded(dps, dpt, n, 11, 0, algo=algo)[0]
            assert torch.isnan(row0).any()
            assert torch.equal(_bits(res.H[0]), _bits(row0))
            assert int(res.inliers[0].item()) == 0 and int(res.index[0].item()) == 0
            assert int(res.mask.sum().item()) == 0


# --------------------------------------------------------------------------- batched pairs
SIZES = {1: [2540], 3: [65, 0, 700],
         33: [700, 1, 4, 65, 12_000, 2540, 0, 4, 700, 65, 1, 2540, 4, 65, 700, 1,
              0,  # the empty pair in the middle
              12_000, 65, 4, 1, 700, 2540, 65, 0, 1, 4, 700, 65, 2540, 1, 4, 12_000]}


def _batch(dev, sizes):
    total = sum(sizes)
    ps, pt = _random_pool(total, seed=7)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return ps, pt, off, _dev(dev, ps, pt)


@pytest.mark.parametrize("pairs", [1, 3, 33])
def test_batched_pairs_equal_single_pair_calls(orc, oracle, pkg, dev, pairs):
    """One call over ragged pairs: each pair equals the single-pair call made on its slice
    with offset + 4 n j (which the tests above pin to the oracle), the empty pairs follow
    their definition, and the mask is right up to both edges of every slice."""
    sizes = SIZES[pairs]
    assert len(sizes) == pairs
    ps, pt, off, (dps, dpt) = _batch(dev, sizes)
    n, seed, offset, thresh = 1000, 11, 6, 3.0
    for algo in ("aca", "sks"):
        res = pkg.ransac_consensus(dps, dpt, n, thresh, pair_offsets=off.tolist(), seed=seed,
                                   offset=offset, algo=algo)
        on_dev = pkg.ransac_consensus(dps, dpt, n, thresh, seed=seed, offset=offset, algo=algo,
                                      pair_offsets=torch.from_numpy(off).to(dev))
        for a, b in zip(res, on_dev):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        want_mask = torch.zeros(sum(sizes), dtype=torch.uint8, device=dev)
        for j, m in enumerate(sizes):
            lo, hi = int(off[j]), int(off[j + 1])
            if m == 0:
                assert _bits(res.H[j]).tolist() == [QNAN] * 9, (algo, j)
                assert int(res.inliers[j].item()) == 0 and int(res.index[j].item()) == 0
                continue
            one = pkg.ransac_consensus(dps[lo:hi], dpt[lo:hi], n, thresh, seed=seed,
                                       offset=offset + 4 * n * j, algo=algo)
            assert torch.equal(_bits(res.H[j]), _bits(one.H[0])), (algo, j, m)
            assert int(res.inliers[j].item()) == int(one.inliers[0].item()), (algo, j, m)
            assert int(res.index[j].item()) == int(one.index[0].item()), (algo, j, m)
            want_mask[lo:hi] = one.mask
        assert torch.equal(res.mask, want_mask), algo
        assert int(res.mask.max().item()) <= 1
        no_mask = pkg.ransac_consensus(dps, dpt, n, thresh, pair_offsets=off.tolist(), seed=seed,
                                       offset=offset, algo=algo, mask=False)
        assert torch.equal(_bits(no_mask.H), _bits(res.H)) and int(no_mask.mask.sum().item()) == 0
    if pairs == 3:  # and the oracle directly, with the pair's slice of the stream
        for j in (0, 2):
            lo, hi = int(off[j]), int(off[j + 1])
            _check_pair(orc, oracle, pkg, res, j, ps[lo:hi], pt[lo:hi], dps[lo:hi], dpt[lo:hi], n,
                        seed, offset + 4 * n * j, "sks", thresh, mask_rows=(lo, hi),
                        label=f"batched pair {j}")


def _call(pkg, dev, dps, dpt, off_dev, pairs, n, thresh, seed, offset, algo, H, count, index,
          mask, work):
    pkg._lib.call("hg_ransac_consensus_f32", dps.data_ptr(), dpt.data_ptr(), dps.shape[0],
                  off_dev.data_ptr(), pairs, n, thresh, seed, offset, ALGO_ID[algo], H, count,
                  index, mask, work, torch.cuda.current_stream(dev).cuda_stream)


def test_offsets_are_clamped(pkg, dev):
    """Offsets below 0, a descending step and a last entry beyond total: the kernel clamps
    them into [0, total] and treats the descending step as an empty pair, so the call
    returns 0, every pair equals the single-pair call on its clamped slice, and nothing is
    written outside the outputs.  Rows 600 ... 899 belong to two pairs (1 and 3): their mask
    bytes may come from either, and are 0 or 1."""
    total, n, thresh, seed, offset = 1000, 600, 3.0, 3, 2
    ps, pt = _random_pool(total, seed=9)
    dps, dpt = _dev(dev, ps, pt)
    raw = [-7, 400, 900, 600, 5000]
    clamped = [(0, 400), (400, 900), None, (600, 1000)]
    pairs = len(raw) - 1
    off_dev = torch.tensor(raw, dtype=torch.int64, device=dev)
    need = pkg.lib().hg_ransac_consensus_workspace(pairs, n)
    aH, ac, ai = Arena(dev, pairs * 36, 4), Arena(dev, pairs * 4, 4), Arena(dev, pairs * 8, 8)
    am, aw = Arena(dev, total, 4), Arena(dev, need, 8)
    keep = [dps.clone(), dpt.clone(), off_dev.clone()]
    _call(pkg, dev, dps, dpt, off_dev, pairs, n, thresh, seed, offset, "aca", aH.ptr(), ac.ptr(),
          ai.ptr(), am.ptr(), aw.ptr())
    ck = Checks()
    for name, a in (("best_H", aH), ("best_count", ac), ("best_index", ai), ("mask", am),
                    ("workspace", aw)):
        ck.scratch(f"clamped {name}", a)
    ck.inputs("clamped", [dps, dpt, off_dev], keep)
    ck.verify()
    H = aH.payload().clone().view(torch.int32).view(pairs, 9)
    count, index = ac.payload().clone().view(torch.int32), ai.payload().clone().view(torch.int64)
    mask = am.payload().clone()
    for j, rows in enumerate(clamped):
        if rows is None:
            assert H[j].tolist() == [QNAN] * 9 and int(count[j]) == 0 and int(index[j]) == 0
            continue
        lo, hi = rows
        one = pkg.ransac_consensus(dps[lo:hi], dpt[lo:hi], n, thresh, seed=seed,
                                   offset=offset + 4 * n * j, algo="aca")
        assert torch.equal(H[j], _bits(one.H[0])), j
        assert int(count[j]) == int(one.inliers[0].item()) and int(index[j]) == int(one.index[0].item())
        own = [(lo, min(hi, 600)), (900, hi)] if j in (1, 3) else [(lo, hi)]
        for a, b in own:
            if a < b:
                assert torch.equal(mask[a:b], one.mask[a - lo:b - lo]), (j, a, b)
    assert int(mask.max().item()) <= 1


# ------------------------------------------------------------------------------ the wall file
def test_wall_file_equals_ransac(pkg, dev):
    """The reference's correspondence file, 20 000 hypotheses, seed 11, thresh 3: the H, the
    count and the index of pkg.ransac, and a mask that holds exactly `inliers` ones."""
    ps, pt = _wall()
    dps, dpt = _dev(dev, ps, pt)
    for algo in ("aca", "sks"):
        want = pkg.ransac(dps, dpt, hypotheses=20_000, thresh=3.0, seed=11, algo=algo)
        res = pkg.ransac_consensus(dps, dpt, 20_000, 3.0, seed=11, algo=algo)
        assert torch.equal(_bits(res.H[0]), _bits(want.H)), algo
        assert int(res.inliers[0].item()) == want.inliers and int(res.index[0].item()) == want.index
        assert int(res.mask.sum().item()) == want.inliers
        assert want.inliers > 0.5 * ps.shape[0]


# ------------------------------------------------------------------------------- inlier_mask
def test_inlier_mask_special_values_vs_oracle(oracle, pkg, dev):
    """inlier_mask alone on the hypotheses and pool of test_score_special_values_vs_oracle
    (NaN, +-Inf, signed zeros, huge and subnormal entries, w' = 0): every byte equals the
    oracle's count over that one point."""
    rng = np.random.default_rng(8)
    npool, n = 777, 5003
    ps = rng.uniform(0, 1000, (npool, 2)).astype(np.float32)
    pt = rng.uniform(0, 1000, (npool, 2)).astype(np.float32)
    H = rng.standard_normal((n, 9)).astype(np.float32)
    H[:, 8] = 1.0
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, 1e-40], np.float32)
    H[::11, 6:9] = 0.0
    for i in range(0, n, 5):
        H[i, rng.integers(0, 9)] = specials[i % len(specials)]
    for i in range(0, npool, 9):
        ps[i, rng.integers(0, 2)] = specials[i % len(specials)]
    H[7] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    pt[::3] = ps[::3]
    K = 120  # rows 0 ... 119: every special value (rows 0, 5, ... 30), w' = 0 rows, the identity
    dps, dpt = _dev(dev, ps, pt)
    dH = torch.from_numpy(H[:K]).to(dev)
    for thresh in (0.0, 2.0):
        want = np.stack([oracle.ransac_score(H[:K], ps[i:i + 1], pt[i:i + 1], thresh)
                         for i in range(npool)], axis=1)          # (K, npool)
        assert want.max() == 1 and want[7].sum() > 100
        got = torch.stack([pkg.inlier_mask(dH[k], dps, dpt, thresh) for k in range(K)])
        assert got.dtype == torch.uint8
        np.testing.assert_array_equal(got.cpu().numpy(), want.astype(np.uint8))
        counts = pkg.ransac_score(dH, dps, dpt, thresh)
        assert torch.equal(got.sum(dim=1, dtype=torch.int32), counts)


# ------------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("offs", [(0, 0, 0, 0, 0), (4, 4, 8, 4, 8), (8, 8, 0, 8, 0), (4, 8, 8, 1, 0)])
def test_outputs_under_guard_bands(pkg, dev, offs):
    """best_H, best_count, best_index, mask and the workspace as arena payloads at byte offsets
    0, +4 and +8 (best_index and the workspace, 8-B types: 0 and +8; the mask also +1): the
    guards keep 0xA5, the payloads equal the plain call's, the inputs are untouched."""
    sizes = [65, 0, 700, 4, 513]
    pairs, total, n = len(sizes), sum(sizes), 600
    ps, pt, off, (dps, dpt) = _batch(dev, sizes)
    off_dev = torch.from_numpy(off).to(dev)
    need = pkg.lib().hg_ransac_consensus_workspace(pairs, n)
    ck = Checks()
    for algo in ("aca", "sks"):
        fresh_vs_arena(
            ck, f"consensus {algo} {offs}", pkg, dev, "hg_ransac_consensus_f32",
            lambda p: (dps.data_ptr(), dpt.data_ptr(), total, off_dev.data_ptr(), pairs, n, 3.0,
                       11, 1, ALGO_ID[algo], p["H"], p["count"], p["index"], p["mask"], p["work"]),
            outs={"H": (pairs * 9, F32), "count": (pairs, I32), "index": (pairs * 2, I32),
                  "mask": (total, torch.uint8)},
            offsets=dict(zip(("H", "count", "index", "mask", "work"), offs)),
            inputs=(dps, dpt, off_dev), scratch={"work": (need // 4, I32)})
    h = pkg.ransac_consensus(dps, dpt, n, 3.0, pair_offsets=off_dev, seed=11, offset=1).H[2]
    for o in (0, 1, 4, 8):
        fresh_vs_arena(
            ck, f"inlier_mask +{o}", pkg, dev, "hg_ransac_inlier_mask_f32",
            lambda p: (h.data_ptr(), dps.data_ptr(), dpt.data_ptr(), total, 3.0, p["mask"]),
            outs={"mask": (total, torch.uint8)}, offsets={"mask": o}, inputs=(h, dps, dpt))
    ck.verify()


# ------------------------------------------------------------------- graph capture, determinism
def _buffers(pkg, dev, pairs, total, n):
    need = pkg.lib().hg_ransac_consensus_workspace(pairs, n)
    return (torch.empty((pairs, 9), dtype=torch.float32, device=dev),
            torch.empty(pairs, dtype=torch.int32, device=dev),
            torch.empty(pairs, dtype=torch.int64, device=dev),
            torch.zeros(total, dtype=torch.uint8, device=dev),
            torch.empty(need // 8, dtype=torch.int64, device=dev))


def test_consensus_in_a_graph(pkg, dev):
    """One batched call captured on a side stream (two launches in a chain, nothing allocated,
    no synchronisation) and replayed twice gives the eager call's bytes both times."""
    sizes = SIZES[33]
    pairs, total, n = len(sizes), sum(sizes), 1000
    _, _, off, (dps, dpt) = _batch(dev, sizes)
    off_dev = torch.from_numpy(off).to(dev)
    want = pkg.ransac_consensus(dps, dpt, n, 3.0, pair_offsets=off_dev, seed=11, offset=6)
    bufs = _buffers(pkg, dev, pairs, total, n)

    def run():
        _call(pkg, dev, dps, dpt, off_dev, pairs, n, 3.0, 11, 6, "aca",
              *[b.data_ptr() for b in bufs])

    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        run()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            run()
    torch.cuda.current_stream(dev).wait_stream(s)
    for _ in range(2):
        for b in bufs:
            b.fill_(0x5A if b.dtype == torch.uint8 else 7)
        bufs[3].zero_()
        g.replay()
        torch.cuda.synchronize(dev)
        for got, w in zip(bufs[:4], want):
            assert torch.equal(got.view(torch.uint8), w.view(torch.uint8))


def test_two_calls_give_identical_bytes(pkg, dev):
    sizes = SIZES[33]
    _, _, off, (dps, dpt) = _batch(dev, sizes)
    for algo in ("aca", "sks"):
        a = pkg.ransac_consensus(dps, dpt, 65_537, 3.0, pair_offsets=off.tolist(), algo=algo)
        b = pkg.ransac_consensus(dps, dpt, 65_537, 3.0, pair_offsets=off.tolist(), algo=algo)
        for x, y in zip(a, b):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
