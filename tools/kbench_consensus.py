"""Batched RANSAC consensus (hg_ransac_consensus_f32) against the only way the library had
before it: ransac() per image pair in a host loop.  Two shapes, one process, the arms
interleaved and rotated round by round, clocks settled by a warm-up of every arm:

  (a) many small pairs   256 pairs x 1024 hypotheses, ~500 points per pair (launch- and
                         sync-bound on the old path);
  (b) one large pair     1 pair x 1 M hypotheses on the wall pool, 2540 points (bound by the
                         scorer's VALU work): the fused call against the sum of the old path's
                         two kernels, sample_solve_seeded + score, timed in the same run.

Host-clock times end in a device synchronise; kernel times are device events around REPS
back-to-back launches.  Before anything is timed the fused results are compared, bit for bit,
with the old path's.  Writes the JSON named by --out (default
profiles/consensus/kbench_consensus.json) with every round's figure, the median and the
spread, and the kernel variants tried.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ROUNDS = 9
REPS = 10

# What was built and measured; one line per kernel shape tried (the shipped one first).  The
# earlier shapes' figures are shape (b)'s medians from their own runs of this tool (each run
# timed the old path's two kernels beside them: "parent" below).
VARIANTS = [
    {"name": "global gather + wave-uniform pool loads, <= 2048 blocks per pair, mask over "
             "several blocks per pair", "shipped": True,
     "shape": "2 hypotheses per lane as one packed pair, 4 gathered points per hypothesis from "
              "global memory, `%` remainder, pool through scalar loads unrolled 8 (the shipped "
              "scorer's loop), no LDS pool; per-block 64-bit key partials, then about one block "
              "per 1024 rows of a pair reduces, re-solves the winner and writes the mask",
     "b_fused_kernels_ms": "this file"},
    {"name": "the same, one block per pair in pass 2", "shipped": False,
     "b_fused_kernels_ms": 0.73471, "b_parent_two_kernels_ms": 0.7001},
    {"name": "the same, <= 1024 blocks per pair (4 waves per SIMD at 1 M hypotheses)",
     "shipped": False, "b_fused_kernels_ms": 0.80737, "b_parent_two_kernels_ms": 0.70955},
    {"name": "pool staged in LDS, remainder by a per-block magic constant", "shipped": False,
     "b_fused_kernels_ms": None, "note": "not built: the old path's scorer already chose scalar "
     "loads over LDS (profiles/r01/kbench_score.json), and the gather is 8 loads per 2540 "
     "point tests"},
]


def _stats(xs):
    med = statistics.median(xs)
    return {"median": round(med, 5), "min": round(min(xs), 5), "max": round(max(xs), 5),
            "spread_rel": round((max(xs) - min(xs)) / med, 4), "rounds": [round(x, 5) for x in xs]}


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _event_ms(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def _rotate(arms, rounds, warm=3):
    """Every arm once per round, the starting arm moving on each round."""
    names = list(arms)
    for _ in range(warm):
        for k in names:
            arms[k]()
    out = {k: [] for k in names}
    for r in range(rounds):
        for i in range(len(names)):
            k = names[(r + i) % len(names)]
            out[k].append(arms[k]())
    return out


def _c_abi(pkg, dev, ps, pt, off_dev, pairs, n, thresh):
    """The C entry on preallocated outputs: the call's own two launches, nothing else."""
    need = pkg.lib().hg_ransac_consensus_workspace(pairs, n)
    H = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
    cnt = torch.empty(pairs, dtype=torch.int32, device=dev)
    idx = torch.empty(pairs, dtype=torch.int64, device=dev)
    mask = torch.zeros(ps.shape[0], dtype=torch.uint8, device=dev)
    work = torch.empty(need // 8, dtype=torch.int64, device=dev)
    keep = (H, cnt, idx, mask, work)
    st = torch.cuda.current_stream(dev).cuda_stream

    def call():
        pkg._lib.call("hg_ransac_consensus_f32", ps.data_ptr(), pt.data_ptr(), ps.shape[0],
                      off_dev.data_ptr(), pairs, n, thresh, 11, 0, 0, H.data_ptr(), cnt.data_ptr(),
                      idx.data_ptr(), mask.data_ptr(), work.data_ptr(), st)
        return keep
    return call


def _same(pkg, ps, pt, off, n, thresh, res):
    """The fused result of every pair equals sample_solve_seeded + score + first arg-max."""
    for j in range(len(off) - 1):
        a, b = ps[off[j]:off[j + 1]], pt[off[j]:off[j + 1]]
        H = pkg.sample_solve_seeded(a, b, n, 11, 4 * n * j)
        c = pkg.ransac_score(H, a, b, thresh)
        i = int((c == c.max()).nonzero()[0].item())
        if not (torch.equal(H[i].view(torch.int32), res.H[j].view(torch.int32))
                and int(res.index[j]) == i and int(res.inliers[j]) == int(c[i])
                and int(res.mask[off[j]:off[j + 1]].sum()) == int(c[i])):
            return False
    return True


def shape_a(pkg, dev):
    pairs, n, thresh = 256, 1024, 3.0
    g = np.random.default_rng(20261019)
    sizes = g.integers(400, 601, pairs)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(off[-1])
    ps = torch.from_numpy((g.random((total, 2)) * 1000).astype(np.float32)).to(dev)
    pt = torch.from_numpy((g.random((total, 2)) * 1000).astype(np.float32)).to(dev)
    off_dev = torch.from_numpy(off).to(dev)
    slices = [(ps[off[j]:off[j + 1]], pt[off[j]:off[j + 1]]) for j in range(pairs)]
    exact = _same(pkg, ps, pt, off.tolist(), n, thresh,
                  pkg.ransac_consensus(ps, pt, n, thresh, pair_offsets=off_dev))

    def parent():
        return [pkg.ransac(a, b, n, thresh) for a, b in slices]

    def fused():
        return pkg.ransac_consensus(ps, pt, n, thresh, pair_offsets=off_dev)

    c_abi = _c_abi(pkg, dev, ps, pt, off_dev, pairs, n, thresh)
    t = _rotate({"parent_ransac_loop_ms": lambda: _host_ms(parent),
                 "fused_call_ms": lambda: _host_ms(fused),
                 "fused_back_to_back_ms": lambda: _event_ms(fused),
                 "fused_c_abi_back_to_back_ms": lambda: _event_ms(c_abi, 50)}, ROUNDS)
    rec = {"pairs": pairs, "hypotheses": n, "points_total": total, "points_per_pair": "400..600",
           "exact_vs_unfused": exact, **{k: _stats(v) for k, v in t.items()}}
    rec["speedup_host_median"] = round(rec["parent_ransac_loop_ms"]["median"]
                                       / rec["fused_call_ms"]["median"], 2)
    return rec


def shape_b(pkg, dev):
    n, thresh = 1 << 20, 3.0
    z = np.load(os.path.join(ROOT, "tests", "golden", "cpp_wall.npz"))
    ps = torch.from_numpy(z["pool_src"]).to(dev)
    pt = torch.from_numpy(z["pool_tar"]).to(dev)
    exact = _same(pkg, ps, pt, [0, ps.shape[0]], n, thresh, pkg.ransac_consensus(ps, pt, n, thresh))
    H = pkg.sample_solve_seeded(ps, pt, n, 11, 0)
    off_dev = torch.tensor([0, ps.shape[0]], dtype=torch.int64, device=dev)
    c_abi = _c_abi(pkg, dev, ps, pt, off_dev, 1, n, thresh)

    t = _rotate({"fused_c_abi_kernels_ms": lambda: _event_ms(c_abi),
                 "parent_sample_solve_seeded_ms": lambda: _event_ms(lambda: pkg.sample_solve_seeded(ps, pt, n, 11, 0)),
                 "parent_score_ms": lambda: _event_ms(lambda: pkg.ransac_score(H, ps, pt, thresh)),
                 "fused_kernels_ms": lambda: _event_ms(lambda: pkg.ransac_consensus(ps, pt, n, thresh)),
                 "parent_ransac_call_ms": lambda: _host_ms(lambda: pkg.ransac(ps, pt, n, thresh)),
                 "fused_call_ms": lambda: _host_ms(lambda: pkg.ransac_consensus(ps, pt, n, thresh))},
                ROUNDS)
    rec = {"pairs": 1, "hypotheses": n, "points_total": int(ps.shape[0]), "exact_vs_unfused": exact,
           **{k: _stats(v) for k, v in t.items()}}
    both = [a + b for a, b in zip(t["parent_sample_solve_seeded_ms"], t["parent_score_ms"])]
    rec["parent_two_kernels_ms"] = _stats(both)
    spread = max(both) - min(both)
    rec["fused_minus_parent_kernels_ms"] = round(rec["fused_kernels_ms"]["median"]
                                                 - rec["parent_two_kernels_ms"]["median"], 5)
    rec["fused_c_abi_minus_parent_kernels_ms"] = round(rec["fused_c_abi_kernels_ms"]["median"]
                                                       - rec["parent_two_kernels_ms"]["median"], 5)
    rec["parent_two_kernels_spread_ms"] = round(spread, 5)
    rec["within_spread"] = bool(rec["fused_c_abi_minus_parent_kernels_ms"] <= spread)
    rec["G_tests_per_s_fused"] = round(n * ps.shape[0] / rec["fused_kernels_ms"]["median"] / 1e6, 1)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "consensus", "kbench_consensus.json"))
    args = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    out = {"tool": "tools/kbench_consensus.py", "device": torch.cuda.get_device_name(dev),
           "library": pkg.version(), "rounds": ROUNDS, "launches_per_event_window": REPS,
           "method": "one process; arms interleaved, starting arm rotated each round; 3 warm-up "
                     "rounds of every arm; host-clock figures end in a device synchronise; "
                     "kernel figures are device events over back-to-back launches (fused_kernels: "
                     "the wrapper's mask memset + the call's two kernels; fused_c_abi: the C "
                     "entry on preallocated outputs, its two kernels alone)",
           "variants": VARIANTS,
           "a_many_small_pairs": shape_a(pkg, dev), "b_one_large_pair": shape_b(pkg, dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("a_many_small_pairs", "b_one_large_pair")}))


if __name__ == "__main__":
    main()
