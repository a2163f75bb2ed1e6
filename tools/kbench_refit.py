"""The least-squares refit (hg_ransac_refit_f32) and ransac_consensus(refine=R), timed.

Three shapes:
  (a) many small pairs   256 pairs x 400..600 points (the consensus benchmark's shape (a), with
                         1024 hypotheses where a consensus runs);
  (b) the wall file      1 pair x 2540 points;
  (c) one large pair     1 pair x 20 000 points.
Pools are correspondences of one homography per pair with 0.7 px noise and 30 % outliers (the
wall file as it is), masks are the consensus masks, so a refit sums over the rows a user would.

Per shape: the C entry alone on preallocated outputs; the same refit composed from torch ops
(binary64, masked sums, torch.linalg.solve per pair: what a user has without the entry);
ransac_consensus with refine 0 / 1 / 2 through the wrapper.  Device events around every single
launch, LAUNCHES of them after a warm-up, the median reported (and the mean of one back-to-back
window of the same length); the wrapper calls also by the host clock with a device synchronise.
Before anything is timed the entry's H is compared with the torch composition (a tolerance:
the orders of summation differ) and refine=0 with the plain call (bytes).
Writes profiles/refit/kbench_refit.json.
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

LAUNCHES = 200
WARM = 20
H_TRUE = np.array([[0.92, -0.11, 31.0], [0.08, 1.05, -12.0], [1.1e-4, -6.0e-5, 1.0]])


def _stats(xs):
    xs = sorted(xs)
    med = statistics.median(xs)
    return {"median": round(med, 5), "min": round(xs[0], 5), "p90": round(xs[int(0.9 * (len(xs) - 1))], 5),
            "max": round(xs[-1], 5), "launches": len(xs)}


def _per_launch_ms(fn, launches=LAUNCHES, warm=WARM):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(launches)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    rec = _stats([e0.elapsed_time(e1) for e0, e1 in ev])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    rec["back_to_back_mean"] = round(e0.elapsed_time(e1) / launches, 5)
    return rec


def _host_ms(fn, launches=LAUNCHES, warm=WARM):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(launches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return _stats(out)


def model_pool(g, npool):
    ps = g.random((npool, 2)) * 1000
    q = np.concatenate([ps, np.ones((npool, 1))], axis=1) @ H_TRUE.T
    pt = q[:, :2] / q[:, 2:] + g.normal(0, 0.7, (npool, 2))
    out = g.random(npool) < 0.3
    pt[out] = g.random((int(out.sum()), 2)) * 1000
    return ps.astype(np.float32), pt.astype(np.float32)


def torch_refit(ps, pt, mask, off):
    """The definition from torch ops, pair by pair, without a host round trip (rows weighted by
    0 / 1 instead of gathered): what a caller composes today.  (pairs,9) binary64."""
    out = []
    for lo, hi in zip(off, off[1:]):
        p = torch.cat([ps[lo:hi], pt[lo:hi]], dim=1).double()
        w = (mask[lo:hi] != 0).double()[:, None]
        n = w.sum()
        c = (p * w).sum(0) / n
        s = n / ((p - c).abs() * w).sum(0)
        q = (p - c) * s
        X, Y, a, b = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        one, zero = torch.ones_like(X), torch.zeros_like(X)
        Lx = torch.stack([X, Y, one, zero, zero, zero, -a * X, -a * Y, -a], dim=1) * w
        Ly = torch.stack([zero, zero, zero, X, Y, one, -b * X, -b * Y, -b], dim=1) * w
        LtL = Lx.T @ Lx + Ly.T @ Ly
        h = torch.linalg.solve(LtL[:8, :8], -LtL[:8, 8])
        Hn = torch.cat([h, torch.ones(1, dtype=h.dtype, device=h.device)]).view(3, 3)
        T2i = torch.stack([torch.stack([1 / s[2], zero[0], c[2]]), torch.stack([zero[0], 1 / s[3], c[3]]),
                           torch.stack([zero[0], zero[0], one[0]])])
        T1 = torch.stack([torch.stack([s[0], zero[0], -c[0] * s[0]]), torch.stack([zero[0], s[1], -c[1] * s[1]]),
                          torch.stack([zero[0], zero[0], one[0]])])
        H = T2i @ Hn @ T1
        out.append((H / H[2, 2]).reshape(9))
    return torch.stack(out)


def shape(pkg, dev, name, sizes, hypotheses, wall=False, torch_launches=LAUNCHES):
    g = np.random.default_rng(20261019)
    if wall:
        z = np.load(os.path.join(ROOT, "tests", "golden", "cpp_wall.npz"))
        ps_h, pt_h = z["pool_src"], z["pool_tar"]
    else:
        pools = [model_pool(g, int(m)) for m in sizes]
        ps_h = np.concatenate([p[0] for p in pools])
        pt_h = np.concatenate([p[1] for p in pools])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    pairs, total = len(sizes), int(off[-1])
    ps, pt = torch.from_numpy(ps_h).to(dev), torch.from_numpy(pt_h).to(dev)
    off_dev, off_list = torch.from_numpy(off).to(dev), off.tolist()
    thresh = 3.0
    base = pkg.ransac_consensus(ps, pt, hypotheses, thresh, pair_offsets=off_dev)
    mask = base.mask
    H = torch.empty((pairs, 9), dtype=torch.float32, device=dev)
    H64 = torch.empty((pairs, 9), dtype=torch.float64, device=dev)
    used = torch.empty(pairs, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def entry():
        pkg._lib.call("hg_ransac_refit_f32", ps.data_ptr(), pt.data_ptr(), total, off_dev.data_ptr(),
                      pairs, mask.data_ptr(), H.data_ptr(), H64.data_ptr(), used.data_ptr(), st)

    zero_mask = torch.zeros_like(mask)
    scratch = (torch.empty_like(H), torch.empty_like(used))

    def entry_zero():
        """The same launch with nothing selected: every block stops after the first pass (the
        count and the centroid sums), so this is the launch and one pass over the rows."""
        pkg._lib.call("hg_ransac_refit_f32", ps.data_ptr(), pt.data_ptr(), total, off_dev.data_ptr(),
                      pairs, zero_mask.data_ptr(), scratch[0].data_ptr(), None, scratch[1].data_ptr(), st)

    entry()
    composed = torch_refit(ps, pt, mask, off_list)
    fitted = torch.isfinite(H64).all(dim=1)
    rel = ((H64 - composed).abs() / composed.abs().clamp_min(1e-300))[fitted]
    plain = pkg.ransac_consensus(ps, pt, hypotheses, thresh, pair_offsets=off_dev)
    r0 = pkg.ransac_consensus(ps, pt, hypotheses, thresh, pair_offsets=off_dev, refine=0)
    same0 = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(plain, r0))
    inl = [pkg.ransac_consensus(ps, pt, hypotheses, thresh, pair_offsets=off_dev, refine=R).inliers.sum().item()
           for R in (0, 1, 2)]
    rec = {"pairs": pairs, "points_total": total, "hypotheses": hypotheses,
           "rows_selected": int(used.sum().item()), "pairs_fitted": int(fitted.sum().item()),
           "entry_vs_torch_composed_max_rel": float(rel.max().item()) if rel.numel() else None,
           "refine0_bytes_equal_plain_call": same0, "inliers_total_by_refine": inl,
           "refit_entry_ms": _per_launch_ms(entry),
           "refit_entry_nothing_selected_ms": _per_launch_ms(entry_zero),
           "refit_wrapper_ms": _per_launch_ms(lambda: pkg.refit(ps, pt, mask, pair_offsets=off_dev)),
           "torch_composed_ms": _per_launch_ms(lambda: torch_refit(ps, pt, mask, off_list),
                                               launches=torch_launches, warm=3)}
    for R in (0, 1, 2):
        fn = lambda R=R: pkg.ransac_consensus(ps, pt, hypotheses, thresh, pair_offsets=off_dev, refine=R)  # noqa: E731
        rec[f"consensus_refine{R}_events_ms"] = _per_launch_ms(fn)
        rec[f"consensus_refine{R}_host_ms"] = _host_ms(fn)
    rec["torch_over_entry"] = round(rec["torch_composed_ms"]["median"] / rec["refit_entry_ms"]["median"], 1)
    print(name, json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refit", "kbench_refit.json"))
    args = ap.parse_args()
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    g = np.random.default_rng(20261019)
    out = {"tool": "tools/kbench_refit.py", "device": torch.cuda.get_device_name(dev),
           "library": pkg.version(), "launches": LAUNCHES, "warm_up_launches": WARM,
           "method": "one process; device events around every single launch, the median of them; "
                     "back_to_back_mean: one event pair around the same number of launches; host: "
                     "perf_counter around a call that ends in a device synchronise",
           "parent_consensus_fused_call_ms": 0.12067,
           "a_256_pairs_x_500": shape(pkg, dev, "a", g.integers(400, 601, 256), 1024, torch_launches=20),
           "b_wall_2540": shape(pkg, dev, "b", [2540], 1024, wall=True),
           "c_one_pair_20000": shape(pkg, dev, "c", [20_000], 1024)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
