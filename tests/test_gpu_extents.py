"""Output extents under guard bands.

Every other GPU test compares elements [0, n) of an output that the caching allocator handed
out: a tail tile that stores one row or one 16-B chunk past n lands in allocator slack or in a
neighbour nobody looks at, and an element a kernel skips can read back the previous test's
(often identical) answer from a recycled block.  Here every device output is a slice of an
``Arena``: one uint8 tensor laid out [guard | payload | guard] and filled with the byte 0xA5,
each guard 64 KiB (more than one workgroup's whole output for every kernel here: at most 512
rows x 72 B), the payload starting at a chosen byte offset from a 256-B boundary -- 0 for the
16-B vector paths, +4 for binary32's generic / per-lane paths, +8 for binary64 that is
element-aligned but not 16-B aligned.  Entry points that require an alignment (the samplers' H,
the 8-B grad_corner, hg_stream_copy) get offset 0 only.

The arena's pointer goes through the C ABI (pkg._lib.call) on torch's current stream.  Then,
on the device:
  * both guards (and the 4 KiB gaps between the batches of a grouped call) still hold 0xA5 in
    every byte;
  * the payload equals, byte for byte, what the plain wrapper (pkg.solve, pkg.tensor_aca_rect,
    ...) returns for the same inputs -- or, where the package has no wrapper with that output
    layout, what the same entry point writes into a fresh 16-B aligned tensor -- which the
    other test files pin to the oracle.  The payload held 0xA5 before the call, so an element
    the kernel never wrote fails here;
  * every input equals a clone taken before the call.
For a buffer documented as scratch (x of the two in-place sums, the workspaces) only the guards
are asserted.  All comparisons run on the device; one vector of booleans per test comes back.

Shapes are the smallest at which the tails differ (csrc constants: wave 64, block 256, AoS tile
128 f32 / 64 f64 per wave, kSoaWideMinN 32768, kAtenGrain 32768, MRG order 2^17, scorer 512
hypotheses per block, the samplers' LDS pool limit).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024
GAP = 4096
FILL = 0xA5
F32, F64, I32 = torch.float32, torch.float64, torch.int32
DT = {"f32": F32, "f64": F64}
ESIZE = {F32: 4, F64: 8, I32: 4, torch.uint8: 1}
ALGOS = {"f32": ("aca", "sks", "ge"), "f64": ("aca", "sks", "ge", "gpt")}
ALGO_ID = {"aca": 0, "sks": 1, "ge": 2, "gpt": 3}
OFFSETS = {"f32": (0, 4), "f64": (0, 8)}
SFX_OFFSETS = [(s, o) for s in ("f32", "f64") for o in OFFSETS[s]]


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _st(dev):
    return torch.cuda.current_stream(dev).cuda_stream


class Arena:
    """[guard | payload 0 | gap | payload 1 | ... | guard] of 0xA5 bytes; payload i starts
    `offset` bytes past a 256-B boundary and holds exactly sizes[i] bytes."""

    def __init__(self, dev, sizes, offset=0, gap=GAP):
        self.sizes = [sizes] if isinstance(sizes, int) else list(sizes)
        room = sum(s + offset + gap + 256 for s in self.sizes)
        self.buf = torch.full((2 * GUARD + 256 + room,), FILL, dtype=torch.uint8, device=dev)
        base = self.buf.data_ptr()
        pos = GUARD + (-(base + GUARD)) % 256
        self.segs = []
        for s in self.sizes:
            lo = pos + offset
            self.segs.append((lo, lo + s))
            pos = lo + s + gap
            pos += (-(base + pos)) % 256
        assert self.segs[0][0] >= GUARD and self.buf.numel() - self.segs[-1][1] >= GUARD

    def ptr(self, i=0):
        return self.buf.data_ptr() + self.segs[i][0]

    def payload(self, i=0):
        lo, hi = self.segs[i]
        return self.buf[lo:hi]

    def put(self, t, i=0):
        """Loads an input / scratch payload with t's bytes."""
        self.payload(i).copy_(_bytes(t))
        return self

    def guards_ok(self):
        """Device bool: every byte outside the payloads is still 0xA5."""
        edges = [0] + [e for seg in self.segs for e in seg] + [self.buf.numel()]
        return torch.stack([(self.buf[edges[k]:edges[k + 1]] == FILL).all()
                            for k in range(0, len(edges), 2)]).all()

    def holds(self, expected, i=0):
        """Device bool: payload i equals `expected` byte for byte."""
        e = _bytes(expected)
        assert e.numel() == self.sizes[i], (e.numel(), self.sizes[i])
        return (self.payload(i) == e).all()


class Checks:
    """Labelled device booleans, brought back in one copy."""

    def __init__(self):
        self.items = []

    def add(self, label, ok):
        self.items.append((label, ok.reshape(())))

    def outputs(self, label, arena, expected):
        self.add(f"{label}: guard bytes changed", arena.guards_ok())
        for i, e in enumerate(expected):
            self.add(f"{label}: payload {i} differs from the plain call", arena.holds(e, i))

    def scratch(self, label, arena):
        self.add(f"{label}: guard bytes changed", arena.guards_ok())

    def inputs(self, label, tensors, clones):
        for k, (t, c) in enumerate(zip(tensors, clones)):
            self.add(f"{label}: input {k} modified", (_bytes(t) == _bytes(c)).all())

    def failures(self):
        if not self.items:
            return []
        flags = torch.stack([ok for _, ok in self.items]).cpu().tolist()
        return [label for (label, _), ok in zip(self.items, flags) if not ok]

    def verify(self):
        assert self.items, "nothing was checked"
        bad = self.failures()
        assert not bad, f"{len(bad)} of {len(self.items)} checks failed: {bad[:12]}"


def _rand(dev, shape, dt=F32, seed=0, lo=0.0, hi=1000.0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.rand(shape, generator=g, dtype=dt, device=dev) * (hi - lo) + lo


def _nbytes(spec):
    return spec[0] * ESIZE[spec[1]]


def fresh_vs_arena(ck, label, pkg, dev, name, build, outs, offsets=None, inputs=(), scratch=None):
    """Calls C entry `name` twice -- outputs into fresh aligned tensors (the plain call), then
    into arenas -- and records the checks.  outs: {key: (elements, dtype) or None (a NULL
    output)}; scratch: {key: a tensor of initial data, or (elements, dtype) uninitialised};
    offsets: {key: byte offset of that arena}; build(p) -> the argument tuple from the
    pointers p[key] (None for NULL), the stream excluded."""
    offsets, scratch = offsets or {}, scratch or {}
    st = _st(dev)
    keep = [t.clone() for t in inputs]
    spec = {k: (v if isinstance(v, tuple) else (v.numel(), v.dtype)) for k, v in scratch.items()}
    fresh = {k: None if v is None else torch.empty(v[0], dtype=v[1], device=dev)
             for k, v in outs.items()}
    fs = {k: (torch.empty(v[0], dtype=v[1], device=dev) if isinstance(v, tuple) else v.clone())
          for k, v in scratch.items()}
    p = {k: None if t is None else t.data_ptr() for k, t in fresh.items()}
    p.update({k: t.data_ptr() for k, t in fs.items()})
    pkg._lib.call(name, *build(p), st)
    arenas = {k: None if v is None else Arena(dev, _nbytes(v), offsets.get(k, 0))
              for k, v in outs.items()}
    sa = {k: Arena(dev, _nbytes(spec[k]), offsets.get(k, 0)) for k in scratch}
    for k, v in scratch.items():
        if not isinstance(v, tuple):
            sa[k].put(v)
    p = {k: None if a is None else a.ptr() for k, a in arenas.items()}
    p.update({k: a.ptr() for k, a in sa.items()})
    pkg._lib.call(name, *build(p), st)
    for k, a in arenas.items():
        if a is not None:
            ck.outputs(f"{label} {k}", a, [fresh[k]])
    for k, a in sa.items():
        ck.scratch(f"{label} {k}", a)
    ck.inputs(label, inputs, keep)


# ------------------------------------------------------------------------ the helper itself
def test_arena_checker_reports_stray_writes_and_unwritten_elements(dev):
    """A one-byte write (made with torch) into either guard or into a gap, or one payload
    element left unwritten, makes the checker report failure; a clean call does not."""
    want = [_rand(dev, (250,), seed=1), _rand(dev, (3,), F64, seed=2)]

    def filled(offset):
        a = Arena(dev, [1000, 24], offset)
        assert (a.ptr(0) - offset) % 256 == 0 and (a.ptr(1) - offset) % 256 == 0
        assert a.ptr(1) - (a.ptr(0) + 1000) >= GAP
        return a.put(want[0], 0).put(want[1], 1)

    for offset in (0, 4, 8):
        ck = Checks()
        ck.outputs("clean", filled(offset), want)
        assert ck.failures() == []
        a = filled(offset)
        n = a.buf.numel()
        strays = {"first byte": 0, "below payload 0": a.segs[0][0] - 1, "above payload 0": a.segs[0][1],
                  "below payload 1": a.segs[1][0] - 1, "above payload 1": a.segs[1][1], "last byte": n - 1}
        for where, at in strays.items():
            a = filled(offset)
            a.buf[at] = 0
            ck = Checks()
            ck.outputs(where, a, want)
            assert ck.failures() == [f"{where}: guard bytes changed"], (offset, where)
        a = Arena(dev, [1000, 24], offset).put(want[1], 1)
        a.payload(0)[:996].copy_(_bytes(want[0])[:996])      # the last float never written
        ck = Checks()
        ck.outputs("unwritten", a, want)
        assert ck.failures() == ["unwritten: payload 0 differs from the plain call"], offset
    ck = Checks()
    x = _rand(dev, (10,), seed=3)
    keep = x.clone()
    x[7] = -x[7]
    ck.inputs("touched", [x], [keep])
    assert ck.failures() == ["touched: input 0 modified"]
    with pytest.raises(AssertionError):
        ck.verify()


# ------------------------------------------------------------------------------ the solvers
def _solver_case(ck, pkg, dev, algo, sfx, n, soa, flag, offset):
    dt = DT[sfx]
    shape = (8, n) if soa else (n, 8)
    src, tar = _rand(dev, shape, dt, seed=2 * n), _rand(dev, shape, dt, seed=2 * n + 1)
    keep = [src.clone(), tar.clone()]
    want = pkg.solve(algo, src, tar, normalize=bool(flag), layout="soa" if soa else "aos")
    H = Arena(dev, 9 * n * ESIZE[dt], offset)
    pkg._lib.call(f"hg_{algo}_{sfx}", src.data_ptr(), tar.data_ptr(), H.ptr(), n, int(soa), flag,
                  _st(dev))
    label = f"hg_{algo}_{sfx} {'soa' if soa else 'aos'} n={n} flags={flag} +{offset}"
    ck.outputs(label, H, [want])
    ck.inputs(label, [src, tar], keep)


@pytest.mark.parametrize("sfx,offset", SFX_OFFSETS)
def test_aos_solvers(pkg, dev, sfx, offset):
    """H (n,9): the LDS-staged 16-B slab stores at offset 0 (full and partial wave tiles), the
    generic per-lane kernel otherwise."""
    ck = Checks()
    for algo in ALGOS[sfx]:
        for flag in (0, 1):
            for n in (1, 63, 65, 127, 129, 255, 257, 511, 513):
                _solver_case(ck, pkg, dev, algo, sfx, n, False, flag, offset)
    ck.verify()


@pytest.mark.parametrize("sfx,offset", SFX_OFFSETS)
def test_soa_solvers(pkg, dev, sfx, offset):
    """H (9,n), the end of row 8: the narrow form everywhere; binary64 at 32768 / 32770 takes
    the 16-B register form (and GPT's) when aligned, 32769 never does."""
    ck = Checks()
    ns = (1, 255, 257) + ((32768, 32769, 32770) if sfx == "f64" else ())
    for algo in ALGOS[sfx]:
        for flag in (0, 1):
            for n in ns:
                _solver_case(ck, pkg, dev, algo, sfx, n, True, flag, offset)
    ck.verify()


@pytest.mark.parametrize("sfx,offset", SFX_OFFSETS)
def test_grouped_solvers(pkg, dev, sfx, offset):
    """33 batches (one more than a launch carries) of sizes cycling 1, 0, 63, 257, 2: every
    H[i] back to back in one arena, 4 KiB of 0xA5 between neighbours."""
    dt = DT[sfx]
    sizes = [(1, 0, 63, 257, 2)[i % 5] for i in range(33)]
    P, st = ctypes.c_void_p * len(sizes), _st(dev)
    ck = Checks()
    for soa in (False, True):
        lay = "soa" if soa else "aos"
        srcs = [_rand(dev, (8, m) if soa else (m, 8), dt, seed=2 * i) for i, m in enumerate(sizes)]
        tars = [_rand(dev, (8, m) if soa else (m, 8), dt, seed=2 * i + 1) for i, m in enumerate(sizes)]
        keep = [t.clone() for t in srcs + tars]
        for algo in ALGOS[sfx]:
            for flag in (0, 1):
                want = [pkg.solve(algo, s, t, normalize=bool(flag), layout=lay) if m else
                        torch.empty((9, 0) if soa else (0, 9), dtype=dt, device=dev)
                        for s, t, m in zip(srcs, tars, sizes)]
                H = Arena(dev, [9 * m * ESIZE[dt] for m in sizes], offset)
                pkg._lib.call(f"hg_solve_grouped_{sfx}", ALGO_ID[algo],
                              P(*[t.data_ptr() if m else None for t, m in zip(srcs, sizes)]),
                              P(*[t.data_ptr() if m else None for t, m in zip(tars, sizes)]),
                              P(*[H.ptr(i) for i in range(len(sizes))]),
                              (ctypes.c_int64 * len(sizes))(*sizes), len(sizes), int(soa), flag, st)
                ck.outputs(f"hg_solve_grouped_{sfx} {algo} {lay} flags={flag} +{offset}", H, want)
        ck.inputs(f"hg_solve_grouped_{sfx} {lay}", srcs + tars, keep)
    ck.verify()


@pytest.mark.parametrize("sfx,offset", SFX_OFFSETS)
def test_solve_one(pkg, dev, sfx, offset):
    """H[9] of the latency path (src / tar read on the host)."""
    dt = DT[sfx]
    rng = np.random.default_rng(5)
    ck = Checks()
    for algo in ("aca", "sks"):
        for flag in (0, 1):
            s = (rng.random(8) * 1000).astype(np.float32 if sfx == "f32" else np.float64)
            t = (rng.random(8) * 1000).astype(s.dtype)
            want = pkg.solve(algo, torch.from_numpy(s[None]).to(dev), torch.from_numpy(t[None]).to(dev),
                             normalize=bool(flag))
            H = Arena(dev, 9 * ESIZE[dt], offset)
            pkg._lib.call(f"hg_solve_one_{sfx}", ALGO_ID[algo], s.ctypes.data, t.ctypes.data, H.ptr(),
                          flag, _st(dev))
            ck.outputs(f"hg_solve_one_{sfx} {algo} flags={flag} +{offset}", H, [want])
    ck.verify()


# -------------------------------------------------------------------- TensorACA, rectangle
RECT_B = (1, 63, 65, 255, 257)


def _rect_batch(pkg, dev, B, seed=0):
    torch.manual_seed(seed + B)
    _, _, src, tar, scale, div = pkg.adjust(dev, B)
    return src.contiguous(), tar.contiguous(), scale.contiguous(), div.contiguous()


def _vary(x, shape, dev, seed):
    """A (shape) tensor of values within 1 % of the one-value x."""
    return (x.reshape(()) * (1 + 0.01 * _rand(dev, shape, seed=seed, hi=1.0))).contiguous()


@pytest.mark.parametrize("offset", [0, 4])
def test_rect_forward(pkg, dev, offset):
    """H (B,3,3) of every forward: device scalars, host scalars (the square specialisation at
    div 1, and 1.25), scale / div per problem ((B,1,1)) and per row ((3,1)), and torch-ROCm's
    order.  kRectP = 1: one problem per lane, 256 per block."""
    ck, st = Checks(), _st(dev)
    for B in RECT_B:
        src, tar, scale, div = _rect_batch(pkg, dev, B)
        sv = float(scale.item())
        s_b, d_b = _vary(scale, (B, 1, 1), dev, 1), _vary(div, (B, 1, 1), dev, 2)
        s_r, d_r = _vary(scale, (3, 1), dev, 3), _vary(div, (3, 1), dev, 4)
        ins = [src, tar, scale, div, s_b, d_b, s_r, d_r]
        keep = [t.clone() for t in ins]
        sp, tp = src.data_ptr(), tar.data_ptr()
        cases = [
            ("hg_tensor_aca_rect_f32", pkg.tensor_aca_rect(src, tar, scale, div),
             lambda h: (sp, tp, h, B, scale.data_ptr(), div.data_ptr())),
            ("hg_tensor_aca_rect_f32_hostscalar div=1", pkg.tensor_aca_rect(src, tar, sv, 1.0),
             lambda h: (sp, tp, h, B, sv, 1.0)),
            ("hg_tensor_aca_rect_f32_hostscalar div=1.25", pkg.tensor_aca_rect(src, tar, sv, 1.25),
             lambda h: (sp, tp, h, B, sv, 1.25)),
            ("hg_tensor_aca_rect_bcast_f32 (B,1,1)", pkg.tensor_aca_rect(src, tar, s_b, d_b),
             lambda h: (sp, tp, h, B, s_b.data_ptr(), 1, 0, d_b.data_ptr(), 1, 0)),
            ("hg_tensor_aca_rect_bcast_f32 (3,1)", pkg.tensor_aca_rect(src, tar, s_r, d_r),
             lambda h: (sp, tp, h, B, s_r.data_ptr(), 0, 1, d_r.data_ptr(), 0, 1)),
            ("hg_tensor_aca_rect_order_f32 rocm", pkg.tensor_aca_rect(src, tar, scale, div, order="rocm"),
             lambda h: (sp, tp, h, B, scale.data_ptr(), 0, 0, div.data_ptr(), 0, 0, 1)),
        ]
        for name, want, args in cases:
            H = Arena(dev, 36 * B, offset)
            pkg._lib.call(name.split()[0], *args(H.ptr()), st)
            ck.outputs(f"{name} B={B} +{offset}", H, [want])
        ck.inputs(f"rect forward B={B}", ins, keep)
    ck.verify()


@pytest.mark.parametrize("offset", [0, 4])
def test_rect_backward(pkg, dev, offset):
    """grad_tar, grad_src (also NULL) and the scale / div gradient layouts: (2,B) sums, (2,B,3)
    terms, and the broadcast backward's per-parameter modes 0 (B), 1 (3,B), 2 (B,3); the
    torch-ROCm order with one (2,B,3) buffer (the staged form) and with separate ones."""
    ck = Checks()
    for B in RECT_B:
        src, tar, scale, div = _rect_batch(pkg, dev, B, seed=7)
        gH = _rand(dev, (B, 3, 3), seed=B, lo=-1.0, hi=1.0)
        s_b, d_b = _vary(scale, (B, 1, 1), dev, 1), _vary(div, (B, 1, 1), dev, 2)
        s_r, d_r = _vary(scale, (3, 1), dev, 3), _vary(div, (3, 1), dev, 4)
        head = (src.data_ptr(), tar.data_ptr(), gH.data_ptr(), B)
        sd = (scale.data_ptr(), div.data_ptr())
        ins = [src, tar, gH, scale, div, s_b, d_b, s_r, d_r]
        for want_src in (True, False):
            gs = (12 * B, F32) if want_src else None
            tag = f"B={B} grad_src={'yes' if want_src else 'NULL'} +{offset}"

            def run(name, build, outs, label):
                outs = dict(grad_src=gs, grad_tar=(12 * B, F32), **outs)
                fresh_vs_arena(ck, f"{label} {tag}", pkg, dev, name, build, outs,
                               {k: offset for k in outs}, ins)

            run("hg_tensor_aca_rect_backward_f32",
                lambda p: head + sd + (p["grad_src"], p["grad_tar"], p["sums"]),
                {"sums": (2 * B, F32)}, "hg_tensor_aca_rect_backward_f32")
            run("hg_tensor_aca_rect_backward_f32",
                lambda p: head + sd + (p["grad_src"], p["grad_tar"], None), {},
                "hg_tensor_aca_rect_backward_f32 no sums")
            run("hg_tensor_aca_rect_backward_terms_f32",
                lambda p: head + sd + (p["grad_src"], p["grad_tar"], p["terms"]),
                {"terms": (6 * B, F32)}, "hg_tensor_aca_rect_backward_terms_f32")
            # the broadcast backward: mode 0 with (B,1,1) parameters, 1 with (3,1), 2 with one value
            for mode, (sc, dv, sb, sr), count in ((0, (s_b, d_b, 1, 0), B), (1, (s_r, d_r, 0, 1), 3 * B),
                                                  (2, (scale, div, 0, 0), 3 * B)):
                for order in (None, 0, 1):
                    name = ("hg_tensor_aca_rect_bcast_backward_f32" if order is None
                            else "hg_tensor_aca_rect_backward_order_f32")
                    tail = () if order is None else (order,)
                    run(name,
                        lambda p: head + (sc.data_ptr(), sb, sr, dv.data_ptr(), sb, sr, p["grad_src"],
                                          p["grad_tar"], p["grad_scale"], mode, p["grad_div"], mode) + tail,
                        {"grad_scale": (count, F32), "grad_div": (count, F32)},
                        f"{name} mode {mode} order {order}")
            # torch-ROCm order, one value each, grad_div = grad_scale + 3B: the one-value staged form
            run("hg_tensor_aca_rect_backward_order_f32",
                lambda p: head + (sd[0], 0, 0, sd[1], 0, 0, p["grad_src"], p["grad_tar"], p["terms"], 2,
                                  p["terms"] + 12 * B, 2, 1),
                {"terms": (6 * B, F32)}, "hg_tensor_aca_rect_backward_order_f32 rocm paired")
            run("hg_tensor_aca_rect_backward_order_f32",
                lambda p: head + (sd[0], 0, 0, sd[1], 0, 0, p["grad_src"], p["grad_tar"], None, 2, None, 2, 1),
                {}, "hg_tensor_aca_rect_backward_order_f32 rocm no terms")
    ck.verify()


@pytest.mark.parametrize("offset", [0, 4])
def test_rect_backward_sum(pkg, dev, offset):
    """The fused all-gradient backward: a workspace of EXACTLY 6B floats (scratch: guards
    only), grad_sd[2], grad_tar, grad_src (also NULL).  Aligned buffers take the fused kernel;
    +4 takes the two-launch form (terms kernel into the workspace, then the ATen-order sum)."""
    ck = Checks()
    for B, T in ((1, 1), (5, 1), (171, 1), (10923, 1), (10924, 2), (43691, 16), (65536, 64)):
        src, tar, scale, div = _rect_batch(pkg, dev, B, seed=3)
        gH = _rand(dev, (B, 3, 3), seed=B, lo=-1.0, hi=1.0)
        for want_src in (True, False):
            outs = {"grad_src": (12 * B, F32) if want_src else None, "grad_tar": (12 * B, F32),
                    "grad_sd": (2, F32)}
            fresh_vs_arena(
                ck, f"hg_tensor_aca_rect_backward_sum_f32 B={B} T={T} src={want_src} +{offset}", pkg, dev,
                "hg_tensor_aca_rect_backward_sum_f32",
                lambda p: (src.data_ptr(), tar.data_ptr(), gH.data_ptr(), B, scale.data_ptr(),
                           div.data_ptr(), p["grad_src"], p["grad_tar"], p["workspace"], 8, T,
                           p["grad_sd"]),
                outs, {k: offset for k in ("grad_src", "grad_tar", "grad_sd", "workspace")},
                [src, tar, gH, scale, div], {"workspace": (6 * B, F32)})
    ck.verify()


# ---------------------------------------------------------------------------------- the sums
def _terms(dev, count, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(count, generator=g, device=dev) * 10.0


@pytest.mark.parametrize("offset", [0, 4])
def test_sum_aten(pkg, dev, offset):
    """hg_sum_aten_f32 uses x as the scratch of its levels: x spans exactly (rows - 1)
    row_stride + (m - 1) elem_stride + 1 floats, out[rows].  Run lengths around the level
    blocks and kAtenGrain (where threads > 1 start chunking), one and two rows (with a hole
    between them), and the one-lane column form (elem stride 3)."""
    ck = Checks()
    for m in (1, 33, 4097, 32767, 32768, 65537):
        for T in (1, 2, 16):
            for rows in (1, 2):
                rs = m + 3 if rows == 2 else 0
                span = (rows - 1) * rs + (m - 1) + 1
                fresh_vs_arena(ck, f"hg_sum_aten_f32 m={m} T={T} rows={rows} +{offset}", pkg, dev,
                               "hg_sum_aten_f32",
                               lambda p: (p["x"], rows, m, rs, 1, 8, T, p["out"]),
                               {"out": (rows, F32)}, {"x": offset, "out": offset}, (),
                               {"x": _terms(dev, span, m + T)})
    for B in (5, 1000):
        fresh_vs_arena(ck, f"hg_sum_aten_f32 columns B={B} +{offset}", pkg, dev, "hg_sum_aten_f32",
                       lambda p: (p["x"], 3, B, 1, 3, 1, 1, p["out"]),
                       {"out": (3, F32)}, {"x": offset, "out": offset}, (),
                       {"x": _terms(dev, 2 + 3 * (B - 1) + 1, B)})
    ck.verify()


@pytest.mark.parametrize("offset", [0, 4])
def test_sum_rows(pkg, dev, offset):
    """hg_sum_rows_f32: x (rows, cols) is overwritten with chunk sums (chunks of 4096), out[rows]."""
    ck = Checks()
    for rows, cols in ((2, 1), (2, 4095), (2, 4097), (3, 8193)):
        fresh_vs_arena(ck, f"hg_sum_rows_f32 ({rows},{cols}) +{offset}", pkg, dev, "hg_sum_rows_f32",
                       lambda p: (p["x"], rows, cols, p["out"]),
                       {"out": (rows, F32)}, {"x": offset, "out": offset}, (),
                       {"x": _terms(dev, rows * cols, cols)})
    ck.verify()


@pytest.mark.parametrize("offset", [0, 4])
def test_sum_rocm(pkg, dev, offset):
    """hg_sum_rocm_f32, FULL and COLS: x (any alignment) unchanged, out[1] / out[3], and the
    HG_SUM_ROCM_WORKSPACE floats of CTA partials (used by FULL at the two largest B)."""
    ck, st = Checks(), _st(dev)
    for B in (1, 2, 7, 4096, 65536, 300000):
        data = _terms(dev, 3 * B, B)
        for kind, nout in ((0, 1), (1, 3)):
            want = torch.empty(nout, device=dev)
            ws0 = torch.empty(1024, device=dev)
            pkg._lib.call("hg_sum_rocm_f32", data.data_ptr(), B, kind, want.data_ptr(), ws0.data_ptr(), st)
            x = Arena(dev, 12 * B, offset).put(data)
            out, ws = Arena(dev, 4 * nout, offset), Arena(dev, 4 * 1024, offset)
            pkg._lib.call("hg_sum_rocm_f32", x.ptr(), B, kind, out.ptr(), ws.ptr(), st)
            label = f"hg_sum_rocm_f32 B={B} kind={kind} +{offset}"
            ck.outputs(f"{label} out", out, [want])
            ck.outputs(f"{label} x", x, [data])
            ck.scratch(f"{label} workspace", ws)
    ck.verify()


# ------------------------------------------------------------------------ TensorACA, offsets
@pytest.mark.parametrize("offset", [0, 4])
def test_offsets_forward_and_backward(pkg, dev, offset):
    """H (B,3,3), grad_offsets (B,4,2) and grad_corner (B,2) (also NULL; 8-B aligned, so it
    stays at offset 0): the square and the general rectangle."""
    ck, st = Checks(), _st(dev)
    for B in (1, 127, 129, 257):
        corner = _rand(dev, (B, 2), seed=B, lo=10.0, hi=30.0)
        offs = _rand(dev, (B, 4, 2), seed=B + 1, lo=0.0, hi=32.0)
        gH = _rand(dev, (B, 3, 3), seed=B + 2, lo=-1.0, hi=1.0)
        ins = [corner, offs, gH]
        keep = [t.clone() for t in ins]
        for w, h in ((128.0, 128.0), (128.0, 96.0)):
            want = pkg.tensor_aca_offsets(corner, offs, w, h)
            H = Arena(dev, 36 * B, offset)
            pkg._lib.call("hg_tensor_aca_offsets_f32", corner.data_ptr(), offs.data_ptr(), H.ptr(), B, w, h, st)
            ck.outputs(f"hg_tensor_aca_offsets_f32 B={B} {w}x{h} +{offset}", H, [want])
            for need_corner in (True, False):
                g_off, g_cor = pkg.tensor_aca_offsets_backward(corner, offs, gH, w, h, need_corner)
                go = Arena(dev, 32 * B, offset)
                gc = Arena(dev, 8 * B, 0) if need_corner else None
                pkg._lib.call("hg_tensor_aca_offsets_backward_f32", corner.data_ptr(), offs.data_ptr(),
                              gH.data_ptr(), B, w, h, go.ptr(), gc.ptr() if gc else None, st)
                label = f"hg_tensor_aca_offsets_backward_f32 B={B} {w}x{h} corner={need_corner} +{offset}"
                ck.outputs(f"{label} grad_offsets", go, [g_off])
                if gc:
                    ck.outputs(f"{label} grad_corner", gc, [g_cor])
        ck.inputs(f"offsets B={B}", ins, keep)
    ck.verify()


# ------------------------------------------------------------------- general-quad ACA backward
@pytest.mark.parametrize("sfx,offset", SFX_OFFSETS)
def test_aca_backward(pkg, dev, sfx, offset):
    """grad_src, grad_tar (n,8), each also NULL: binary32's LDS-staged kernel when every buffer
    is 16-B aligned, the per-lane kernel otherwise and for binary64."""
    dt = DT[sfx]
    ck, st = Checks(), _st(dev)
    for n in (1, 63, 65, 257):
        src, tar = _rand(dev, (n, 8), dt, seed=n), _rand(dev, (n, 8), dt, seed=n + 1)
        gH = _rand(dev, (n, 9), dt, seed=n + 2, lo=-1.0, hi=1.0)
        ins = [src, tar, gH]
        keep = [t.clone() for t in ins]
        for need_src, need_tar in ((True, True), (True, False), (False, True)):
            g_src, g_tar = pkg.aca_backward(src, tar, gH, need_src, need_tar)
            a_src = Arena(dev, 8 * n * ESIZE[dt], offset) if need_src else None
            a_tar = Arena(dev, 8 * n * ESIZE[dt], offset) if need_tar else None
            pkg._lib.call(f"hg_aca_backward_{sfx}", src.data_ptr(), tar.data_ptr(), gH.data_ptr(), n,
                          a_src.ptr() if a_src else None, a_tar.ptr() if a_tar else None, st)
            label = f"hg_aca_backward_{sfx} n={n} src={need_src} tar={need_tar} +{offset}"
            if a_src:
                ck.outputs(f"{label} grad_src", a_src, [g_src])
            if a_tar:
                ck.outputs(f"{label} grad_tar", a_tar, [g_tar])
        ck.inputs(f"hg_aca_backward_{sfx} n={n}", ins, keep)
    ck.verify()


# -------------------------------------------------------------------------------- generators
@pytest.mark.parametrize("offset", [0, 4])
def test_generators(pkg, dev, offset):
    """out[count] of the uniform stream and of the MRG32K3A words (word i = position i / 2^17
    of subsequence i % 2^17: counts around 2^17 add the second position)."""
    ck, st = Checks(), _st(dev)
    for count in (1, 2, 3, 255, 257, 131071, 131073):
        want = pkg.fill_uniform(count, seed=5, offset=3, lo=-1.0, hi=2.0, device=dev)
        out = Arena(dev, 4 * count, offset)
        pkg._lib.call("hg_fill_uniform_f32", out.ptr(), count, 5, 3, -1.0, 2.0, st)
        ck.outputs(f"hg_fill_uniform_f32 count={count} +{offset}", out, [want])
        want = pkg.rand_mrg32k3a(count, seed=11, device=dev)
        out = Arena(dev, 4 * count, offset)
        pkg._lib.call("hg_rand_mrg32k3a_u32", out.ptr(), count, 11, st)
        ck.outputs(f"hg_rand_mrg32k3a_u32 count={count} +{offset}", out, [want])
    ck.verify()


# ----------------------------------------------------------------------------- RANSAC pieces
def test_samplers(pkg, dev):
    """H (n,9) of the indexed and the seeded fused sampler (16-B aligned by contract: offset 0),
    ACA and SKS: a 4-point pool (kept in LDS) and 20 000 points (gathered from global memory)."""
    ck, st = Checks(), _st(dev)
    for npool in (4, 20000):
        ps, pt = _rand(dev, (npool, 2), seed=npool), _rand(dev, (npool, 2), seed=npool + 1)
        for n in (1, 127, 129, 255, 257):
            idx = pkg.fill_bits(4 * n, 7, 0, dev).view(n, 4)
            ins = [ps, pt, idx]
            keep = [t.clone() for t in ins]
            for algo_id, algo in ((0, "aca"), (1, "sks")):
                for flag in (0, 1):
                    label = f"npool={npool} n={n} {algo} flags={flag}"
                    want = pkg.sample_solve(ps, pt, idx, algo=algo, normalize=bool(flag))
                    H = Arena(dev, 36 * n)
                    pkg._lib.call("hg_sample_solve_f32", ps.data_ptr(), pt.data_ptr(), npool,
                                  idx.data_ptr(), H.ptr(), n, algo_id, flag, st)
                    ck.outputs(f"hg_sample_solve_f32 {label}", H, [want])
                    want = pkg.sample_solve_seeded(ps, pt, n, 7, 3, algo=algo, normalize=bool(flag))
                    H = Arena(dev, 36 * n)
                    pkg._lib.call("hg_sample_solve_seeded_f32", ps.data_ptr(), pt.data_ptr(), npool, 7, 3,
                                  H.ptr(), n, algo_id, flag, st)
                    ck.outputs(f"hg_sample_solve_seeded_f32 {label}", H, [want])
            ck.inputs(f"samplers npool={npool} n={n}", ins, keep)
    ck.verify()


def test_seeded_sampler_packed_pair_shape(pkg, dev):
    """n = 2^22 + 129: past kSeededPairMinN the seeded ACA launch takes the 4-wave packed-pair
    shape (SKS packs pairs at every size).  151 MB of H, compared on the device."""
    g = load_golden("cpp_wall.npz")
    ps, pt = torch.from_numpy(g["pool_src"]).to(dev), torch.from_numpy(g["pool_tar"]).to(dev)
    keep = [ps.clone(), pt.clone()]
    n = (1 << 22) + 129
    ck = Checks()
    for algo_id, algo in ((0, "aca"), (1, "sks")):
        want = pkg.sample_solve_seeded(ps, pt, n, 11, 3, algo=algo)
        H = Arena(dev, 36 * n)
        pkg._lib.call("hg_sample_solve_seeded_f32", ps.data_ptr(), pt.data_ptr(), ps.shape[0], 11, 3,
                      H.ptr(), n, algo_id, 1, _st(dev))
        ck.outputs(f"hg_sample_solve_seeded_f32 {algo} n=2^22+129", H, [want])
        del H, want
    ck.inputs("seeded sampler", [ps, pt], keep)
    ck.verify()


@pytest.mark.parametrize("offset", [0, 4])
def test_scorer(oracle, pkg, dev, offset):
    """counts[n]: two hypotheses per lane, 512 per block; pools around the unroll of 8 and the
    empty pool.  The counts also equal the oracle's."""
    ck, st = Checks(), _st(dev)
    for n in (1, 2, 511, 512, 513):
        H = pkg.solve("aca", _rand(dev, (n, 8), seed=n), _rand(dev, (n, 8), seed=n + 1))
        for npool in (0, 7, 8, 9):
            ps, pt = _rand(dev, (npool, 2), seed=npool), _rand(dev, (npool, 2), seed=npool + 50)
            ins = [H, ps, pt]
            keep = [t.clone() for t in ins]
            want = pkg.ransac_score(H, ps, pt, 300.0)
            counts = Arena(dev, 4 * n, offset)
            pkg._lib.call("hg_ransac_score_f32", H.data_ptr(), n, ps.data_ptr() if npool else None,
                          pt.data_ptr() if npool else None, npool, 300.0, counts.ptr(), st)
            label = f"hg_ransac_score_f32 n={n} npool={npool} +{offset}"
            ck.outputs(label, counts, [want])
            ck.inputs(label, ins, keep)
            ref = oracle.ransac_score(H.cpu().numpy(), ps.cpu().numpy().reshape(npool, 2),
                                      pt.cpu().numpy().reshape(npool, 2), 300.0)
            ck.add(f"{label}: counts differ from the oracle",
                   (want == torch.from_numpy(ref.view(np.int32)).to(dev)).all())
    ck.verify()


# ------------------------------------------------------------------- the Table-8 pipeline
@pytest.mark.parametrize("offset", [0, 8])
@pytest.mark.parametrize("size", [97, 20000])
def test_table8(pkg, dev, size, offset):
    """d_src / d_tar (8,n) of get_rand_list and H (9,n) of the two fused forms (per-row buffer
    stores), four solvers, both flags: a 97-point pool (kept in LDS, persistent grid) and
    20 000 points (gathered from global memory); n around the blocks and the MRG order 2^17."""
    ck, st = Checks(), _st(dev)
    ps, pt = _rand(dev, (size, 2), F64, seed=size), _rand(dev, (size, 2), F64, seed=size + 1)
    for n in (1, 4095, 4097, 131071, 131073):
        rl = pkg.rand_mrg32k3a(4 * n, seed=11, device=dev).view(4, n)
        ins = [ps, pt, rl]
        keep = [t.clone() for t in ins]
        w_src, w_tar = pkg.get_rand_list(rl, ps, pt)
        d_src, d_tar = Arena(dev, 64 * n, offset), Arena(dev, 64 * n, offset)
        pkg._lib.call("hg_get_rand_list_f64", rl.data_ptr(), size, ps.data_ptr(), pt.data_ptr(),
                      d_src.ptr(), d_tar.ptr(), n, st)
        ck.outputs(f"hg_get_rand_list_f64 n={n} d_src", d_src, [w_src])
        ck.outputs(f"hg_get_rand_list_f64 n={n} d_tar", d_tar, [w_tar])
        del d_src, d_tar, w_src, w_tar
        for algo in ALGOS["f64"]:
            for flag in (0, 1):
                want = pkg.gather_solve(ps, pt, rl, algo=algo, normalize=bool(flag))
                H = Arena(dev, 72 * n, offset)
                pkg._lib.call("hg_gather_solve_f64", ALGO_ID[algo], ps.data_ptr(), pt.data_ptr(), size,
                              rl.data_ptr(), H.ptr(), n, flag, st)
                ck.outputs(f"hg_gather_solve_f64 {algo} n={n} flags={flag}", H, [want])
                want = pkg.rand_gather_solve(ps, pt, n, seed=11, algo=algo, normalize=bool(flag))
                H = Arena(dev, 72 * n, offset)
                pkg._lib.call("hg_rand_gather_solve_f64", ALGO_ID[algo], ps.data_ptr(), pt.data_ptr(),
                              size, 11, H.ptr(), n, flag, st)
                ck.outputs(f"hg_rand_gather_solve_f64 {algo} n={n} flags={flag}", H, [want])
        ck.inputs(f"table 8 n={n}", ins, keep)
    ck.verify()


# -------------------------------------------------------------------------------- stream copy
def test_stream_copy(pkg, dev):
    """dst of the float4 copy (16-B aligned, a multiple of 16 bytes by contract)."""
    ck = Checks()
    for nbytes in (16, 4080, 65552):
        src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device=dev)
        keep = src.clone()
        dst = Arena(dev, nbytes)
        pkg._lib.call("hg_stream_copy", src.data_ptr(), dst.ptr(), nbytes, _st(dev))
        ck.outputs(f"hg_stream_copy {nbytes} B", dst, [src])
        ck.inputs(f"hg_stream_copy {nbytes} B", [src], [keep])
    ck.verify()
