"""The operator route -- cm_selective_scan_fwd / _bwd and cm_causal_conv1d_fwd / _bwd, the drop-in ABI and every layer the gates send
off the rows route -- at every compiled instance, held to the fp64 oracle (oracle/conmamba_oracle.py) under guard bands.

Every launch is tests/guard_bands.two_step through the wrappers' ``bufs``: a plain launch, then the same launch with every
floating-point input inside NaN, every output inside sentinels and the workspace NaN inside sentinels.  The second launch must give the
first one's bits, finite, with nothing outside written; the first is held to the oracle.  Without the workspace the parameter
gradients are fp32 atomics whose order is free, so there they are held to the oracle in both launches instead of to each other's bits.

Instances (restated from the dispatch tables, looped over below, nothing skipped)
  scan forward   dstate 16 x split {1, 2, 4, 8, 16}, dstate 8 x {1, 2, 4, 8}  x  {fp32/fp32, bf16/bf16, bf16 with fp32 B/C}  x  both
                 directions on the vector path; the element path exists for split 4 only (the library takes 4 whenever a row is not
                 whole aligned vectors, csrc/selective_scan_fwd.hip:46), so odd L run once per dstate, pair and direction.
  scan backward  (16,4) (16,8) (16,16) (8,4) (8,8)  x  the three pairs  x  both directions, each on the vector and the element path
                 (one kernel, a run-time flag), each with the workspace and without it.
  conv           width {2, 3, 4} x {fp32, bf16, fp16} x direction; forward on the vector and the element path; the backward has
                 one element-wise kernel per (width, type, direction).  ops reaches fp16 (ops._DT), so nothing compiled is unreachable.
The split the library runs is restated (fwd_split / bwd_split, csrc/selective_scan_fwd.hip:12-22, selective_scan_bwd.hip:10-19); the
backward's is observable and checked through cm_selective_scan_bwd_workspace_bytes (gx depends on it); the forward reports nothing.

Shapes.  C = 4 x 64 / S channels per workgroup.  The time sweep L = 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 128, 129 (vector width, 8-step
sub-block, 64-step checkpoint chunk, each -1 / 0 / +1) runs at dim C + 1 (two workgroups, the second with one live channel: the
dB / dC fold has gx = 2) in _MambaInner's layout; dim 1 and dim C run once each; the forward adds its tile 16 S at -1 / 0 / +1 and at
+-8 (the nearest lengths that stay on the vector path).  Odd L takes the element path; L = 64 with every view one element off
alignment forces it once per pair.  Batch 2 (forward) and 3 (backward: dA, dD, ddelta_bias sum over the batch).
Layouts: contiguous once per instance; otherwise _MambaInner's: u, delta, dout, du, ddelta, out, out_z are (batch, dim, L) views of
(dim, batch, L) storage, B and C (batch, 1, n, L) views of (n, batch, L) storage, z and dz second halves of a (batch, 2 dim, L) tensor.
There the element behind a row is the next utterance's: NaN in the guarded launch.
h0 is a random state handed to the oracle as initial_state (tests/test_seqpar.py's reference: the chunks of one sequence chained by it).
Reverse cases hand the kernel the oracle's inputs flipped in time, so one oracle run serves both directions.  bf16 inputs are rounded
before the oracle sees them.  The backward reads the checkpoints x of the ORACLE (rounded to fp32), not of the forward kernel.

Bounds (tests/test_hip_ops.py's figures, not tuned): scan forward and x 5e-5 + 2e-4 |ref|; scan backward 2e-4 max(1, max|ref|) +
2e-3 |ref| per tensor; conv forward 1e-5 + 1e-5 |ref|; conv backward 1e-4 + 1e-4 |ref|, the atol x max(1, max|ref|) on dweight / dbias.
A bf16 / fp16 result adds half an ulp of the reference, 2^-8 |ref| / 2^-11 |ref|; fp32 gradients of bf16 runs keep the plain bound.
Parameter gradients are prefilled with random fp32 values and must come back as prefill + gradient.

Worst error / bound per kernel and result type, measured on an MI355X (the last test prints the table per instance; the log is
profiles/operator_kernels/test_operator_kernels_gpu.log):
  scan forward    out / out_z   fp32 0.047   bf16 0.946        x (fp32)  0.013
  scan backward   du / ddelta / dz bf16 0.624; fp32 results and every parameter gradient 0.002; recomputed out_z fp32 0.039, bf16 0.941
  conv forward    fp32 0.019   bf16 0.988   fp16 0.957
  conv backward   fp32 0.003   bf16 0.958   fp16 0.771 (dweight / dbias are fp32: within the fp32 figure)
The bf16 / fp16 figures are the final rounding (an allowance of half an ulp, errors up to half an ulp); the fp32 ones show the
arithmetic itself 20 to 500 times inside the project's bounds.  No instance missed its bound, so none was re-derived.
3230 two-launch cases (scan forward 782, scan backward 1080, conv 684 + 684); the whole file takes 12 s on an MI355X, its slowest test
(test_scan_fwd_instances[16-f32-fwd], which also computes the shared fp64 references) 1.2 s.
"""
import functools
import os
import sys

import pytest
import torch

from oracle import conmamba_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NAME = {BF16: "bf16", F16: "fp16", F32: "fp32"}
HALF_ULP = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
PAIRS = {"f32": (F32, F32), "bf16": (BF16, BF16), "bf16_f32": (BF16, F32)}          # (io, B/C)
FWD_INSTANCES = [(16, 1), (16, 2), (16, 4), (16, 8), (16, 16), (8, 1), (8, 2), (8, 4), (8, 8)]
BWD_INSTANCES = [(16, 4), (16, 8), (16, 16), (8, 4), (8, 8)]
SCAN_L = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 128, 129)
CONV_L = (1, 2, 3, 4, 7, 8, 9, 1023, 1024, 1025)
CK = 64                                     # CM_SCAN_CHUNK
BMAX, DMAX = 3, 257                         # the data of one (dstate, pair, L): every case is a [:batch, :dim] slice of it
FWD_TOL, BWD_TOL, CONV_FWD_TOL, CONV_BWD_TOL = (2e-4, 5e-5), (2e-3, 2e-4), (1e-5, 1e-5), (1e-4, 1e-4)
WORST = {}                                  # (kernel, instance, result dtype) -> worst error / bound
CASES = {}                                  # kernel -> two-launch cases


def fwd_split(batch, dim, dstate, want):
    """cm_scan_pick_split: a requested power of two clamped to min(dstate, 16); else the smallest split with 1024 waves."""
    smax = min(dstate, 16)
    if want >= 1 and want & (want - 1) == 0:
        return min(want, smax)
    s = 1
    while s < smax and batch * -(-dim // (64 // s)) < 1024:
        s *= 2
    return s


def bwd_split(batch, dim, dstate, want):
    """bwd_split: the forward's pick, at least 4, at least 8 when the caller did not ask, at most dstate."""
    s = max(fwd_split(batch, dim, dstate, want), 4)
    if s < 8 and want == 0:
        s = 8
    return min(s, dstate)


def vec_of(io, bc=None):
    return max(4 if io == F32 else 8, 4 if bc in (None, F32) else 8)


def dev(t):
    return None if t is None else t.to(DEV)


def cpu64(t):
    return t.detach().double().cpu()


def flip(t, rev):
    return t.flip(-1) if (rev and t is not None) else t


def bound_of(ref, tol, res_dtype, scaled=False):
    rtol, atol = tol
    if scaled:
        atol = atol * max(1.0, float(ref.abs().max()))
    return atol + (rtol + HALF_ULP[res_dtype]) * ref.abs()


def within(kernel, inst, name, got, ref, tol, scaled=False, tag=""):
    """|got - ref| <= bound element by element; records the worst ratio per (kernel, instance, result dtype)."""
    bound = bound_of(ref, tol, got.dtype, scaled)
    err = (cpu64(got) - ref).abs()
    assert err.shape == bound.shape, (kernel, name, err.shape, bound.shape)
    worst = float((err / bound).max()) if err.numel() else 0.0
    key = (kernel, inst, NAME[got.dtype])
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if not worst <= 1.0:
        ratio = err / bound
        at = tuple(int(i) for i in (~(ratio <= 1)).nonzero()[0])
        raise AssertionError(f"{kernel} {inst} {name} {tag}: error / bound {worst:.3f}; first over at {at}: got {float(cpu64(got)[at])!r}, "
                             f"ref {float(ref[at])!r}, bound {float(bound[at]):.3e}; {int((~(ratio <= 1)).sum())} of {ratio.numel()} over")


def two_step(kernel, run, loose=(), held=None):
    """G.two_step; ``loose``: outputs whose bits the two launches need not share (atomics): ``held(name, tensor, which)`` holds both."""
    CASES[kernel] = CASES.get(kernel, 0) + 1
    plain, guard = G.Launch(False, DEV), G.Launch(True, DEV)
    try:
        run(plain)
        run(guard)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):          # a faulted device: nothing more is launched on it
            pytest.exit(f"{kernel}: the device reported {e}", returncode=3)
        raise
    for name in loose:
        held(name, guard.outs[name], "guarded launch")
    guard.g.check({k: (guard.outs[k].clone() if k in loose else v) for k, v in plain.outs.items()})
    return plain.outs


def row_align(l, dtype):
    """Rows of l + LEFT + RIGHT elements start 16-byte aligned only when that is whole 16-byte vectors."""
    size = torch.empty((), dtype=dtype).element_size()
    return 16 if ((l + G.LEFT + G.RIGHT) * size) % 16 == 0 else size


def half_in(L, t, first):
    """t (batch, dim, time) as one half of a (batch, 2 dim, time) tensor whose other half the kernel must not read (NaN when guarded)."""
    if t is None:
        return None
    b, d, l = t.shape
    other = torch.full_like(t, float("nan") if L.guard else 0.0)
    both = torch.cat([t, other] if first else [other, t], dim=1)
    both = G.poisoned(both, rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT, align=row_align(l, t.dtype)) if L.guard else both.clone()
    return both[:, :d] if first else both[:, d:]


def half_out(L, name, shape, dtype, first):
    """An output that is one half of a (batch, 2 dim, time) tensor; the other half starts as zeros and must stay so."""
    b, d, l = shape
    both = L.out(name, (b, 2 * d, l), dtype, fill=0, rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT, align=row_align(l, dtype))
    return both[:, :d] if first else both[:, d:]


# ------------------------------------------------------------------------------------------------------------------------------
# selective scan: data and fp64 references
# ------------------------------------------------------------------------------------------------------------------------------
class Opts:
    """Which optional inputs a case has."""

    def __init__(self, z=True, D=True, bias=True, softplus=True, h0=False):
        self.z, self.D, self.bias, self.softplus, self.h0 = z, D, bias, softplus, h0
        self.key = (z, D, bias, softplus, h0)

    def __repr__(self):
        return "".join(c if on else "-" for c, on in zip("zDbsh", self.key))


ALL = Opts()
VARIANTS = [Opts(z=False), Opts(D=False), Opts(bias=False), Opts(softplus=False, bias=False)]


@functools.lru_cache(maxsize=None)
def scan_data(n, pair, l):
    """The existing generators (tests/test_hip_ops.py): A = -exp(0.3 randn), delta = 0.5 randn, bias = randn - 1; values as the kernel
    sees them (rounded to the pair's types), held in fp32."""
    io, bc = PAIRS[pair]
    g = torch.Generator().manual_seed(1000 * n + 7 * l + len(pair))
    r = lambda *s: torch.randn(*s, generator=g)
    rio = lambda t: t.to(io).float()
    rbc = lambda t: t.to(bc).float()
    d = dict(u=rio(r(BMAX, DMAX, l)), delta=rio(r(BMAX, DMAX, l) * 0.5), z=rio(r(BMAX, DMAX, l)), dout=rio(r(BMAX, DMAX, l)),
             A=-torch.exp(r(DMAX, n) * 0.3), B=rbc(r(BMAX, n, l)), C=rbc(r(BMAX, n, l)), D=r(DMAX), bias=r(DMAX) - 1, h0=r(BMAX, DMAX, n))
    d["delta_lin"] = rio(d["delta"].abs() * 0.1)                # softplus off: a positive step, as test_scan_fwd_variants
    return d


def case_inputs(n, pair, l, o):
    d = scan_data(n, pair, l)
    return dict(u=d["u"], delta=d["delta"] if o.softplus else d["delta_lin"], A=d["A"], B=d["B"], C=d["C"], D=d["D"] if o.D else None,
                z=d["z"] if o.z else None, bias=d["bias"] if o.bias else None, h0=d["h0"] if o.h0 else None, dout=d["dout"])


def chunk_bounds(l, rev):
    """The steps of each checkpoint chunk in SCAN order and the chunk's index in x.  Forward: chunk c = steps 64 c .. ; reverse (scan
    order is descending time): the first steps scanned are the ragged LAST chunk, and x keeps the chunks indexed by time."""
    nch = -(-l // CK)
    if not rev:
        return [(c * CK, min(l, c * CK + CK), c) for c in range(nch)]
    r = l - CK * (nch - 1)
    return [(0, r, nch - 1)] + [(r + (k - 1) * CK, r + k * CK, nch - 1 - k) for k in range(1, nch)]


@functools.lru_cache(maxsize=None)
def _fwd_ref(n, pair, l, okey):
    """fp64 forward at (BMAX, DMAX) in scan order (channels are independent: cases slice it): the gated output and the forward chunking's
    x from one chunk-by-chunk oracle run, the pre-gate output and the reverse chunking's x from another (initial_state carries the
    state across, as tests/test_seqpar.py does; with h0 the first chunk starts from it)."""
    o = Opts(*okey)
    c = case_inputs(n, pair, l, o)
    dd = lambda t: None if t is None else t.double()
    u, dl, B, C, z = dd(c["u"]), dd(c["delta"]), dd(c["B"]), dd(c["C"]), dd(c["z"])
    A = c["A"].double()
    dtp = dl if c["bias"] is None else dl + c["bias"].double()[None, :, None]
    dtp = O.softplus(dtp) if o.softplus else dtp
    res = {}
    for rev, zz in ((False, z), (True, None)):
        h = dd(c["h0"])
        outs, x = [], torch.zeros(BMAX, DMAX, -(-l // CK), 2 * n, dtype=F64)
        for s0, s1, ci in chunk_bounds(l, rev):
            out, h = O.selective_scan(u[..., s0:s1], dl[..., s0:s1], A, B[..., s0:s1], C[..., s0:s1], c["D"], None if zz is None else zz[..., s0:s1],
                                      c["bias"], o.softplus, True, work_dtype=F64, initial_state=h)
            outs.append(out)
            x[:, :, ci, 0::2] = torch.exp(A[None] * dtp[..., s0:s1].sum(-1)[..., None])     # include/conmamba_hip.h:105-107
            x[:, :, ci, 1::2] = h
        res["x_rev" if rev else "x_fwd"] = x
        res["out" if zz is None else "out_z"] = torch.cat(outs, -1)
    return res


def fwd_ref(n, pair, l, o, batch, dim):
    return {k: v[:batch, :dim] for k, v in _fwd_ref(n, pair, l, o.key).items()}


@functools.lru_cache(maxsize=None)
def _bwd_ref(n, pair, l, okey, batch, dim):
    o = Opts(*okey)
    c = case_inputs(n, pair, l, o)
    s = lambda t: None if t is None else (t[:dim] if t.dim() < 3 else t[:batch, :dim])
    r = O.selective_scan_bwd(s(c["u"]), s(c["delta"]), s(c["A"]), c["B"][:batch], c["C"][:batch], s(c["D"]), s(c["z"]), s(c["bias"]), s(c["dout"]),
                             o.softplus)
    r["dB"], r["dC"] = r["dB"][:, None], r["dC"][:, None]
    return r


def bwd_ref(n, pair, l, o, batch, dim):
    return _bwd_ref(n, pair, l, o.key, batch, dim)


def place_scan_inputs(L, c, io, bc, batch, dim, rev, layout, shift):
    """The case's inputs on the device in the launch's layout -> dict."""
    act = lambda k: None if c[k] is None else dev(flip(c[k][:batch, :dim], rev).to(io).contiguous())
    bcv = lambda k: dev(flip(c[k][:batch], rev).to(bc).contiguous())
    p = dict(A=L.vec(dev(c["A"][:dim].contiguous())), D=L.vec(dev(None if c["D"] is None else c["D"][:dim].contiguous())),
             bias=L.vec(dev(None if c["bias"] is None else c["bias"][:dim].contiguous())),
             h0=None if c["h0"] is None else L.flat(dev(c["h0"][:batch, :dim].contiguous()), dim))
    if layout == "contig":
        p.update(u=L.flat(act("u"), CK), delta=L.flat(act("delta"), CK), z=L.flat(act("z"), CK), dout=L.flat(act("dout"), CK),
                 B=L.flat(bcv("B"), CK), C=L.flat(bcv("C"), CK))
    else:
        p.update(u=L.chan(act("u"), shift=shift), delta=L.chan(act("delta"), shift=shift), dout=L.chan(act("dout"), shift=shift),
                 z=half_in(L, act("z"), first=False), B=L.chan(bcv("B"), shift=shift).unsqueeze(1), C=L.chan(bcv("C"), shift=shift).unsqueeze(1))
    return p


def act_out(L, name, shape, dtype, layout, shift):
    if layout == "contig":
        return L.out(name, shape, dtype, rows=CK, contiguous=True)
    return L.out(name, shape, dtype, transposed=True, rows=1, shift=shift)


def scan_fwd_case(ops, n, split, pair, rev, l, batch, dim, o=ALL, layout="inner", shift=0, both=True):
    """One forward case: out and out_z together (``both``) or only what z decides, x always."""
    io, bc = PAIRS[pair]
    c = case_inputs(n, pair, l, o)
    inst = f"n{n} S{split} {pair} {'rev' if rev else 'fwd'}"
    tag = f"L={l} batch={batch} dim={dim} {o!r} {layout} shift={shift}"
    want_out = o.z is False or both

    def run(L):
        p = place_scan_inputs(L, c, io, bc, batch, dim, rev, layout, shift)
        bufs = dict(x=L.out("x", (batch, dim, -(-l // CK), 2 * n), F32, rows=CK, contiguous=True))
        if want_out:
            bufs["out"] = act_out(L, "out", (batch, dim, l), io, layout, shift)
        if o.z:
            bufs["out_z"] = act_out(L, "out_z", (batch, dim, l), io, layout, shift)
        out, x, out_z = ops.selective_scan_fwd(p["u"], p["delta"], p["A"], p["B"], p["C"], p["D"], p["z"], p["bias"], o.softplus, reverse=rev,
                                               need_out=want_out, h0=p["h0"], split=split, bufs=bufs)
        assert x.data_ptr() == bufs["x"].data_ptr() and (out is None) == (not want_out) and (out_z is None) == (not o.z)
        assert out is None or out.data_ptr() == bufs["out"].data_ptr()
        assert out_z is None or out_z.data_ptr() == bufs["out_z"].data_ptr()

    got = two_step("scan_fwd", run)
    ref = fwd_ref(n, pair, l, o, batch, dim)
    if want_out:
        within("scan_fwd", inst, "out", got["out"], flip(ref["out"], rev), FWD_TOL, tag=tag)
    if o.z:
        within("scan_fwd", inst, "out_z", got["out_z"], flip(ref["out_z"], rev), FWD_TOL, tag=tag)
    within("scan_fwd x", inst, "x", got["x"], ref["x_rev" if rev else "x_fwd"], FWD_TOL, tag=tag)


def fwd_lengths(n, split, pair):
    """The vector-path lengths of an instance: the sweep's and the tile's (16 S, +-8 beside it); -1 / +1 of the tile are odd and run
    what the library runs there (the split-4 element kernel)."""
    v, tile = vec_of(*PAIRS[pair]), 16 * split
    sweep = [l for l in SCAN_L if l % v == 0]
    edges = [l for l in (tile - 8, tile, tile + 8) if l > 0 and l % v == 0]
    return sorted(set(sweep + edges)), [tile - 1, tile + 1]


@pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("n", [16, 8])
def test_scan_fwd_instances(n, pair, rev):
    from mamba_asr_amd import ops
    for nn, split in FWD_INSTANCES:
        if nn != n:
            continue
        cpw = 4 * 64 // split
        assert fwd_split(2, cpw + 1, n, split) == split
        vec_l, odd_l = fwd_lengths(n, split, pair)
        for l in vec_l:
            scan_fwd_case(ops, n, split, pair, rev, l, 2, cpw + 1)
        for l in odd_l:
            scan_fwd_case(ops, n, split, pair, rev, l, 2, 5)
        scan_fwd_case(ops, n, split, pair, rev, 16 * split, 2, 1)
        scan_fwd_case(ops, n, split, pair, rev, 16 * split, 2, cpw, layout="contig")
        scan_fwd_case(ops, n, split, pair, rev, 64, 2, cpw, both=False)
    # the element path: split 4 whatever is asked
    cpw = 64
    for l in SCAN_L:
        if l % vec_of(*PAIRS[pair]) != 0:
            scan_fwd_case(ops, n, 4, pair, rev, l, 2, cpw + 1)
    scan_fwd_case(ops, n, 4, pair, rev, 9, 2, 1)
    scan_fwd_case(ops, n, 4, pair, rev, 65, 2, cpw, layout="contig")
    scan_fwd_case(ops, n, 4, pair, rev, 64, 2, cpw + 1, shift=1)                      # whole vectors, every view off alignment


@pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_scan_fwd_options(pair, rev):
    """z / D / delta_bias absent, softplus off, and an initial state, on the (16, 8) instance and on the element path."""
    from mamba_asr_amd import ops
    for o in VARIANTS + [Opts(h0=True)]:
        for l in (64, 129):
            scan_fwd_case(ops, 16, 8, pair, rev, l, 2, 33, o=o)
    scan_fwd_case(ops, 8, 4, pair, rev, 72, 2, 65, o=Opts(h0=True))


def scan_bwd_case(ops, n, split, pair, rev, l, batch, dim, det, o=ALL, layout="inner", shift=0, recompute=True):
    io, bc = PAIRS[pair]
    c = case_inputs(n, pair, l, o)
    inst = f"n{n} S{split} {pair} {'rev' if rev else 'fwd'} {'ws' if det else 'atomics'}"
    tag = f"L={l} batch={batch} dim={dim} {o!r} {layout} shift={shift}"
    fref, ref = fwd_ref(n, pair, l, o, batch, dim), bwd_ref(n, pair, l, o, batch, dim)
    xref = fref["x_rev" if rev else "x_fwd"].float()
    g = torch.Generator().manual_seed(l + dim)
    shapes = dict(dA=(dim, n), dB=(batch, 1, n, l), dC=(batch, 1, n, l))
    if o.D:
        shapes["dD"] = (dim,)
    if o.bias:
        shapes["ddelta_bias"] = (dim,)
    prefill = {k: torch.randn(*s, generator=g) for k, s in shapes.items()}
    want = {k: prefill[k].double() + (flip(ref[k], rev) if k in ("dB", "dC") else ref[k]) for k in shapes}
    recompute = recompute and o.z
    assert ops.DETERMINISTIC == det
    s_ran = bwd_split(batch, dim, n, split)
    assert s_ran == split
    nws = 2 * -(-dim // (4 * 64 // s_ran)) * batch * n * l + batch * dim * n + 2 * batch * dim

    def run(L):
        p = place_scan_inputs(L, c, io, bc, batch, dim, rev, layout, shift)
        bufs = dict(du=act_out(L, "du", (batch, dim, l), io, layout, shift), ddelta=act_out(L, "ddelta", (batch, dim, l), io, layout, shift))
        if o.z:
            bufs["dz"] = L.out("dz", (batch, dim, l), io, rows=CK, contiguous=True) if layout == "contig" else half_out(L, "dz", (batch, dim, l), io, first=False)
        if recompute:
            bufs["out_z"] = act_out(L, "out_z", (batch, dim, l), io, layout, shift)
        for k, s in shapes.items():
            bufs[k] = L.out(k, s, F32, fill=dev(prefill[k]), rows=CK, contiguous=True)
        if det:
            bufs["workspace"] = L.scratch("workspace", nws)         # a wrong size is refused by ops: the library's figure is the formula's
        r = ops.selective_scan_bwd(p["u"], p["delta"], p["A"], p["B"], p["C"], p["D"], p["z"], p["bias"], p["dout"], L.flat(dev(xref), CK), o.softplus,
                                   reverse=rev, recompute_out_z=recompute, split=split, bufs=bufs)
        du, ddelta, dA, dB, dC, dD, dbias, dz, out_z = r
        for t, k in ((du, "du"), (ddelta, "ddelta"), (dA, "dA"), (dB, "dB"), (dC, "dC"), (dD, "dD"), (dbias, "ddelta_bias"), (dz, "dz"), (out_z, "out_z")):
            assert (t is None) == (k not in bufs) and (t is None or t.data_ptr() == bufs[k].data_ptr()), k

    def held(k, t, which):
        within("scan_bwd", inst, k, t, want[k], BWD_TOL, scaled=True, tag=f"{tag} {which}")

    got = two_step("scan_bwd", run, loose=() if det else tuple(shapes), held=held)
    for k in ("du", "ddelta") + (("dz",) if o.z else ()):
        t = got[k][:, dim:] if (k == "dz" and layout != "contig") else got[k]
        if k == "dz" and layout != "contig":
            assert not bool(got[k][:, :dim].any()), "dz: the other half of dxz was written"
        within("scan_bwd", inst, k, t, flip(ref[k], rev), BWD_TOL, scaled=True, tag=tag)
    if recompute:
        within("scan_bwd out_z", inst, "out_z", got["out_z"], flip(fref["out_z"], rev), FWD_TOL, tag=tag)
    for k in shapes:
        held(k, got[k], "plain launch")


def scan_bwd_instance(ops, n, split, pair, rev, det):
    cpw = 4 * 64 // split
    for l in SCAN_L:
        scan_bwd_case(ops, n, split, pair, rev, l, 3, cpw + 1, det)
    scan_bwd_case(ops, n, split, pair, rev, 64, 3, 1, det)
    scan_bwd_case(ops, n, split, pair, rev, 9, 3, 1, det, recompute=False)
    scan_bwd_case(ops, n, split, pair, rev, 64, 3, cpw, det, layout="contig")
    scan_bwd_case(ops, n, split, pair, rev, 65, 3, cpw, det, layout="contig", recompute=False)


@pytest.mark.parametrize("det", [True, False], ids=["workspace", "atomics"])
@pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("n,split", BWD_INSTANCES)
def test_scan_bwd_instances(n, split, pair, rev, det, monkeypatch):
    from mamba_asr_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", det)
    scan_bwd_instance(ops, n, split, pair, rev, det)


@pytest.mark.parametrize("det", [True, False], ids=["workspace", "atomics"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_scan_bwd_options(pair, det, monkeypatch):
    """z / D / delta_bias absent and softplus off on the default instance (16, 8), both directions; the forced element path (L = 64,
    every view one element off alignment) once per pair."""
    from mamba_asr_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", det)
    for rev in (False, True):
        for o in VARIANTS:
            scan_bwd_case(ops, 16, 8, pair, rev, 72, 3, 33, det, o=o)
            scan_bwd_case(ops, 16, 8, pair, rev, 9, 3, 33, det, o=o)
        scan_bwd_case(ops, 16, 8, pair, rev, 64, 3, 33, det, shift=1)
        scan_bwd_case(ops, 8, 4, pair, rev, 64, 3, 65, det, shift=1)


# ------------------------------------------------------------------------------------------------------------------------------
# causal conv
# ------------------------------------------------------------------------------------------------------------------------------
CONV_DTYPES = [F32, BF16, F16]


@functools.lru_cache(maxsize=None)
def conv_data(width, dtype, l):
    g = torch.Generator().manual_seed(100 * width + l)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(3, 5, l).to(dtype).float(), dy=r(3, 5, l).to(dtype).float(), w=r(5, width) * 0.5, b=r(5) * 0.1)


@functools.lru_cache(maxsize=None)
def conv_ref(width, dtype, l, dim, has_bias, silu):
    d = conv_data(width, dtype, l)
    x, dy, w, b = d["x"][:, :dim].double(), d["dy"][:, :dim].double(), d["w"][:dim], (d["b"][:dim] if has_bias else None)
    y = O.causal_conv1d(x, w, b, silu, work_dtype=F64)
    dx, dw, db = O.causal_conv1d_bwd(x, w, b, dy, silu)
    return dict(y=y, dx=dx, dweight=dw, dbias=db)


def conv_case(ops, width, dtype, rev, l, dim, has_bias=True, silu=True, det=True, layout="inner", shift=0):
    d = conv_data(width, dtype, l)
    ref = conv_ref(width, dtype, l, dim, has_bias, silu)
    inst = f"w{width} {NAME[dtype]} {'rev' if rev else 'fwd'}"
    tag = f"L={l} dim={dim} bias={has_bias} silu={silu} ws={det} {layout} shift={shift}"
    x, dy = (dev(flip(d[k][:, :dim], rev).to(dtype).contiguous()) for k in ("x", "dy"))
    w, b = dev(d["w"][:dim].contiguous()), (dev(d["b"][:dim].contiguous()) if has_bias else None)
    g = torch.Generator().manual_seed(l + dim)
    prefill = dict(dweight=torch.randn(dim, width, generator=g))
    if has_bias:
        prefill["dbias"] = torch.randn(dim, generator=g)
    want = {k: prefill[k].double() + ref[k] for k in prefill}
    assert ops.DETERMINISTIC == det

    def inp(L, t):
        return L.flat(t, CK) if layout == "contig" else L.chan(t, shift=shift)

    def fwd(L):
        y = act_out(L, "y", (3, dim, l), dtype, layout, shift)
        assert ops.causal_conv1d_fwd(inp(L, x), L.vec(w), L.vec(b), silu, reverse=rev, bufs=dict(y=y)).data_ptr() == y.data_ptr()

    got = two_step("conv_fwd", fwd)
    within("conv_fwd", inst, "y", got["y"], flip(ref["y"], rev), CONV_FWD_TOL, tag=tag)

    def bwd(L):
        dx = L.out("dx", (3, dim, l), dtype, rows=CK, contiguous=True) if layout == "contig" else half_out(L, "dx", (3, dim, l), dtype, first=True)
        bufs = dict(dx=dx, **{k: L.out(k, v.shape, F32, fill=dev(v), rows=CK, contiguous=True) for k, v in prefill.items()})
        if det:
            bufs["workspace"] = L.scratch("workspace", 3 * dim * (width + 1), pad=64)
        r = ops.causal_conv1d_bwd(inp(L, x), L.vec(w), L.vec(b), inp(L, dy), silu, reverse=rev, bufs=bufs)
        assert r[0].data_ptr() == dx.data_ptr() and r[1].data_ptr() == bufs["dweight"].data_ptr() and (r[2] is None) == (not has_bias)

    def held(k, t, which):
        within("conv_bwd", inst, k, t, want[k], CONV_BWD_TOL, scaled=True, tag=f"{tag} {which}")

    got = two_step("conv_bwd", bwd, loose=() if det else tuple(prefill), held=held)
    dx = got["dx"] if layout == "contig" else got["dx"][:, :dim]
    if layout != "contig":
        assert not bool(got["dx"][:, dim:].any()), "dx: the other half of dxz was written"
    within("conv_bwd", inst, "dx", dx, flip(ref["dx"], rev), CONV_BWD_TOL, tag=tag)
    for k in prefill:
        held(k, got[k], "plain launch")


@pytest.mark.parametrize("rev", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("dtype", CONV_DTYPES, ids=[NAME[d] for d in CONV_DTYPES])
@pytest.mark.parametrize("width", [2, 3, 4])
def test_conv_instances(width, dtype, rev, monkeypatch):
    """Batch 3, dim 1 and 5, every L of the sweep (whole vectors: the forward's vector path; the rest, and L = 8 / 1024 off alignment,
    its element path; 1023 / 1024 / 1025 the backward's 1024-step block loop; L below the width in both directions)."""
    from mamba_asr_amd import ops
    for det in (True, False):
        monkeypatch.setattr(ops, "DETERMINISTIC", det)
        for l in CONV_L:
            conv_case(ops, width, dtype, rev, l, 5, det=det)
        conv_case(ops, width, dtype, rev, 9, 1, det=det)
        conv_case(ops, width, dtype, rev, 1024, 1, det=det, layout="contig")
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    for l in (8, 1024):
        conv_case(ops, width, dtype, rev, l, 5, shift=1)
    for has_bias, silu in ((False, True), (True, False), (False, False)):
        for l in (3, 8, 1025):
            conv_case(ops, width, dtype, rev, l, 5, has_bias=has_bias, silu=silu)
        conv_case(ops, width, dtype, rev, 1025, 5, has_bias=has_bias, silu=silu, layout="contig")


# ------------------------------------------------------------------------------------------------------------------------------
# refusals of badly placed buffers, and the table
# ------------------------------------------------------------------------------------------------------------------------------
def refused(run, match):
    """A launch the wrapper must refuse: RuntimeError, and neither an output nor a workspace touched."""
    L = G.Launch(True, DEV)
    with pytest.raises(RuntimeError, match=match):
        run(L)
    torch.cuda.synchronize()
    for name, (buf, view, outside) in L.g.items.items():
        G.assert_untouched(buf, outside, name)
        if name not in L.g.scratches:
            assert bool((view == G.sentinel_of(view.dtype)).all()), f"{name}: written by a refused launch"


def test_bufs_are_validated_before_any_launch(monkeypatch):
    from mamba_asr_amd import ops
    monkeypatch.setattr(ops, "DETERMINISTIC", True)
    b, d, l, n = 2, 5, 8, 16
    c = case_inputs(n, "f32", l, ALL)
    u, dl, z, dout = (dev(c[k][:b, :d].contiguous()) for k in ("u", "delta", "z", "dout"))
    A, B, C, D, bias = dev(c["A"][:d].contiguous()), dev(c["B"][:b]), dev(c["C"][:b]), dev(c["D"][:d].contiguous()), dev(c["bias"][:d].contiguous())
    x = torch.zeros(b, d, 1, 2 * n, device=DEV)
    good = lambda L, name, dt=F32: L.out(name, (b, d, l), dt, rows=CK, contiguous=True)

    def fwd(**bad):
        def run(L):
            bufs = dict(out_z=good(L, "out_z"), x=L.out("x", (b, d, 1, 2 * n), F32, rows=CK, contiguous=True))
            bufs.update({k: v(L) for k, v in bad.items()})
            ops.selective_scan_fwd(u, dl, A, B, C, D, z, bias, True, need_out="out" in bufs, bufs=bufs)
        return run
    refused(fwd(out_z=lambda L: good(L, "oz16", BF16)), "out_z_buf must be a time-contiguous")
    refused(fwd(out=lambda L: L.out("o6", (b, d + 1, l), F32, rows=CK, contiguous=True)), r"selective_scan_fwd: bufs\['out'\] must be a torch.float32 tensor of shape \(2, 5, 8\)")
    refused(fwd(out=lambda L: L.out("ot", (b, d, l), F32, transposed=True, rows=1)), "out and a strided out_z_buf cannot be requested together")
    refused(fwd(x=lambda L: L.out("x3", (b, d, 2, 2 * n), F32, rows=CK, contiguous=True)), r"selective_scan_fwd: bufs\['x'\] must be a contiguous torch.float32 tensor of shape \(2, 5, 1, 32\)")
    refused(fwd(h=lambda L: good(L, "h")), r"selective_scan_fwd: bufs has no \['h'\]")

    def run(L):
        ops.selective_scan_fwd(u, dl, A, B, C, D, None, bias, True, bufs=dict(out_z=good(L, "out_z")))
    refused(run, r"selective_scan_fwd: bufs\['out_z'\] places an output this call does not produce")

    def bwd(**bad):
        def run(L):
            bufs = dict(du=good(L, "du"), ddelta=good(L, "ddelta"), dz=good(L, "dz"), dA=L.out("dA", (d, n), F32, rows=CK, contiguous=True))
            bufs.update({k: v(L) for k, v in bad.items()})
            ops.selective_scan_bwd(u, dl, A, B, C, D, z, bias, dout, x, True, bufs=bufs)
        return run
    refused(bwd(du=lambda L: good(L, "du16", BF16)), "du_buf must be a time-contiguous")
    refused(bwd(dz=lambda L: L.out("dz6", (b, d + 1, l), F32, rows=CK, contiguous=True)), r"selective_scan_bwd: bufs\['dz'\] must be a time-contiguous")
    refused(bwd(dA=lambda L: L.out("dAt", (n, d), F32, rows=CK, contiguous=True)), r"selective_scan_bwd: bufs\['dA'\] must be a contiguous torch.float32 tensor of shape \(5, 16\)")
    refused(bwd(dB=lambda L: L.out("dB3", (b, n, l), F32, rows=CK, contiguous=True)), r"selective_scan_bwd: bufs\['dB'\] must be a contiguous torch.float32 tensor of shape \(2, 1, 16, 8\)")
    refused(bwd(dD=lambda L: L.out("dD16", (d,), BF16, rows=CK, contiguous=True)), r"selective_scan_bwd: bufs\['dD'\] must be a contiguous torch.float32")
    refused(bwd(workspace=lambda L: L.scratch("workspace", 16, pad=64)), r"selective_scan_bwd: bufs\['workspace'\] must be a contiguous torch.float32 tensor of shape \(\d+,\)")
    refused(bwd(out_z=lambda L: good(L, "out_z")), r"selective_scan_bwd: bufs\['out_z'\] places a buffer this call does not use")
    refused(bwd(dx=lambda L: good(L, "dx")), r"selective_scan_bwd: bufs has no \['dx'\]")
    w, cb = torch.ones(d, 4, device=DEV), torch.zeros(d, device=DEV)

    def conv_f(L):
        ops.causal_conv1d_fwd(u, w, cb, bufs=dict(y=L.out("y", (b, d, l + 1), F32, rows=CK, contiguous=True)))
    refused(conv_f, r"causal_conv1d_fwd: bufs\['y'\] must be a torch.float32 tensor of shape \(2, 5, 8\)")

    def conv_b(**bad):
        def run(L):
            bufs = dict(dx=good(L, "dx"))
            bufs.update({k: v(L) for k, v in bad.items()})
            ops.causal_conv1d_bwd(u, w, cb, dout, bufs=bufs)
        return run
    refused(conv_b(dx=lambda L: L.out("dxt", (b, l, d), F32, rows=CK, contiguous=True).transpose(1, 2)), r"causal_conv1d_bwd: bufs\['dx'\] must be .* with the time axis contiguous")
    refused(conv_b(dweight=lambda L: L.out("dw", (d, 3), F32, rows=CK, contiguous=True)), r"causal_conv1d_bwd: bufs\['dweight'\] must be a contiguous torch.float32 tensor of shape \(5, 4\)")
    refused(conv_b(workspace=lambda L: L.scratch("workspace", 16, pad=64)), r"causal_conv1d_bwd: bufs\['workspace'\] must be a contiguous torch.float32 tensor of shape \(50,\)")
    monkeypatch.setattr(ops, "DETERMINISTIC", False)
    refused(conv_b(workspace=lambda L: L.scratch("workspace", 50, pad=64)), r"causal_conv1d_bwd: bufs\['workspace'\] places a buffer this call does not use")


def test_bufs_none_is_the_old_call():
    """bufs=None: fresh outputs, zeroed parameter gradients, the bits of a placed launch."""
    from mamba_asr_amd import ops
    b, d, l, n = 2, 33, 72, 16
    c = case_inputs(n, "bf16", l, ALL)
    u, dl, z, dout = (dev(c[k][:b, :d].bfloat16().contiguous()) for k in ("u", "delta", "z", "dout"))
    A, B, C, D, bias = dev(c["A"][:d].contiguous()), dev(c["B"][:b].bfloat16()), dev(c["C"][:b].bfloat16()), dev(c["D"][:d].contiguous()), dev(c["bias"][:d].contiguous())
    out, x, out_z = ops.selective_scan_fwd(u, dl, A, B, C, D, z, bias, True)
    bufs = dict(out=torch.empty_like(u), out_z=torch.empty_like(u), x=torch.empty_like(x))
    ops.selective_scan_fwd(u, dl, A, B, C, D, z, bias, True, bufs=bufs)
    assert torch.equal(out, bufs["out"]) and torch.equal(out_z, bufs["out_z"]) and torch.equal(x, bufs["x"])
    r0 = ops.selective_scan_bwd(u, dl, A, B, C, D, z, bias, dout, x, True)
    zeros = dict(dA=torch.zeros(d, n, device=DEV), dB=torch.zeros(b, 1, n, l, device=DEV), dC=torch.zeros(b, 1, n, l, device=DEV))
    r1 = ops.selective_scan_bwd(u, dl, A, B, C, D, z, bias, dout, x, True, bufs=zeros)
    assert r0[8] is None and all(torch.equal(p, q) for p, q in zip(r0[:8], r1[:8]))
    w, cb = dev(torch.randn(d, 4)), dev(torch.randn(d))
    c0 = ops.causal_conv1d_bwd(u, w, cb, dout)
    c1 = ops.causal_conv1d_bwd(u, w, cb, dout, bufs=dict(dweight=torch.zeros(d, 4, device=DEV), dbias=torch.zeros(d, device=DEV)))
    assert all(torch.equal(p, q) for p, q in zip(c0, c1))
    assert torch.equal(ops.causal_conv1d_fwd(u, w, cb), ops.causal_conv1d_fwd(u, w, cb, bufs=dict(y=torch.empty_like(u))))


def test_zz_report():
    """Prints the worst error / bound per kernel, instance and result dtype (and per kernel and dtype), and the number of cases."""
    for (kernel, inst, dt), w in sorted(WORST.items()):
        print(f"worst {kernel:14s} {inst:34s} {dt:5s} {w:.3f}")
    top = {}
    for (kernel, inst, dt), w in WORST.items():
        top[(kernel, dt)] = max(top.get((kernel, dt), (0.0, "")), (w, inst))
    for (kernel, dt), (w, inst) in sorted(top.items()):
        print(f"summary {kernel:14s} {dt:5s} worst error / bound {w:.3f} ({inst})")
    print("two-launch cases:", ", ".join(f"{k} {v}" for k, v in sorted(CASES.items())))
    assert all(w <= 1.0 for w in WORST.values())
