"""Guard bands around the kernels of the training step's backward (tests/guard_bands.py; tests/test_guard_bands_cpu.py shows the checker
catches what it is for): cm_ffn_bwd_fused, cm_wgrad_bf16, cm_layernorm_fwd / _bwd, cm_dwconv_cl_fwd / _bwd, cm_bias_act_dropout_fwd / _bwd
(GLU form included), and the accumulate mode (overwrite = 0) of the five entry points that document one.

Every case is two launches through the wrappers' ``bufs`` keyword: (a) on ordinary tensors, (b) with every floating-point input a view
of a NaN-filled buffer, every output a view of a sentinel-filled one and every workspace NaN inside sentinels.  Then: (b)'s outputs have
(a)'s bits, nothing outside an output or a workspace is written, every output is finite, (a)'s outputs are far from the sentinel -- and
(a) is held to an fp64 reference computed on the CPU from the inputs as the kernel sees them (bf16 inputs rounded first; dropout
decisions from oracle.conmamba_oracle.drop_keep, never from a kernel).  The tolerances are those of the kernels' existing tests, named
at each use; every bias / gamma / tap gradient is also held PER COLUMN to the fp32 summation bound of what it sums.

Guards: 64 rows around the tensors of cm_ffn_bwd_fused and cm_wgrad_bf16 (their workgroup tile), 32 rows for LayerNorm, 16 rows for the
element-wise kernels, 32 time steps behind every utterance of the depthwise conv plus one whole guard utterance in front of and behind
the batch, 8 columns left and 16 right of column slices, at least one partial row around every workspace.  Packed weight images are
opaque to the tests and stay plain; the uint8 keep mask the element-wise backward reads is no floating-point input and stays plain.

The last test prints the worst error-to-bound ratio per kernel, dtype and tensor, and the number of two-launch cases.
"""
import functools
import itertools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import conmamba_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, F64, U8 = torch.bfloat16, torch.float32, torch.float64, torch.uint8
NAME = {BF16: "bf16", F32: "fp32"}
EPS24, EPS23 = 2.0 ** -24, 2.0 ** -23
WORST = {}                               # (kernel, dtype, tensor) -> worst error / bound
CASES = [0]                              # two-launch cases run so far


def two_step(run):
    CASES[0] += 1
    return G.two_step(run, DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def cpu64(t):
    return t.detach().double().cpu()


def close(a, b, rtol, atol, scaled=False):
    """assert_close in fp64; ``scaled``: atol x max(1, max|ref|) (tests/test_scan_rows_bwd.py, tests/test_dropout_stream.py)."""
    b = cpu64(b)
    torch.testing.assert_close(cpu64(a), b, rtol=rtol, atol=atol * (max(1.0, float(b.abs().max())) if scaled else 1.0))


def within(kernel, dt, name, got, ref64, bound, tag=""):
    """|got - ref| <= bound element by element; records the worst ratio."""
    err = (cpu64(got) - ref64).abs()
    assert err.shape == bound.shape, (kernel, name, err.shape, bound.shape)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    key = (kernel, NAME.get(dt, dt), name)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if worst > 1.0:
        at = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{kernel} {name} {tag}: error / bound {worst:.3f} at {at}: |err| {float(err[at]):.3e}, bound {float(bound[at]):.3e}, "
                             f"{int((ratio > 1).sum())} of {ratio.numel()} element(s) over")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu64_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def host_keep(seed, shape, p):
    """-> (keep (bool), scale) of the dropout stream's host restatement; p = 0: everything kept."""
    keep, sc = O.drop_keep(seed, shape, p)
    return torch.from_numpy(keep.copy()), sc


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


# ------------------------------------------------------------------------------------------------------------------------
# cm_ffn_bwd_fused
# ------------------------------------------------------------------------------------------------------------------------
D = 256


@functools.lru_cache(maxsize=None)
def _ffn_case(hidden):
    from mamba_asr_amd import ops
    g = gen(4000 + hidden)
    dout = torch.randn(130, D, generator=g)
    pre = torch.randn(130, hidden, generator=g).bfloat16()
    w1 = (torch.randn(hidden, D, generator=g) / 16).bfloat16()
    w2 = (torch.randn(D, hidden, generator=g) / hidden ** 0.5).bfloat16()
    return dict(dout=dout, pre=pre, w1=w1, w2=w2, w2t=ops.PackedWeight(dev(w2.t().contiguous())), w1t=ops.PackedWeight(dev(w1.t().contiguous())))


@pytest.mark.parametrize("p1,p2", [(0.0, 0.0), (0.1, 0.2)])
@pytest.mark.parametrize("hidden", [256, 512, 2048])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 130])
def test_ffn_bwd_fused(rows, hidden, p1, p2):
    """64 tokens per workgroup, 256-wide hidden slabs.  Guarded: da2, da1, act, dh, the [db1 | db2] buffer, the workspace (one partial
    row of hidden + 256 floats around it); poisoned: dout, pre.  Reference: the fp64 chain of
    test_ffn_bwd_fused_against_the_kernel_per_stage_chain (tests/test_scan_rows_bwd.py) on host masks, with its tolerances for da2 (4e-3,
    1e-5), da1 (3e-2, 1e-2), act (1e-2, 4e-3), dh (3e-2, 1.5e-2), atol x max(1, max|ref|); zero patterns exact against the host masks.
    Bias gradients per column against the fp64 column sum of the kernel's own stored da2 / da1.  Both sum the ROUNDED values in fp32
    (db2: the bf16 tile of phase 0; db1: csrc/ffn_bwd_fused.hip accumulates cs[] from the packed dv_ words, "the rounded values, as the
    GEMMs see them"), so both obey |err| <= rows x 2^-24 x sum|da| of the column, with no 2^-8 term.  rows = 1: each is that row."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    c = _ffn_case(hidden)
    dout, pre = c["dout"][:rows], c["pre"][:rows]
    s1, s2, alpha = 99 + rows, 77 + hidden, 0.5
    nws = int(N.lib().cm_ffn_bwd_workspace_floats(rows, hidden))

    def run(L):
        bufs = dict(da2=L.out("da2", (rows, D), BF16), da1=L.out("da1", (rows, hidden), BF16), act=L.out("act", (rows, hidden), BF16),
                    dh=L.out("dh", (rows, D), BF16), db1=L.out("db", (hidden + D,), F32), workspace=L.scratch("workspace", nws, pad=hidden + D))
        ret = ops.ffn_bwd_fused(L.rows(dev(dout)), c["w2t"], c["w1t"], L.rows(dev(pre)), alpha, p1, p2, s1, s2, bufs=bufs)
        assert ret[0].data_ptr() == bufs["da2"].data_ptr() and ret[4].data_ptr() == bufs["db1"].data_ptr()
        assert ret[5].data_ptr() == bufs["db1"][hidden:].data_ptr()
    outs = two_step(run)
    da2, da1, act, dh, db = (outs[k].cpu() for k in ("da2", "da1", "act", "dh", "db"))
    db1, db2 = db[:hidden], db[hidden:]
    k1, sc1 = host_keep(s1, (rows, hidden), p1)
    k2, sc2 = host_keep(s2, (rows, D), p2)
    m1, m2 = k1.double() * sc1, k2.double() * sc2
    x = pre.double()
    ref_da2 = alpha * dout.double() * m2
    close(da2, ref_da2, 4e-3, 1e-5, scaled=True)
    assert torch.equal(da2 == 0, ~k2), "da2's zeros are not the host mask's"
    ref_da1 = (da2.double() @ c["w2"].double()) * m1 * gelu64_grad(x)
    close(da1, ref_da1, 3e-2, 1e-2, scaled=True)
    assert torch.equal(da1 == 0, ~k1), "da1's zeros are not the host mask's"
    assert bool(((act == 0) | k1).all()), "act is not zero where the host dropped"
    close(act, gelu64(x) * m1, 1e-2, 4e-3, scaled=True)
    close(dh, ref_da1 @ c["w1"].double(), 3e-2, 1.5e-2, scaled=True)
    tag = f"rows {rows} hidden {hidden} p ({p1}, {p2})"
    within("cm_ffn_bwd_fused", BF16, "db2", db2, da2.double().sum(0), rows * EPS24 * da2.double().abs().sum(0), tag)
    within("cm_ffn_bwd_fused", BF16, "db1", db1, da1.double().sum(0), rows * EPS24 * da1.double().abs().sum(0), tag)
    if rows == 1:
        assert torch.equal(db2, da2[0].float()) and torch.equal(db1, da1[0].float()), "one row: each bias gradient is that row"


# ------------------------------------------------------------------------------------------------------------------------
# cm_wgrad_bf16
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _wgrad_case(m, n):
    g = gen(m * 7 + n)
    return torch.randn(257, m, generator=g).bfloat16(), torch.randn(257, n, generator=g).bfloat16()


@pytest.mark.parametrize("m,n", [(128, 128), (256, 128), (128, 384)])
@pytest.mark.parametrize("rows", [1, 31, 32, 33, 63, 64, 65, 127, 129, 257])
def test_wgrad_bf16(rows, m, n):
    """128 x 128 output tiles, K split over 64-row chunks; the ring kernel (variants 0, 2) steps 32 rows, the two-buffer kernels (1, 3)
    64.  Operands contiguous with 64 NaN rows around them, and as column slices of wider matrices: NaN columns on both sides, NaN rows
    behind -- rows at or past a chunk's end must come out of the buffer descriptors as zero, never out of memory.  Guarded: out, the
    workspace (one 128 x 128 partial tile around it).  Reference a^T b in fp64, per element:
        |err| <= (rows + ksplit) x 2^-23 x sum_k |a_ki| |b_kj|
    (products of bf16 values are exact in fp32; the MFMA's accumulation is not documented as round-to-nearest, hence 2^-23 per addition)."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    a, b = (t[:rows] for t in _wgrad_case(m, n))
    nws = int(N.lib().cm_wgrad_workspace_floats(rows, m, n))
    ksplit = nws // (m * n)
    if m == 128 and n == 128:
        assert ksplit == {1: 1, 31: 1, 32: 1, 33: 1, 63: 1, 64: 1, 65: 2, 127: 2, 129: 3, 257: 5}[rows]
    ref = a.double().t() @ b.double()
    bound = (rows + ksplit) * EPS23 * (a.double().abs().t() @ b.double().abs())
    for variant, sliced in itertools.product(range(4), (False, True)):
        def run(L):
            aa, bb = (L.cols(dev(t), rows=64) if sliced else L.rows(dev(t)) for t in (a, b))
            assert not (sliced and L.guard) or (aa.stride(0), bb.stride(0)) == (m + G.LEFT + G.RIGHT, n + G.LEFT + G.RIGHT)
            bufs = dict(out=L.out("out", (m, n), F32), workspace=L.scratch("workspace", nws, pad=128 * 128))
            assert ops.wgrad(aa, bb, variant=variant, bufs=bufs).data_ptr() == bufs["out"].data_ptr()
        outs = two_step(run)
        within(f"cm_wgrad_bf16 variant {variant}", BF16, "out", outs["out"], ref, bound, f"rows {rows} ({m}, {n}) {'slices' if sliced else 'contiguous'}")


def test_wgrad_refusals():
    """m = 64, n = 4224 and an operand stride that is no multiple of 8: refused by the entry point (code, no launch) and, with caller
    buffers, by the wrapper; out and the workspace untouched."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    import ctypes as ct
    z = lambda r, c: torch.zeros(r, c, dtype=BF16, device=DEV)
    odd = torch.zeros(32, 132, dtype=BF16, device=DEV)[:, :128]              # row stride 132: no multiple of 8
    for a, b in ((z(32, 64), z(32, 128)), (z(32, 128), z(32, 4224)), (odd, z(32, 128)), (z(32, 128), odd)):
        m, n = a.shape[1], b.shape[1]

        def run(L):
            out, ws = L.out("out", (m, n), F32), L.scratch("workspace", 4 * 128 * 128, pad=128 * 128)
            args = N.WgradArgs()
            args.rows, args.m, args.n, args.variant = 32, m, n, 0
            args.a, args.b, args.lda, args.ldb = a.data_ptr(), b.data_ptr(), a.stride(0), b.stride(0)
            args.out, args.workspace, args.workspace_floats, args.stream = out.data_ptr(), ws.data_ptr(), ws.numel(), None
            assert N.lib().cm_wgrad_bf16(ct.byref(args)) in (-2, -3), "the entry point launched"
            ops.wgrad(a, b, bufs=dict(out=out, workspace=ws))
        refused(run, "wgrad: bufs places the buffers of cm_wgrad_bf16")


def test_bufs_are_validated_before_any_launch():
    """A caller-supplied buffer of the wrong shape, dtype, layout or name is refused with a message that names it; nothing is written."""
    from mamba_asr_amd import ops
    x, w = torch.zeros(5, 16, device=DEV), torch.ones(16, device=DEV)
    stats = torch.zeros(2, 5, device=DEV)

    def ln_fwd(**bad):
        def run(L):
            bufs = dict(y=L.out("y", (5, 16), F32, rows=LN_ROWS), mean=L.out("stats", (2, 5), F32, rows=LN_ROWS))
            bufs.update({k: v(L) for k, v in bad.items()})
            ops.layernorm_fwd(x, w, w, 1e-5, bufs=bufs)
        return run
    refused(ln_fwd(y=lambda L: L.out("y6", (6, 16), F32, rows=LN_ROWS)), r"layernorm_fwd: bufs\['y'\] must be a contiguous torch.float32 tensor of shape \(5, 16\)")
    refused(ln_fwd(mean=lambda L: L.out("s16", (2, 5), BF16, rows=LN_ROWS)), r"layernorm_fwd: bufs\['mean'\] must be a contiguous torch.float32")
    refused(ln_fwd(y=lambda L: L.out("yt", (16, 5), F32, rows=LN_ROWS).t()), r"layernorm_fwd: bufs\['y'\] must be a contiguous")
    refused(ln_fwd(y=lambda L: torch.zeros(5, 16)), r"layernorm_fwd: bufs\['y'\] must be .* on cuda")
    refused(ln_fwd(rstd=lambda L: L.out("rstd", (5,), F32, rows=LN_ROWS)), r"layernorm_fwd: bufs has no \['rstd'\]")

    def ln_bwd(L):
        ops.layernorm_bwd(x, x, stats, w, 1e-5, bufs=dict(dgamma=L.out("dgb", (2, 16), F32, rows=LN_ROWS), workspace=L.scratch("workspace", 16, pad=64)))
    refused(ln_bwd, r"layernorm_bwd: bufs\['workspace'\] must be a contiguous torch.float32 tensor of shape \(16384,\)")

    def dw_bwd(L):
        x3 = torch.zeros(2, 5, 16, device=DEV)
        ops.dwconv_cl_bwd(x3, torch.ones(16, 3, device=DEV), x3, True, 1, bufs=dict(dx=L.out("dx", (2, 16, 5), F32, rows=G.TIME_TILE, contiguous=True).transpose(1, 2)))
    refused(dw_bwd, r"dwconv_cl_bwd: bufs\['dx'\] must be .* with the channel axis contiguous")

    def elem(L):
        ops.bias_act_dropout_fwd(x, None, p=0.1, seed=1, bufs=dict(mask=L.out("mask", (5, 16), F32, rows=EL_ROWS)))
    refused(elem, r"bias_act_dropout_fwd: bufs\['mask'\] must be a contiguous torch.uint8")


# ------------------------------------------------------------------------------------------------------------------------
# cm_layernorm_fwd / cm_layernorm_bwd
# ------------------------------------------------------------------------------------------------------------------------
LN_ROWS = 32                                                                  # guard rows: 8 waves x 4 rows of the narrow kernels
LN_EDGES = [(1, 8), (3, 144), (5, 256), (33, 260), (31, 640), (5, 1024), (3, 1028), (2, 4096)]
BRANCH = 2e-5          # |LN output| below which LeakyReLU's branch is not determined in fp32 (the forward's own bound is 1e-5 + 1e-5 |z|)


def _ln_ref(x, w, b, dy, slope, cm, mask_rows, dres):
    """fp64: y, dx (+ dres), dgamma, dbeta, and for dbeta's bound: |dy| where the epilogue lets the element through, and the gradient
    an element of undetermined LeakyReLU branch could add or lose."""
    rows, dim = x.shape
    xr, wr, br = (t.double().clone().requires_grad_(True) for t in (x, w, b))
    z = F.layer_norm(xr, (dim,), wr, br, 1e-5)
    y = z if slope is None else F.leaky_relu(z, slope)
    full = torch.ones(rows, dim, dtype=F64) if cm is None else cm.double().repeat_interleave(mask_rows, 0).repeat(1, dim // cm.shape[1])
    y = y * full
    dx, dg, db = torch.autograd.grad(y, [xr, wr, br], dy.double())
    if dres is not None:
        dx = dx + dres.double()
    through = dy.double().abs() * (full != 0)
    unsure = torch.zeros(dim, dtype=F64) if slope is None else ((z.detach().abs() < BRANCH) * (dy.double() * full).abs() * (1 - slope)).sum(0)
    return y.detach(), dx, dg, db, through.sum(0), unsure


def _ln_case(rows, dim, xdt, ydt, seed, epilogue=None):
    g = gen(seed)
    x = (torch.randn(rows, dim, generator=g) * 2.0 + 0.5).to(xdt)
    w, b = torch.randn(dim, generator=g) * 0.5 + 1.0, torch.randn(dim, generator=g) * 0.2
    dy = torch.randn(rows, dim, generator=g).to(ydt)
    dres = torch.randn(rows, dim, generator=g)
    slope, cm, mask_rows = None, None, 1
    if epilogue is not None:
        mask_rows, mask_c = epilogue
        slope = 0.01
        cm = (torch.rand(rows // mask_rows, mask_c, generator=g) > 0.3).float() / 0.7
    return x, w, b, dy, dres, slope, cm, mask_rows


def _ln_fwd_bwd(rows, dim, xdt, ydt, seed, directions=("fwd", "bwd"), need_dx=True, with_dres=False, epilogue=None):
    """The forward and / or the backward of one shape through two_step, against fp64.  Tolerances (tests/test_hip_ops.py):
    test_layernorm_forward_backward's -- y (1e-5, 1e-5) in fp32, (1.6e-2, 1e-2) in bf16; dx (1e-4, 1e-4) where x is fp32, (1.6e-2, 1e-2)
    where dx is rounded to bf16; dgamma (1e-4, 1e-4 x max(1, max|ref|)) -- and with the epilogue test_layernorm_leaky_dropout2d_epilogue's:
    (1e-4, 1e-4) / (3e-2, 3e-2), gradients' atol x max(1, max|ref|).  Statistics: mean (1e-5, 1e-5), 1/std (1e-4, 1e-5) as the forward
    guard file holds cm_ffn_fused's.  dbeta per column: rows x 2^-24 x sum|dy| over the rows the epilogue lets through, plus what the
    elements whose LeakyReLU branch fp32 cannot determine (|LN(x)| < 2e-5) would change."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    x, w, b, dy, dres, slope, cm, mask_rows = _ln_case(rows, dim, xdt, ydt, seed, epilogue)
    dres = dres if with_dres else None
    ry, rdx, rdg, rdb, through, unsure = _ln_ref(x, w, b, dy, slope, cm, mask_rows, dres)
    ekw = lambda L: dict(leaky_slope=slope, chan_mask=None if cm is None else L.rows(dev(cm), rows=4), mask_rows=mask_rows)
    tag = f"({rows}, {dim}) x {NAME[xdt]} y {NAME[ydt]}"
    kernel = "cm_layernorm" + (" + epilogue" if epilogue else "")

    def fwd(L):
        bufs = dict(y=L.out("y", (rows, dim), ydt, rows=LN_ROWS), mean=L.out("stats", (2, rows), F32, rows=LN_ROWS))
        y, x2, stats = ops.layernorm_fwd(L.rows(dev(x), rows=LN_ROWS), L.vec(dev(w)), L.vec(dev(b)), 1e-5, ydt, bufs=bufs, **ekw(L))
        assert y.data_ptr() == bufs["y"].data_ptr() and stats.data_ptr() == bufs["mean"].data_ptr()
    outs = two_step(fwd)
    stats = outs["stats"]
    if "fwd" in directions:
        yt = ((1e-5, 1e-5) if ydt == F32 else (1.6e-2, 1e-2)) if epilogue is None else ((1e-4, 1e-4) if ydt == F32 else (3e-2, 3e-2))
        close(outs["y"], ry, *yt)
        x64 = x.double()
        close(stats[0], x64.mean(1), 1e-5, 1e-5)
        close(stats[1], (x64.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4, 1e-5)
    if "bwd" not in directions:
        return
    nws = int(N.lib().cm_layernorm_bwd_workspace_floats(rows, dim))

    def bwd(L):
        bufs = dict(dgamma=L.out("dgb", (2, dim), F32, rows=LN_ROWS), workspace=L.scratch("workspace", nws, pad=4 * dim))
        if need_dx:
            bufs["dx"] = L.out("dx", (rows, dim), xdt, rows=LN_ROWS)
        dx, dg, db = ops.layernorm_bwd(L.rows(dev(dy), rows=LN_ROWS), L.rows(dev(x), rows=LN_ROWS), L.rows(stats, rows=LN_ROWS), L.vec(dev(w)), 1e-5,
                                       need_dx=need_dx, dres=L.rows(dev(dres), rows=LN_ROWS), bias=L.vec(dev(b)), bufs=bufs, **ekw(L))
        assert (dx is None) == (not need_dx) and dg.data_ptr() == bufs["dgamma"].data_ptr() and db.data_ptr() == bufs["dgamma"][1].data_ptr()
        assert dx is None or dx.data_ptr() == bufs["dx"].data_ptr()
    outs = two_step(bwd)
    gt = (1e-4, 1e-4) if xdt == F32 else (1.6e-2, 1e-2)
    if epilogue is not None:
        gt = (1e-4, 1e-4) if (xdt, ydt) == (F32, F32) else (3e-2, 3e-2)
    scale = lambda t: max(1.0, float(t.abs().max()))
    if need_dx:
        close(outs["dx"], rdx, gt[0], gt[1] * (scale(rdx) if epilogue is not None else 1.0))
    et = 1e-4 if (epilogue is None or (xdt, ydt) == (F32, F32)) else 3e-2
    close(outs["dgb"][0], rdg, et, et * scale(rdg))
    within(kernel, ydt, "dbeta", outs["dgb"][1], rdb, rows * EPS24 * through + unsure, tag)


@pytest.mark.parametrize("xdt,ydt", [(F32, F32), (BF16, F32), (F32, BF16), (BF16, BF16)], ids=["f32-f32", "bf16-f32", "f32-bf16", "bf16-bf16"])
@pytest.mark.parametrize("rows,dim", LN_EDGES)
def test_layernorm_edges(rows, dim, xdt, ydt):
    """Shapes that do not loop, the four x / y dtype instances: 16 lanes per row up to dim 256, one wave per row up to 1024, one
    workgroup per row above; rows that are no multiple of the rows per wave / workgroup.  Guarded: y, the (2, rows) statistics, dx, the
    (2, dim) gradients, the workspace; poisoned: x, dy, gamma, beta, the statistics as inputs of the backward."""
    _ln_fwd_bwd(rows, dim, xdt, ydt, 7 * rows + dim)


@pytest.mark.parametrize("direction,rows,dim", [("bwd", 8195, 8), ("bwd", 2051, 260), ("bwd", 515, 1028),
                                                ("fwd", 65540, 8), ("fwd", 8195, 260), ("fwd", 2051, 1028)])
def test_layernorm_grid_stride_second_round(direction, rows, dim):
    """Row counts just above what one round of the grid covers (backward: 256 workgroups x 32 rows, 512 x 4, 512 x 1; forward: 2048
    workgroups x 32, x 4, x 1): the last rows are a second trip through the loop, with the prefetch of the backward across it."""
    for xdt, ydt in ((F32, F32), (BF16, BF16)):
        _ln_fwd_bwd(rows, dim, xdt, ydt, rows + dim, directions=(direction,))


@pytest.mark.parametrize("rows,dim", [(3, 144), (33, 260), (5, 1024), (3, 1028)])
def test_layernorm_options(rows, dim):
    """need_dx=False (no dx, the gradients unchanged) and dres (fp32, dim <= 1024: added to dx in the same pass)."""
    for xdt, ydt in ((F32, F32), (BF16, BF16)):
        _ln_fwd_bwd(rows, dim, xdt, ydt, 11 * rows + dim, directions=("bwd",), need_dx=False)
    if dim <= 1024:
        for ydt in (F32, BF16):
            _ln_fwd_bwd(rows, dim, F32, ydt, 13 * rows + dim, directions=("bwd",), with_dres=True)


@pytest.mark.parametrize("rows,dim,mask_rows,mask_c", [(33, 144, 3, 16), (33, 260, 11, 20), (9, 1028, 3, 4), (35, 8, 7, 8)])
def test_layernorm_leaky_channel_mask_epilogue(rows, dim, mask_rows, mask_c):
    """y = LeakyReLU(LN(x)) x chan_mask[row / mask_rows][col % mask_c], forward and backward; mask_rows is no multiple of the rows of a
    wave, so the last mask group ends inside one.  chan_mask and beta (the backward recomputes LN's output) are poisoned too."""
    for xdt, ydt in ((F32, F32), (BF16, BF16), (BF16, F32)):
        _ln_fwd_bwd(rows, dim, xdt, ydt, 17 * rows + dim, epilogue=(mask_rows, mask_c))


# ------------------------------------------------------------------------------------------------------------------------
# cm_dwconv_cl_fwd / cm_dwconv_cl_bwd
# ------------------------------------------------------------------------------------------------------------------------
DW_TAPS = [(1, 0), (2, 0), (2, 1), (31, 15), (31, 30), (32, 16), (32, 31), (32, 0)]
DW_BATCH = 3


@functools.lru_cache(maxsize=None)
def _dw_data(l, dim, dtype):
    g = gen(100 * l + dim)
    return torch.randn(DW_BATCH, l, dim, generator=g).to(dtype), torch.randn(DW_BATCH, l, dim, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _dw_taps(dim, k):
    g = gen(dim + k)
    return torch.randn(dim, k, generator=g) / k ** 0.5, torch.randn(dim, generator=g) * 0.1


def _dwconv(l, dim, k, pad_left, dtype, left=G.LEFT, align=16):
    """One (seqlen, dim, taps, dtype) through two_step, forward and backward.  Reference: torch conv1d + autograd in fp64 on the explicitly
    padded rows (pad_left zeros in front, k - 1 - pad_left behind: seqlen outputs, what test_dwconv_channels_last_forward_backward cuts
    its output to).  Tolerances: that test's -- y (1e-5, 1e-5) / (1.6e-2, 1e-2), dx (1e-4, 1e-4) / (2e-2, 2e-2) -- and per channel
    dbias: n x 2^-24 x sum|dy|, per (channel, tap) dweight: (n + 1) x 2^-24 x sum|dy x|, n = batch x seqlen."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    x, dy = _dw_data(l, dim, dtype)
    w, bias = _dw_taps(dim, k)
    nws = int(N.lib().cm_dwconv_cl_workspace_floats(DW_BATCH, l, dim))
    geo = dict(rows=G.TIME_TILE, left=left, right=G.RIGHT, align=align)

    def rows3(L, t=None, name=None):
        """An input (t) or output (name) in the launch's geometry.  The launcher picks the kernel by alignment, so the plain launch of a
        misaligned case is the same column slice of an ordinary wider tensor: both launches take the same route and sum in the same order."""
        if L.guard or left == G.LEFT:
            return L.cols(t, **geo) if name is None else L.out(name, (DW_BATCH, l, dim), dtype, **geo)
        v = torch.zeros(DW_BATCH, l, left + dim + G.RIGHT, dtype=dtype, device=DEV)[:, :, left:left + dim]
        if name is None:
            v.copy_(t)
        else:
            L.outs[name] = v
        return v

    def fwd(L):
        y = rows3(L, name="y")
        assert ops.dwconv_cl_fwd(rows3(L, dev(x)), L.vec(dev(w)), L.vec(dev(bias)), pad_left, bufs=dict(y=y)).data_ptr() == y.data_ptr()

    def bwd(L):
        bufs = dict(dx=rows3(L, name="dx"), dweight=L.out("dweight", (dim, k), F32, rows=G.TIME_TILE),
                    dbias=L.out("dbias", (dim,), F32, rows=G.TIME_TILE), partial=L.scratch("partial", nws, pad=dim * 33 * 4))
        dx, dw, db = ops.dwconv_cl_bwd(rows3(L, dev(x)), L.vec(dev(w)), rows3(L, dev(dy)), True, pad_left, bufs=bufs)
        assert (dx.data_ptr(), dw.data_ptr(), db.data_ptr()) == tuple(bufs[n].data_ptr() for n in ("dx", "dweight", "dbias"))
    fo, bo = two_step(fwd), two_step(bwd)
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), bias.double().requires_grad_(True)
    xp = F.pad(xr.transpose(1, 2), (pad_left, k - 1 - pad_left))
    ref = F.conv1d(xp, wr[:, None, :], br, groups=dim).transpose(1, 2)
    assert ref.shape == x.shape
    rdx, rdw, rdb = torch.autograd.grad(ref, [xr, wr, br], dy.double())
    ft, gt = ((1e-5, 1e-5), (1e-4, 1e-4)) if dtype == F32 else ((1.6e-2, 1e-2), (2e-2, 2e-2))
    close(fo["y"], ref, *ft)
    close(bo["dx"], rdx, *gt)
    n = DW_BATCH * l
    tag = f"L {l} dim {dim} k {k} pad_left {pad_left} left {left}"
    kernel = "cm_dwconv_cl_bwd" + ("" if left == G.LEFT and dim % 8 == 0 else " (untiled)")
    within(kernel, dtype, "dbias", bo["dbias"], rdb, n * EPS24 * dy.double().abs().sum((0, 1)), tag)
    win = xp.detach().unfold(2, k, 1)                                         # (batch, dim, seqlen, k): x[t + j - pad_left]
    absdw = (dy.double().transpose(1, 2)[..., None] * win).abs().sum((0, 2))
    within(kernel, dtype, "dweight", bo["dweight"], rdw, (n + 1) * EPS24 * absdw, tag)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("l", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_dwconv_cl_tiled(l, dtype):
    """The tiled kernels (32-step tiles, 256-channel blocks; the backward walks two tiles per workgroup): every tap shape x dim 8, 48,
    256, 264 at batch 3.  x and dy are (batch, seqlen, dim) views with 32 NaN steps behind every utterance, NaN utterances around the
    batch and NaN columns beside every row: a halo that comes from memory instead of being zero shows.  Guarded: y, dx (the same
    geometry), dweight, dbias, partial (four partial rows around it)."""
    for (k, pad_left), dim in itertools.product(DW_TAPS, (8, 48, 256, 264)):
        _dwconv(l, dim, k, pad_left, dtype)


@pytest.mark.parametrize("l", [1, 2, 31, 32, 33, 63, 64, 65, 97])
def test_dwconv_cl_untiled(l):
    """The plain kernels (64-step runs), reached both ways: dim 12 in bf16 (no multiple of the 8-element vector), and a bf16 view with 4
    guard columns on the left (8-byte aligned only)."""
    for k, pad_left in DW_TAPS:
        _dwconv(l, 12, k, pad_left, BF16, align=8)
        _dwconv(l, 48, k, pad_left, BF16, left=4, align=8)


# ------------------------------------------------------------------------------------------------------------------------
# cm_bias_act_dropout_fwd / cm_bias_act_dropout_bwd, GLU form included
# ------------------------------------------------------------------------------------------------------------------------
EL_ROWS = 16                                                                  # rows per workgroup of the backward


def _colsum_bound(kernel, dt, name, dbias, da, rows, tag):
    """dbias against the fp64 column sums of the kernel's own STORED da (what it sums, in fp32): rows x 2^-24 x sum|da| per column."""
    da = cpu64(da)
    within(kernel, dt, name, dbias, da.sum(0), rows * EPS24 * da.abs().sum(0), tag)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", [8, 136, 256, 1024, 2048])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33])
def test_bias_act_dropout(rows, dim, dtype):
    """16 rows per workgroup of the backward, 8 elements per thread; dim 136 leaves a workgroup's last thread idle, 2048 is one row per
    pass.  Forward: act none / GELU x {no dropout, stored mask, seed only} and the residual form; backward: act x {stored mask, seed
    only} x {dy in the I/O dtype, dy fp32 under bf16} x want_act (bf16 GELU) and want_dbias=False.  Guarded: y, the uint8 mask (integer
    sentinel), da, act_out, dbias, the workspace; poisoned: a, bias, res, dy.  Reference and tolerances: tests/test_dropout_stream.py's
    -- the stored mask IS the host mask, zero patterns exact, y (1e-5, 1e-5) / (8e-3, 1e-3), da (1e-4, 1e-5) / (8e-3, 5e-4), atol x
    max(1, max|ref|); act_out (1e-2, 4e-3) as tests/test_scan_rows_bwd.py -- and dbias per column (_colsum_bound)."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    g = gen(rows * 31 + dim + (dtype == BF16))
    a = torch.randn(rows, dim, generator=g).to(dtype)
    bias = 0.1 * torch.randn(dim, generator=g)
    res = torch.randn(rows, dim, generator=g)
    dy32 = torch.randn(rows, dim, generator=g)
    p, alpha, seed = 0.1, 0.5, 0x5EED_0000 + rows * 4099 + dim
    keep, sc = host_keep(seed, (rows, dim), p)
    ones = torch.ones(rows, dim, dtype=torch.bool)
    nws = int(N.lib().cm_bias_act_dropout_bwd_workspace_floats(rows, dim))
    rows_in = lambda L, t: L.rows(dev(t), rows=EL_ROWS)
    tag = f"({rows}, {dim}) {NAME[dtype]}"
    # forward
    for act, (drop, store), with_res in itertools.product((0, 1), ((False, False), (True, True), (True, False)), (False, True)):
        ydt = F32 if with_res else dtype

        def fwd(L):
            bufs = dict(y=L.out("y", (rows, dim), ydt, rows=EL_ROWS))
            if drop and store:
                bufs["mask"] = L.out("mask", (rows, dim), U8, rows=EL_ROWS)
            y, m = ops.bias_act_dropout_fwd(rows_in(L, a), L.vec(dev(bias)), act=act, p=p if drop else 0.0, res=rows_in(L, res) if with_res else None,
                                            alpha=alpha, seed=seed, store_mask=store, bufs=bufs)
            assert y.data_ptr() == bufs["y"].data_ptr() and (m is None) == (not (drop and store))
        outs = two_step(fwd)
        kp, s = (keep, sc) if drop else (ones, 1.0)
        if drop and store:
            assert torch.equal(outs["mask"].cpu(), kp.to(U8)), f"{tag}: the stored mask is not the host mask"
        t = a.double() + bias.double()
        d = (gelu64(t) if act else t) * kp.double() * s
        y = cpu64(outs["y"])
        if with_res:
            assert torch.equal(y[~kp], res.double()[~kp]), f"{tag}: a dropped element changed the stream"
        elif drop:
            assert torch.equal(y == 0, ~kp), f"{tag}: y's zeros are not the host mask's"
        close(y, res.double() + alpha * d if with_res else d, *((1e-5, 1e-5) if dtype == F32 else (8e-3, 1e-3)), scaled=True)
    # backward
    forms = [(act, form, dyf, False, True) for act in (0, 1) for form in ("none", "mask", "seed") for dyf in ((False, True) if dtype == BF16 else (False,))]
    forms += [(1, "seed", False, True, True)] if dtype == BF16 else []
    forms += [(1, "mask", False, False, False)]
    for act, form, dy_f32, want_act, want_dbias in forms:
        dy = dy32 if (dy_f32 or dtype == F32) else dy32.to(BF16)
        kp, s = (keep, sc) if form != "none" else (ones, 1.0)

        def bwd(L):
            bufs = dict(da=L.out("da", (rows, dim), dtype, rows=EL_ROWS))
            if want_act:
                bufs["act_out"] = L.out("act_out", (rows, dim), dtype, rows=EL_ROWS)
            if want_dbias:
                bufs.update(dbias=L.out("dbias", (dim,), F32, rows=EL_ROWS), dbias_part=L.scratch("workspace", nws, pad=4 * dim))
            ret = ops.bias_act_dropout_bwd(rows_in(L, dy), dev(kp.to(U8)) if form == "mask" else None, p if form != "none" else 0.0,
                                           a=rows_in(L, a) if act else None, bias=L.vec(dev(bias)) if act else None, act=act, alpha=alpha,
                                           out_dtype=dtype, want_dbias=want_dbias, seed=seed if form == "seed" else None, want_act=want_act, bufs=bufs)
            assert ret[0].data_ptr() == bufs["da"].data_ptr() and (ret[1] is None) == (not want_dbias)
        outs = two_step(bwd)
        da = cpu64(outs["da"])
        t = a.double() + bias.double()
        assert torch.equal(da == 0, ~kp), f"{tag}: da's zeros are not the host mask's"
        close(da, alpha * dy.double() * kp.double() * s * (gelu64_grad(t) if act else 1.0), *((1e-4, 1e-5) if dtype == F32 else (8e-3, 5e-4)), scaled=True)
        if want_act:
            close(outs["act_out"], gelu64(t) * kp.double() * s, 1e-2, 4e-3, scaled=True)
            assert bool(((outs["act_out"].cpu() == 0) | kp).all())
        if want_dbias:
            _colsum_bound("cm_bias_act_dropout_bwd", dtype, "dbias", outs["dbias"], outs["da"], rows, tag)
            if rows == 1:
                assert torch.equal(outs["dbias"].cpu(), outs["da"][0].float().cpu())


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dim", [8, 136, 256, 1024])
@pytest.mark.parametrize("rows", [1, 15, 16, 17, 33])
def test_bias_glu(rows, dim, dtype):
    """The GLU form (a and da (rows, 2 dim), dbias (2 dim), up to dim 1024).  Reference and bounds: test_bias_glu_fwd_bwd_vs_fp64
    (tests/test_row_kernels_fp64.py): fp32 results rtol 2e-3, atol 2e-4 x max(1, max|ref|); bf16 results against the fp64 result
    rounded to bf16, rtol 2e-2; dbias per column against the fp64 da:
        rows 2^-24 sum|da| + 8 x 2^-24 sum_rows |dy| (value half) or |dy v| (gate half) (+ 2^-8 sum|da| in bf16)
    as that file's docstring derives it -- and against the kernel's own stored da with the summation term alone."""
    from mamba_asr_amd import ops
    import mamba_asr_amd._native as N
    g = gen(rows * 3 + dim + (dtype == BF16))
    bias = torch.cat([torch.randn(dim, generator=g) * 2.0, torch.randn(dim, generator=g) * 0.5])
    a = torch.cat([torch.randn(rows, dim, generator=g) * 4.0, torch.randn(rows, dim, generator=g)], dim=1).to(dtype)
    dy = (torch.randn(rows, dim, generator=g) * 1.5).to(dtype)
    nws = int(N.lib().cm_bias_act_dropout_bwd_workspace_floats(rows, dim))
    rows_in = lambda L, t: L.rows(dev(t), rows=EL_ROWS)
    tag = f"({rows}, {dim}) {NAME[dtype]}"

    def fwd(L):
        y = L.out("y", (rows, dim), dtype, rows=EL_ROWS)
        assert ops.bias_glu_fwd(rows_in(L, a), L.vec(dev(bias)), bufs=dict(y=y)).data_ptr() == y.data_ptr()

    def bwd(L):
        bufs = dict(da=L.out("da", (rows, 2 * dim), dtype, rows=EL_ROWS), dbias=L.out("dbias", (2 * dim,), F32, rows=EL_ROWS),
                    dbias_part=L.scratch("workspace", nws, pad=4 * dim))
        da, db = ops.bias_glu_bwd(rows_in(L, dy), rows_in(L, a), L.vec(dev(bias)), bufs=bufs)
        assert da.data_ptr() == bufs["da"].data_ptr() and db.data_ptr() == bufs["dbias"].data_ptr()
    fo, bo = two_step(fwd), two_step(bwd)
    a64, dy64, b64 = a.double(), dy.double(), bias.double()
    v, sg = a64[:, :dim] + b64[:dim], torch.sigmoid(a64[:, dim:] + b64[dim:])
    ry, rda = v * sg, torch.cat([dy64 * sg, dy64 * v * sg * (1 - sg)], dim=1)
    for got, ref in ((fo["y"], ry), (bo["da"], rda)):
        want = (ref.to(BF16) if dtype == BF16 else ref).double()
        torch.testing.assert_close(cpu64(got), want, rtol=2e-2 if dtype == BF16 else 2e-3, atol=2e-4 * max(1.0, float(want.abs().max())))
    sumabs = rda.abs().sum(0)
    bound = rows * EPS24 * sumabs + (2.0 ** -8 * sumabs if dtype == BF16 else 0.0) + 8 * EPS24 * torch.cat([dy64.abs().sum(0), (dy64 * v).abs().sum(0)])
    within("cm_bias_act_dropout_bwd (GLU)", dtype, "dbias vs fp64 da", bo["dbias"], rda.sum(0), bound, tag)
    _colsum_bound("cm_bias_act_dropout_bwd (GLU)", dtype, "dbias vs stored da", bo["dbias"], bo["da"], rows, tag)


# ------------------------------------------------------------------------------------------------------------------------
# accumulate mode (overwrite = 0)
# ------------------------------------------------------------------------------------------------------------------------
class _Twice:
    """ops._launch patched for the calls of ``entry``: the launch as given (overwrite = 1), then the same struct with overwrite = 0."""

    def __init__(self, monkeypatch, entry):
        from mamba_asr_amd import ops
        self.ops, self.mp, self.entry, self.calls = ops, monkeypatch, entry, 0

    def __enter__(self):
        orig = self.ops._launch

        def hook(name, fn, args, units=0):
            orig(name, fn, args, units)
            if name == self.entry:
                assert args.overwrite == 1, "the wrapper did not ask for overwrite"
                args.overwrite = 0
                orig(name, fn, args, units)
                self.calls += 1
        self.ctx = self.mp.context()
        self.ctx.__enter__().setattr(self.ops, "_launch", hook)
        return self

    def __exit__(self, *exc):
        self.ctx.__exit__(*exc)
        torch.cuda.synchronize()
        assert exc[0] is not None or self.calls == 1, f"{self.entry}: {self.calls} launches seen"


def _doubled(plain, twice, params, data, what):
    for k in params:
        if plain[k] is not None:
            assert torch.equal(twice[k], plain[k] + plain[k]), f"{what}: {k} is not twice the plain call's after an accumulating second launch"
    for k in data:
        if plain[k] is not None:
            assert torch.equal(twice[k], plain[k]), f"{what}: {k} changed its bits"


@pytest.mark.parametrize("l", [17, 33])
def test_accumulate_scan_cl_bwd(l, monkeypatch):
    """cm_scan_cl_bwd, both directions in one launch: dA / ddt_weight / dD / ddelta_bias accumulate, du / dz / dxdbl keep their bits."""
    import test_scan_rows_bwd_edges as E
    from mamba_asr_amd import ops
    case = E.make_case(2, l, 72, 16, F32, 5100 + l)
    dirs, gz = E.forward(ops, case)
    plain = ops.scan_cl_bwd(dirs, gz)
    with _Twice(monkeypatch, "cm_scan_cl_bwd"):
        twice = ops.scan_cl_bwd(dirs, gz)
    for i, (o, o2) in enumerate(zip(plain, twice)):
        assert float(o["dA"].abs().max()) > 0 or l == 1
        _doubled(o, o2, ("dA", "ddt_weight", "dD", "ddelta_bias"), ("du", "dz", "dxdbl"), f"scan_cl_bwd direction {i}")


@pytest.mark.parametrize("l", [17, 33])
def test_accumulate_conv_cl_bwd(l, monkeypatch):
    """cm_conv_cl_bwd, both directions: the four parameter gradients accumulate, dx / dz keep their bits."""
    from mamba_asr_amd import ops
    g = gen(5200 + l)
    e = 72
    t = lambda *s: dev(torch.randn(*s, generator=g))
    x, duf, dub, dzf, dzb = (t(2, l, e) for _ in range(5))
    w, bs = [t(e, 4) * 0.5 for _ in range(2)], [t(e) * 0.2 for _ in range(2)]
    call = lambda: dict(zip(("dx", "dz", "dwf", "dbf", "dwb", "dbb"), ops.conv_cl_bwd(x, w[0], bs[0], duf, w[1], bs[1], dub, dz_f=dzf, dz_b=dzb)))
    plain = call()
    with _Twice(monkeypatch, "cm_conv_cl_bwd"):
        twice = call()
    _doubled(plain, twice, ("dwf", "dbf", "dwb", "dbb"), ("dx", "dz"), "conv_cl_bwd")


@pytest.mark.parametrize("l,dim,dtype", [(33, 48, BF16), (17, 12, F32)])
def test_accumulate_dwconv_cl_bwd(l, dim, dtype, monkeypatch):
    """cm_dwconv_cl_bwd, the tiled and the plain kernel's reduce: dweight / dbias accumulate, dx keeps its bits."""
    from mamba_asr_amd import ops
    g = gen(5300 + l)
    x, dy = (dev(torch.randn(2, l, dim, generator=g).to(dtype)) for _ in range(2))
    w = dev(torch.randn(dim, 31, generator=g) / 31 ** 0.5)
    call = lambda: dict(zip(("dx", "dweight", "dbias"), ops.dwconv_cl_bwd(x, w, dy, True, 15)))
    plain = call()
    with _Twice(monkeypatch, "cm_dwconv_cl_bwd"):
        twice = call()
    _doubled(plain, twice, ("dweight", "dbias"), ("dx",), "dwconv_cl_bwd")


@pytest.mark.parametrize("glu", [False, True], ids=["plain", "glu"])
def test_accumulate_bias_act_dropout_bwd(glu, monkeypatch):
    """cm_bias_act_dropout_bwd, plain (GELU, seed-only dropout) and GLU: dbias accumulates, da keeps its bits."""
    from mamba_asr_amd import ops
    g = gen(5400 + glu)
    rows, dim = 33, 136
    dy = dev(torch.randn(rows, dim, generator=g))
    a, bias = dev(torch.randn(rows, (2 if glu else 1) * dim, generator=g)), dev(0.1 * torch.randn((2 if glu else 1) * dim, generator=g))
    if glu:
        call = lambda: dict(zip(("da", "dbias"), ops.bias_glu_bwd(dy, a, bias)))
    else:
        call = lambda: dict(zip(("da", "dbias"), ops.bias_act_dropout_bwd(dy, None, 0.1, a=a, bias=bias, act=1, alpha=0.5, seed=4242)))
    plain = call()
    with _Twice(monkeypatch, "cm_bias_act_dropout_bwd"):
        twice = call()
    _doubled(plain, twice, ("dbias",), ("da",), "bias_act_dropout_bwd" + (" (GLU)" if glu else ""))


# ------------------------------------------------------------------------------------------------------------------------
def test_report_worst_ratios_and_case_count():
    """Prints what the tests above recorded (run the file with -s): the worst error / bound per kernel, dtype and tensor."""
    print()
    for (kernel, dt, name), r in sorted(WORST.items()):
        print(f"worst error / bound  {kernel:36s} [{dt}] {name:20s} {r:.3f}")
    print(f"two-launch guard-band cases in this file: {CASES[0]}")
    assert all(r <= 1.0 for r in WORST.values())
