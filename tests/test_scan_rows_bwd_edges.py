"""cm_scan_cl_bwd / cm_conv_cl_bwd (and the checkpoints / ypre cm_scan_cl_fwd writes for them) at the edges the comfortable
shapes of tests/test_scan_rows_bwd.py leave out: sequences shorter than a 16-step block or an 8-step half block and lengths on /
next to their boundaries, extreme time steps, every option of the wrappers, strided views with poisoned surroundings, conv
sequences shorter than the window, and the mixer node at decoder lengths.

Reference: the fp64 oracle on the CPU (oracle.selective_scan_bwd / causal_conv1d_bwd / bimamba_v2 / mamba_uni; reverse time
through flipped tensors, the dt_proj part as fp64 einsums; bf16 I/O: on the bf16-rounded inputs and the bf16-rounded W_dt).

Comparison: per channel.  tests/test_scan_rows_bwd.py's close() scales atol by the tensor's global max |ref|; with extreme time
steps dA spans 1e5 .. 1e-18 between channels, so one wrong 64-channel group would pass.  chan_check() scales by the channel's
own max |ref| (floor 1e-6 x the global max; at most 25 % of a tensor's channels may take the floor).  dB, dC and d dt are sums
over channels: their "channel" is the time step (all sequences, all columns of the step).  Not the single (sequence, step) row: at
dt_rank 1 that row is ONE number, a cancelling sum over the channels of products whose ddelta operand the bf16 kernel rounds to
bf16 (as the reference's GEMM does), and the bound would be a relative one on that sum -- the rounding of the operand alone, emulated
in fp64, misses it at 3.6e-2 on the (2, 37, 72) rank-1 case.  The numbers are those of the existing tests.
"""
import functools
import importlib.util
import math
import os

import pytest
import torch

from oracle import conmamba_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

_spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(os.path.dirname(__file__), "golden", "synth.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)

# (rtol, atol x scale): test_scan_rows_bwd_two_directions / test_conv_cl_bwd / test_bimamba_d256_forward_backward
SCAN_DATA = {torch.float32: (2e-3, 2e-4), torch.bfloat16: (2e-2, 1.2e-2)}
SCAN_PAR = {torch.float32: (3e-3, 3e-4), torch.bfloat16: (2e-2, 5e-3)}
SCAN_DW = {torch.float32: (3e-3, 3e-4), torch.bfloat16: (2e-2, 8e-3)}
CONV_DATA = {torch.float32: (2e-4, 2e-5), torch.bfloat16: (1.6e-2, 1e-2)}
CONV_PAR = {torch.float32: (1e-3, 1e-4), torch.bfloat16: (1e-2, 2e-3)}
MIXER_F32 = (3e-3, 3e-4)


def chan_metric(got, ref, axis):
    """-> (per-channel max |got - ref|, per-channel scale, channels under the floor, |diff| and |ref| as (channel, rest))."""
    g, r = got.detach().double().cpu(), ref.detach().double().cpu()
    assert g.shape == r.shape, (g.shape, r.shape)
    axis = (axis,) if isinstance(axis, int) else tuple(axis)
    perm = list(axis) + [d for d in range(r.dim()) if d not in axis]
    n = math.prod(r.shape[a] for a in axis)
    diff, ra = (g - r).abs().permute(perm).reshape(n, -1), r.abs().permute(perm).reshape(n, -1)
    mx = ra.amax(1)
    floor = 1e-6 * float(mx.max())
    return diff.amax(1), mx.clamp_min(floor), mx < floor, diff, ra


def chan_check(name, got, ref, axis, tol, report=None):
    """Per channel c: err_c = max |got - ref|, scale_c = max(max |ref| over c, 1e-6 x global max |ref|); err_c <= rtol scale_c, and
    every element within atol scale_c + rtol |ref| (assert_close's form on the channel's scale).  -> worst err_c / scale_c."""
    rtol, atol = tol
    assert torch.isfinite(got).all(), f"{name}: not finite"
    err, scale, floored, diff, ra = chan_metric(got, ref, axis)
    assert float(floored.double().mean()) <= 0.25, f"{name}: {int(floored.sum())} of {floored.numel()} channels under the floor"
    rel = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst, c = float(rel.max()), int(rel.argmax())
    if report is not None:
        report[name] = max(report.get(name, 0.0), worst)
    bound = torch.minimum(rtol * scale[:, None].expand_as(diff), atol * scale[:, None] + rtol * ra)
    bad = diff > bound
    assert not bool(bad.any()), (f"{name}: {int(bad.any(1).sum())} of {bad.shape[0]} channels out of bounds; worst channel {c}: err {float(err[c]):.3e}, "
                                 f"scale {float(scale[c]):.3e} (err / scale {worst:.3e}, rtol {rtol:.1e} atol {atol:.1e}; tensor max |ref| {float(ra.max()):.3e})")
    return worst


def same_bits(first, second):
    for o, o2 in zip(first, second):
        for k in o:
            assert (o[k] is None and o2[k] is None) or torch.equal(o[k], o2[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# scan backward: cases and references
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_case(b, l, e, rank, dtype, seed, revs=(False, True), recipe="plain", with_d=True, with_bias=True):
    """Host tensors of one launch (never modified afterwards).  recipe "extreme": test_scan_rows_extreme_time_steps' numbers."""
    P = 16 if rank <= 16 else 32
    RW = P + 32
    n = len(revs)
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(b, l, e, generator=gen).to(dtype)
    dmix = (torch.randn(b, l, e, generator=gen) * 0.5).to(dtype)                    # shared by the directions, as in BiMamba v2
    ucat = torch.randn(b, l, n * e, generator=gen).to(dtype)
    xcat = torch.randn(b, l, n * RW, generator=gen)
    par = []
    for i in range(n):
        xd = xcat[:, :, RW * i:RW * (i + 1)]
        xd[:, :, rank:P] = 0.0
        if recipe == "extreme":
            assert e == 64 and rank == 16
            xd[:, :, P:P + 16] *= 3.0
            xd[0, 10:20] = 0.0                                                      # a stretch of all-zero projections
            A = -torch.exp(torch.randn(e, 16, generator=gen) * 2.0)                 # |A| from 0.01 to 100
            bias = torch.cat([torch.full((16,), 30.0), torch.full((16,), -25.0), torch.randn(32, generator=gen)])
        else:
            A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
            bias = torch.randn(e, generator=gen) - 1
        Wdt = torch.randn(e, rank, generator=gen) * 0.3
        D = torch.randn(e, generator=gen)
        par.append(dict(A=A, Wdt=Wdt, D=D if with_d else None, bias=bias if with_bias else None))
    return dict(b=b, l=l, e=e, rank=rank, P=P, RW=RW, dtype=dtype, revs=revs, z=z, dmix=dmix, ucat=ucat, xcat=xcat.to(dtype), par=par)


def reference(case, work_dtype=torch.float64):
    """Per direction: the oracle's gradients in (batch, seqlen, .) layout + d dt and ddt_weight."""
    e, rank, P, RW, dtype = case["e"], case["rank"], case["P"], case["RW"], case["dtype"]
    tr = lambda t: t.double().transpose(1, 2)
    refs = []
    for i, rev in enumerate(case["revs"]):
        p = case["par"][i]
        u = case["ucat"][:, :, e * i:e * (i + 1)]
        xd = case["xcat"][:, :, RW * i:RW * (i + 1)].double()
        Wq = p["Wdt"].to(dtype).double()                                            # bf16 I/O: the product runs on the bf16-rounded weight
        delta = torch.einsum("er,blr->bel", Wq, xd[:, :, :rank])
        Bm, Cm = xd[:, :, P:P + 16].transpose(1, 2), xd[:, :, P + 16:].transpose(1, 2)
        f = (lambda t: t.flip(-1)) if rev else (lambda t: t)
        r = O.selective_scan_bwd(f(tr(u)), f(delta), p["A"], f(Bm), f(Cm), p["D"], f(tr(case["z"])), p["bias"], f(tr(case["dmix"])), True,
                                 work_dtype=work_dtype)
        r = {k: (f(v).double() if v is not None and v.dim() == 3 else (None if v is None else v.double())) for k, v in r.items()}
        out = dict(du=r["du"].transpose(1, 2), dz=r["dz"].transpose(1, 2), dB=r["dB"].transpose(1, 2), dC=r["dC"].transpose(1, 2),
                   ddt=torch.einsum("bel,er->blr", r["ddelta"], Wq), dW=torch.einsum("bel,blr->er", r["ddelta"], xd[:, :, :rank]),
                   dA=r["dA"], dD=r["dD"], ddelta_bias=r["ddelta_bias"])
        refs.append(out)
    return refs


@functools.lru_cache(maxsize=None)
def cached_reference(*key):
    return reference(make_case(*key))


def forward(ops, case):
    """The training forward on the case -> (direction descriptors ready for scan_cl_bwd, z on the device)."""
    b, l, e, RW, dtype = case["b"], case["l"], case["e"], case["RW"], case["dtype"]
    n = len(case["revs"])
    gz, gd, gu, gx = case["z"].to(DEV), case["dmix"].to(DEV), case["ucat"].to(DEV), case["xcat"].to(DEV)
    ycat = torch.zeros(b, l, n * e, dtype=dtype, device=DEV)
    pcat = torch.zeros(b, l, n * e, dtype=dtype, device=DEV)
    dirs = []
    for i, rev in enumerate(case["revs"]):
        p = case["par"][i]
        dirs.append(dict(u=gu[:, :, e * i:e * (i + 1)], xdbl=gx[:, :, RW * i:RW * (i + 1)], A=p["A"].to(DEV),
                         D=None if p["D"] is None else p["D"].to(DEV), delta_bias=None if p["bias"] is None else p["bias"].to(DEV),
                         dt_weight=ops.pad_dt_weight(p["Wdt"].to(DEV)), reverse=rev, out=ycat[:, :, e * i:e * (i + 1)],
                         ypre=pcat[:, :, e * i:e * (i + 1)], ckpt=torch.empty(ops.scan_ckpt_shape(b, l, e), device=DEV)))
    ops.scan_cl_fwd(dirs, z=gz, delta_softplus=True, time_chunks=1)
    for dd in dirs:
        dd["dout"] = gd
    return dirs, gz


def check_scan(outs, refs, case, report=None, tag=""):
    """EVERY output of every direction against the oracle, per channel."""
    rank, P, dtype = case["rank"], case["P"], case["dtype"]
    data, par, dw = SCAN_DATA[dtype], SCAN_PAR[dtype], SCAN_DW[dtype]
    assert len(outs) == len(refs) == len(case["revs"])
    for i, (o, r) in enumerate(zip(outs, refs)):
        nm = lambda k: f"{tag}{k}[{'rev' if case['revs'][i] else 'fwd'}]"
        x = o["dxdbl"].float()
        chan_check(nm("du"), o["du"].float(), r["du"], 2, data, report)
        chan_check(nm("dz"), o["dz"].float(), r["dz"], 2, data, report)
        chan_check(nm("dB"), x[:, :, P:P + 16], r["dB"], 1, data, report)
        chan_check(nm("dC"), x[:, :, P + 16:], r["dC"], 1, data, report)
        chan_check(nm("ddt"), x[:, :, :rank], r["ddt"], 1, data, report)
        assert x.shape[-1] == P + 32 and (rank == P or float(x[:, :, rank:P].abs().max()) == 0.0), "dxdbl padding columns"
        chan_check(nm("dA"), o["dA"], r["dA"], 0, par, report)
        chan_check(nm("ddt_weight"), o["ddt_weight"][:, :rank], r["dW"], 0, dw, report)
        assert rank == P or float(o["ddt_weight"][:, rank:].abs().max()) == 0.0, "ddt_weight padding columns"
        for k in ("dD", "ddelta_bias"):
            if r[k] is None:
                assert o[k] is None, k
            else:
                chan_check(nm(k), o[k], r[k], 0, par, report)


def print_report(title, report):
    print(f"\n{title}")
    for k in sorted(report):
        print(f"  {k:28s} worst per-channel err / scale {report[k]:.3e}")


# ------------------------------------------------------------------------------------------------------------------------
# 1. boundary lengths and widths
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l", [1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33])
@pytest.mark.parametrize("e", [8, 72])
@pytest.mark.parametrize("dtype,rank", [(torch.float32, 16), (torch.bfloat16, 9), (torch.bfloat16, 32)])
def test_scan_bwd_boundary_lengths(l, e, dtype, rank):
    """Sequences below one 8-step half block, on and next to the half-block / block boundaries; dim 8 (one channel octet of one
    wave, every other lane masked) and 72 (a full 64-channel group + 8).  L = 1: dA is exactly 0 (no earlier state), so the kernel's
    must be: a_t h_{t-1} as h_t - w_t B_t left the rounding residue of w_t B_t there (1e-8) before it was formed as a_t x h_{t-1}.
    Also the forward's training outputs at these lengths."""
    from mamba_asr_amd import ops
    key = (2, l, e, rank, dtype, 1000 * l + e + rank)
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    outs = ops.scan_cl_bwd(dirs, gz)
    torch.cuda.synchronize()
    check_scan(outs, refs, case)
    silu = torch.nn.functional.silu(gz.float())
    for dd in dirs:
        assert dd["ckpt"].shape == ops.scan_ckpt_shape(2, l, e) and torch.isfinite(dd["ckpt"]).all()
        # out = y silu(z) and ypre = y, each rounded once to the I/O dtype: fp32 as test_scan_rows_fwd_training_outputs; bf16 (8
        # significant bits): half an ulp is up to 2^-8 of the value, two independent roundings 2^-7 (+ 1 % for the fp32 silu)
        rt, at = (1e-5, 1e-6) if dtype == torch.float32 else (1.01 * 2.0 ** -7, 1e-6)
        torch.testing.assert_close(dd["out"].float(), dd["ypre"].float() * silu, rtol=rt, atol=at)
    same_bits(outs, ops.scan_cl_bwd(dirs, gz))


# ------------------------------------------------------------------------------------------------------------------------
# 2. extreme time steps
# ------------------------------------------------------------------------------------------------------------------------
EXTREME = {}            # worst per-channel error per tensor over the extreme cases (printed by the last of them)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("l,chunks", [(70, 1), (70, 3), (20, 8), (33, 2)])
def test_scan_bwd_extreme_time_steps(dtype, l, chunks):
    """The forward test's recipe in the backward: time steps beyond softplus' linear threshold (bias 30), negligible ones (bias -25),
    decays that underflow to 0, |A| from 0.01 to 100, a stretch of all-zero projections; one pass and cut along time (70 / 3: chunks
    of 32 with a ragged last one; 20 / 8: more chunks asked for than blocks; 33 / 2: a last chunk of one step).  Every output finite
    and within the per-channel bounds.  The fp64 oracle's plain recurrence evaluated in fp32 on this recipe stays within 5e-6 of
    fp64 under the same metric (worst: ddelta_bias 5.0e-6, dA 3.4e-6), so fp32 arithmetic is no excuse here.
    Measured on an MI355X, worst per-channel err / scale over the four cases and both directions (profiles/scan_bwd_edges): fp32
    ddelta_bias 1.1e-4, dD 2.5e-5, dA 2.7e-6, every other tensor <= 1.7e-6 (bounds 2e-3 / 3e-3); bf16 dz 6.3e-3, d dt 6.1e-3,
    du 3.6e-3, dC 3.5e-3, dB 3.4e-3 (bound 2e-2: their own bf16 rounding), dD 2.3e-5, ddt_weight 1.3e-5, ddelta_bias 8.7e-6,
    dA 3.3e-6 (bound 2e-2).  With a_t h_{t-1} formed as h_t - w_t B_t the fp32 cases missed d dt (3.5e-4 of the step's scale on an
    element bounded by 2e-4 of it) and ddelta_bias (7.2e-3)."""
    from mamba_asr_amd import ops
    key = (2, l, 64, 16, dtype, 99 + l, (False, True), "extreme")
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    outs = ops.scan_cl_bwd(dirs, gz, time_chunks=chunks)
    torch.cuda.synchronize()
    for o in outs:
        for k, v in o.items():
            assert torch.isfinite(v).all(), k
    report = {}
    try:
        check_scan(outs, refs, case, report, tag=f"{'f32' if dtype == torch.float32 else 'bf16'} L{l} c{chunks} ")
    finally:
        print_report(f"extreme time steps, {dtype}, L = {l}, time_chunks = {chunks}", report)
    same_bits(outs, ops.scan_cl_bwd(dirs, gz, time_chunks=chunks))


# ------------------------------------------------------------------------------------------------------------------------
# 3. options
# ------------------------------------------------------------------------------------------------------------------------
OPT = (2, 37, 72, 16, torch.float32, 4242)


def test_scan_bwd_da_log():
    """da_log=True (the only mode the model uses) returns dA x A: the reduce pass multiplies the same fp32 sum by the same fp32 A as
    torch does on the da_log=False launch's result: equal bits."""
    from mamba_asr_amd import ops
    case, refs = make_case(*OPT), cached_reference(*OPT)
    dirs, gz = forward(ops, case)
    plain = ops.scan_cl_bwd(dirs, gz, da_log=False)
    logs = ops.scan_cl_bwd(dirs, gz, da_log=True)
    torch.cuda.synchronize()
    check_scan(plain, refs, case)
    for o, lg, dd in zip(plain, logs, dirs):
        assert torch.equal(lg["dA"], o["dA"] * dd["A"])
        for k in o:
            if k != "dA":
                assert torch.equal(lg[k], o[k]), k
    same_bits(logs, ops.scan_cl_bwd(dirs, gz, da_log=True))


def test_scan_bwd_without_d_and_bias():
    """D=None and delta_bias=None: no dD / ddelta_bias, every other output as the oracle's called with None."""
    from mamba_asr_amd import ops
    key = OPT + ((False, True), "plain", False, False)
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    outs = ops.scan_cl_bwd(dirs, gz)
    torch.cuda.synchronize()
    for o in outs:
        assert o["dD"] is None and o["ddelta_bias"] is None
    check_scan(outs, refs, case)
    same_bits(outs, ops.scan_cl_bwd(dirs, gz))


def test_scan_bwd_reverse_direction_alone():
    from mamba_asr_amd import ops
    key = OPT + ((True,),)
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    outs = ops.scan_cl_bwd(dirs, gz)
    torch.cuda.synchronize()
    check_scan(outs, refs, case)
    same_bits(outs, ops.scan_cl_bwd(dirs, gz))


@pytest.mark.parametrize("rank", [1, 17, 24])
def test_scan_bwd_bf16_ranks(rank):
    """dt_rank 1 (one live column of the 16-wide tile), 17 (one live column of the second tile) and 24 in bf16.  At rank 1 a row of
    ddt_weight is ONE cancelling sum over the steps: with its ddelta operand rounded to bf16 the kernel missed 4 (forward) and 6
    (reverse) of the 72 rows by 0.33 / 0.94 of the row's own scale (bound 2e-2) -- the figure the rounding alone gives in fp64 -- and
    keeps the operand as bf16 head + tail since."""
    from mamba_asr_amd import ops
    key = (2, 37, 72, rank, torch.bfloat16, 777 + rank)
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    outs = ops.scan_cl_bwd(dirs, gz)
    torch.cuda.synchronize()
    check_scan(outs, refs, case)
    same_bits(outs, ops.scan_cl_bwd(dirs, gz))


# ------------------------------------------------------------------------------------------------------------------------
# 4. views and guards
# ------------------------------------------------------------------------------------------------------------------------
SENTINEL = -65536.0                                  # exact in bf16; no result of these cases comes near it


def _poisoned(t, left, right, rows=3):
    """t (b, l, w) as a view of a NaN-filled (b, l + rows, left + w + right) buffer."""
    b, l, w = t.shape
    buf = torch.full((b, l + rows, left + w + right), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :l, left:left + w] = t
    return buf[:, :l, left:left + w]


def _guarded(shape, dtype, left, right, rows=3):
    """-> (sentinel-filled buffer, its (b, l, w) view, mask of the elements outside the view)."""
    b, l, w = shape
    buf = torch.full((b, l + rows, left + w + right), SENTINEL, dtype=dtype, device=DEV)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[:, :l, left:left + w] = False
    return buf, buf[:, :l, left:left + w], outside


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_scan_bwd_views_and_guards(dtype):
    """Every input a view of a wider, longer NaN-filled buffer, every output a view of a sentinel-filled one (8 extra columns in front,
    16 behind, 3 rows behind the sequence: 16-byte aligned, strides multiples of 8 elements): the results are those of the contiguous
    launch bit for bit -- lanes past dim and steps past L read nothing into them -- and no element outside the views is written."""
    from mamba_asr_amd import ops
    b, l, e = 2, 21, 72
    key = (b, l, e, 16, dtype, 2100)
    case, refs = make_case(*key), cached_reference(*key)
    dirs, gz = forward(ops, case)
    want = ops.scan_cl_bwd(dirs, gz)
    check_scan(want, refs, case)
    vz = _poisoned(gz, 8, 16)
    vdirs, guards = [], []
    for dd in dirs:
        v = dict(dd)
        for k in ("u", "xdbl", "dout", "ypre"):
            v[k] = _poisoned(dd[k], 8, 16)
        g = {k: _guarded((b, l, w), dtype, 8, 16) for k, w in (("du", e), ("dz", e), ("dxdbl", case["RW"]))}
        v.update({k: g[k][1] for k in g})
        vdirs.append(v), guards.append(g)
    got = ops.scan_cl_bwd(vdirs, vz)
    torch.cuda.synchronize()
    for o, w_, g in zip(got, want, guards):
        for k in w_:
            assert torch.equal(o[k], w_[k]), k
        for k, (buf, view, outside) in g.items():
            assert o[k].data_ptr() == view.data_ptr()
            assert bool((buf[outside] == SENTINEL).all()), f"{k}: written outside its view"
    same_bits(got, ops.scan_cl_bwd(vdirs, vz))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_bwd_views_and_guards(dtype):
    """cm_conv_cl_bwd on views (2 extra columns in front, 4 behind, 3 rows behind the sequence: 4-byte aligned, even strides) of NaN /
    sentinel buffers against its contiguous launch, bit for bit; nothing outside dx / dz written."""
    from mamba_asr_amd import ops
    b, l, e = 2, 21, 70
    gen = torch.Generator().manual_seed(2170)
    t = lambda *s: torch.randn(*s, generator=gen).to(dtype).to(DEV)
    x, duf, dub, dzf, dzb = (t(b, l, e) for _ in range(5))
    w = [(torch.randn(e, 4, generator=gen) * 0.5).to(DEV) for _ in range(2)]
    bs = [(torch.randn(e, generator=gen) * 0.2).to(DEV) for _ in range(2)]
    want = ops.conv_cl_bwd(x, w[0], bs[0], duf, w[1], bs[1], dub, dz_f=dzf, dz_b=dzb)
    gx, gz = _guarded((b, l, e), dtype, 2, 4), _guarded((b, l, e), dtype, 2, 4)
    pv = [_poisoned(v, 2, 4) for v in (x, duf, dub, dzf, dzb)]
    got = ops.conv_cl_bwd(pv[0], w[0], bs[0], pv[1], w[1], bs[1], pv[2], dz_f=pv[3], dz_b=pv[4], dx=gx[1], dz=gz[1])
    torch.cuda.synchronize()
    for a_, b_ in zip(got, want):
        assert torch.equal(a_, b_)
    for buf, view, outside in (gx, gz):
        assert bool((buf[outside] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------
# 5. cm_conv_cl_bwd at short lengths
# ------------------------------------------------------------------------------------------------------------------------
def _conv_case(ops, b, l, e, dtype, two, with_dz):
    gen = torch.Generator().manual_seed(100 * l + e)
    x = torch.randn(b, l, e, generator=gen).to(dtype)
    du = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    dzs = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    w = [torch.randn(e, 4, generator=gen) * 0.5 for _ in range(2)]
    bs = [torch.randn(e, generator=gen) * 0.2 for _ in range(2)]
    gx, gdu, gdz = x.to(DEV), du.to(DEV), dzs.to(DEV)
    kw = dict(du_b=gdu[:, :, e:], weight_b=w[1].to(DEV), bias_b=bs[1].to(DEV)) if two else {}
    if with_dz:
        kw["dz_f"] = gdz[:, :, :e]
        if two:
            kw["dz_b"] = gdz[:, :, e:]
    run = lambda: ops.conv_cl_bwd(gx, w[0].to(DEV), bs[0].to(DEV), gdu[:, :, :e], **kw)
    dx, dz, dwf, dbf, dwb, dbb = run()
    torch.cuda.synchronize()
    tr = lambda t: t.double().transpose(1, 2)
    rdx, rdw, rdb = O.causal_conv1d_bwd(tr(x), w[0], bs[0], tr(du[:, :, :e]), True)
    want_dx, want_dz = rdx, dzs[:, :, :e].double()
    data, par = CONV_DATA[dtype], CONV_PAR[dtype]
    if two:
        bdx, bdw, bdb = O.causal_conv1d_bwd(tr(x).flip(-1), w[1], bs[1], tr(du[:, :, e:]).flip(-1), True)
        want_dx = want_dx + bdx.flip(-1)
        want_dz = want_dz + dzs[:, :, e:].double()
        chan_check("dweight_b", dwb, bdw, 0, par)
        chan_check("dbias_b", dbb, bdb, 0, par)
    else:
        assert dwb is None and dbb is None
    chan_check("dx", dx.float(), want_dx.transpose(1, 2), 2, data)
    if with_dz:
        chan_check("dz", dz.float(), want_dz, 2, data)
    else:
        assert dz is None
    chan_check("dweight_f", dwf, rdw, 0, par)
    chan_check("dbias_f", dbf, rdb, 0, par)
    for a_, b_ in zip(run(), (dx, dz, dwf, dbf, dwb, dbb)):
        assert (a_ is None and b_ is None) or torch.equal(a_, b_)


@pytest.mark.parametrize("l", [1, 2, 3, 4, 5, 7, 8, 33])
@pytest.mark.parametrize("e", [6, 70])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("two", [True, False])
def test_conv_bwd_short_sequences(l, e, dtype, two):
    """L < 4: one chunk is the first and the last edge chunk and the window is longer than the sequence; L <= 7: no interior chunk;
    8 and 33: interior chunks next to the edges.  dim 6 / 70: a handful of live threads / a ragged last wave."""
    from mamba_asr_amd import ops
    _conv_case(ops, 2, l, e, dtype, two, True)


@pytest.mark.parametrize("l", [5, 33])
@pytest.mark.parametrize("two", [True, False])
def test_conv_bwd_bf16_second_workgroup(l, two):
    """dim 514 in bf16 = 257 channel words: a second workgroup along x with one live thread."""
    from mamba_asr_amd import ops
    _conv_case(ops, 2, l, 514, torch.bfloat16, two, True)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_bwd_without_dz(dtype):
    from mamba_asr_amd import ops
    _conv_case(ops, 2, 7, 70, dtype, True, False)


# ------------------------------------------------------------------------------------------------------------------------
# 6. the mixer node at decoder lengths
# ------------------------------------------------------------------------------------------------------------------------
def _mixer(kind):
    from mamba_asr_amd.modules.mamba.bimamba import Mamba, UniMamba
    m = Mamba(64, d_state=16, d_conv=4, expand=2, bimamba_type="v2") if kind == "bi" else UniMamba(d_model=64, d_state=16, d_conv=4, expand=2)
    m.load_state_dict(S.synth_like(m, 640), strict=True)
    return m


def _oracle_grads(kind, sd, names, x, dy):
    """fp64 autograd through the oracle -> (y, [dx] + the parameters' gradients in ``names`` order)."""
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    scan64 = functools.partial(O.selective_scan, work_dtype=torch.float64)          # the mixers hand work_dtype to everything but the scan
    y = (O.bimamba_v2 if kind == "bi" else O.mamba_uni)(p, xr, scan=scan64, work_dtype=torch.float64)
    grads = torch.autograd.grad(y, [xr] + [p[k] for k in names], dy.double())
    return y.detach(), [g.detach() for g in grads]


def _rel_l2(a, b):
    """|a - b| / |b|; (0, 0) -> 0, (x, 0) -> inf."""
    d, n = float((a.double() - b.double()).norm()), float(b.double().norm())
    return d / n if n > 0 else (0.0 if d == 0 else float("inf"))


@functools.lru_cache(maxsize=None)
def _mixer_reference(kind, T):
    m = _mixer(kind)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    names = [k for k, _ in m.named_parameters()]
    x, dy = S.synth_input(f"edges.{kind}.x", (2, T, 64), 640), S.synth_input(f"edges.{kind}.dy", (2, T, 64), 640)
    y, g = _oracle_grads(kind, sd, names, x, dy)
    rb = lambda t: t.bfloat16().float()
    yq, gq = _oracle_grads(kind, {k: rb(v) for k, v in sd.items()}, names, rb(x), dy)
    return x, dy, names, y, g, yq, gq


@pytest.mark.parametrize("T", [1, 3, 8, 17])
@pytest.mark.parametrize("kind", ["bi", "uni"])
def test_mixer_node_decoder_lengths_fp32(kind, T):
    """bimamba.Mamba (v2) / UniMamba, d_model 64 (E = 128, dt_rank 4), at the label-sequence lengths the S2S Mamba decoder trains
    on: output, input gradient and every parameter's gradient against fp64 autograd through the oracle, per channel (last axis of
    (B, T, D) tensors, first axis of parameters).  Measured on an MI355X: worst per-channel err / scale 4.0e-4 (dt_proj.bias,
    bidirectional, T = 3), output 2.2e-6, dx 3.2e-6 (bound 3e-3)."""
    x, dy, names, y, g, _, _ = _mixer_reference(kind, T)
    m = _mixer(kind).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = m(xg)
    grads = torch.autograd.grad(out, [xg] + [p for _, p in m.named_parameters()], dy.to(DEV))
    torch.cuda.synchronize()
    report = {}
    try:
        chan_check("y", out, y, 2, MIXER_F32, report)
        chan_check("dx", grads[0], g[0], 2, MIXER_F32, report)
        for k, a_, b_ in zip(names, grads[1:], g[1:]):
            chan_check("g." + k, a_, b_, 0, MIXER_F32, report)
    finally:
        print_report(f"mixer node fp32, {kind}, T = {T}", report)


@pytest.mark.parametrize("T", [1, 3, 8, 17])
@pytest.mark.parametrize("kind", ["bi", "uni"])
def test_mixer_node_decoder_lengths_bf16(kind, T):
    """The same under bf16 autocast (the bidirectional mixer takes cm_conv_xproj).  Per tensor, d_q = the relative L2 distance between
    the fp64 oracle on the bf16-rounded input and parameters and on the unrounded ones: what ONE rounding of the operands costs.  The
    node rounds xz, u, x_dbl, y, dxz and du once each: six independent roundings ~ 2.5 x one; bound 4 x d_q on the relative L2
    distance to the unrounded fp64 oracle.  Measured on an MI355X: worst pair d_q 2.65e-3 / err 7.30e-3 (2.76 x: the gradient of D,
    UniMamba, T = 1); the output 1.43 x, dx 1.86 x at most; the gradient of A_log at T = 1 is exactly 0 on both sides."""
    x, dy, names, y, g, yq, gq = _mixer_reference(kind, T)
    m = _mixer(kind).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m(xg)
    grads = torch.autograd.grad(out, [xg] + [p for _, p in m.named_parameters()], dy.to(DEV))
    torch.cuda.synchronize()
    rows = [("y", out, y, yq), ("dx", grads[0], g[0], gq[0])] + [("g." + k, a_, b_, c_) for k, a_, b_, c_ in zip(names, grads[1:], g[1:], gq[1:])]
    bad = []
    print(f"\nmixer node bf16, {kind}, T = {T}")
    for name, got, ref, refq in rows:
        assert torch.isfinite(got).all(), name
        dq, err = _rel_l2(refq, ref), _rel_l2(got.detach().cpu(), ref)
        print(f"  {name:24s} d_q {dq:.3e}  err {err:.3e}  err / d_q {err / dq if dq > 0 else float('nan'):.2f}")
        if not err <= 4 * dq:
            bad.append((name, dq, err))
    assert not bad, bad
