"""Every layer-configuration gate, run to a value on both of its sides (tests/layer_config_ref.py: the fp64 reference and CASES).

(a) inference, every case, fp32 and bf16: fused.encoder_forward where fused.supports holds, else the module path; the launch the
    gate flips is present or absent as the table says, the library GEMM count is the table's, the output is within the project's
    bounds of the fp64 reference;
(b) the autograd route (eval mode, grad enabled: dropout off), fp32 and bf16 autocast: output, input gradient and every parameter
    gradient against torch autograd over the fp64 reference, the backward kernels the gates select, and the same set of parameters
    with a gradient;
(c) the causal cases whole and streamed in chunks of 5 and 14 rows against the same reference; the documented refusals;
(d) the kernels at the limits the gates allow, op-level, against fp64 on the kernel's own bf16-rounded operands.

Worst error / allowance per case, measured on MI355X (1.000 = the bound; nothing is asserted against these figures; '-' = the
route refuses the case as documented):

    case                 infer fp32  infer bf16  train fp32  train bf16  stream 5/14 fp32  stream 5/14 bf16
    expand1                   0.002       0.407       0.002       0.250
    expand2                   0.002       0.317       0.001       0.230
    expand4                   0.001       0.334       0.002       0.235
    expand8                   0.002       0.282       0.002       0.261
    expand8_dt_rank24         0.002       0.304       0.001       0.259
    expand4_dt_rank24         0.002       0.314       0.001       0.337
    expand1p5_d200            0.001       0.418       0.001       0.241
    dt_rank5                  0.002       0.345       0.001       0.241
    dt_rank16                 0.002       0.317       0.001       0.230
    dt_rank17                 0.002       0.383       0.003       0.241
    dt_rank24                 0.002       0.625       0.001       0.318
    dt_rank32                 0.002       0.475       0.002       0.321
    dt_rank33                 0.003       0.701       0.004       0.436
    dt_rank40                 0.002       0.674       0.003       0.377
    d144                      0.001       0.309       0.001       0.266
    d192                      0.002       0.376       0.001       0.265
    d256                      0.002       0.317       0.001       0.230
    d264                      0.002       0.441       0.002       0.322
    d1024                     0.002       0.722       0.001       0.354
    d1032                     0.002       0.878       0.002       0.429
    ffn256                    0.002       0.317       0.001       0.230
    ffn264                    0.002       0.438       0.001       0.226
    ffn2048                   0.002       0.303       0.002       0.218
    ffn2304                   0.002       0.320       0.001       0.202
    ffn2056                   0.001       0.305       0.001       0.194
    k31                       0.002       0.317       0.001       0.230
    k15                       0.001       0.416       0.001       0.339
    k32_causal                0.001       0.366       0.001       0.226
    k33                       0.002       0.544       0.001       0.293
    d_state8                  0.002       0.421       0.001       0.271
    d_conv3                   0.002       0.379       0.002       0.315
    opt_bias                  0.001       0.390       0.004       0.260
    opt_no_conv_bias          0.001       0.278       0.001       0.226
    opt_no_devide             0.002       0.537       0.001       0.332
    opt_layer_scale           0.001       0.301       0.001       0.247
    opt_all                   0.001       0.380       0.001       0.249
    causal_expand1            0.002       0.406       0.001       0.239     0.002 / 0.002     0.406 / 0.406
    causal_expand4            0.001       0.323       0.001       0.235     0.001 / 0.002     0.323 / 0.323
    causal_dt_rank5           0.002       0.300       0.001       0.220     0.001 / 0.002     0.300 / 0.300
    causal_dt_rank24          0.003       0.606       0.002       0.473                 -     0.606 / 0.606
    causal_dt_rank40          0.003       0.482       0.002       0.398                 -                 -

The file takes 17 s on MI355X (202 tests, the slowest 2.6 s: the first launch of a process).
"""
import copy
from collections import Counter

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import layer_config_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
# test_hip_parity_r3.py::test_training_step_loss_and_every_gradient_vs_oracle's bounds
TRAIN_L2 = {"fp32": 2e-3, "bf16": 6e-2}
TRAIN_ELEM_FP32 = 2e-3
RATIOS = {}                                     # (section, case, dtype) -> worst error / allowance; printed by the last test


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_fault():
    """A faulted context fails every later launch: end the session instead of starting them."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                    # pragma: no cover
        pytest.exit(f"GPU fault, nothing more is launched: {e}", returncode=3)


class _LibraryGemms(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.count += func.overloadpacket.__name__ in ("mm", "addmm", "_addmm_activation", "bmm")
        return func(*args, **(kwargs or {}))


_BUILT = {}


def _case(name):
    """-> (case, CPU encoder, input, fp64 reference dict), computed once per case and left unchanged."""
    if name not in _BUILT:
        case = R.CASES[name]
        enc, x = R.build(case)
        p = R.params64(enc, requires_grad=True)
        xg = x.double().requires_grad_(True)
        out = R.reference(case, p, xg)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
        (out * w).sum().backward()
        ref = dict(out=out.detach(), w=w, dx=xg.grad, grads={k: v.grad for k, v in p.items() if v.grad is not None})
        _BUILT[name] = (case, enc, x, ref)
    return _BUILT[name]


def _on_gpu(enc):
    return copy.deepcopy(enc).to(DEV).eval()


def _logged(fn):
    """-> (result, Counter of native launch names, library GEMM count)."""
    from mamba_asr_amd import ops
    ops.LAUNCH_LOG = []
    try:
        with _LibraryGemms() as gemms:
            out = fn()
        torch.cuda.synchronize()
        names = Counter(e[0] for e in ops.LAUNCH_LOG)
    finally:
        ops.LAUNCH_LOG = None
    return out, names, gemms.count


def _ratio(got, ref, rtol, atol):
    """Worst |error| / allowance: assert_close's criterion as one figure."""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float(((got - ref).abs() / (atol + rtol * ref.abs())).max())


def _rel_l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float((got - ref).norm() / ref.norm().clamp_min(1e-30))


# ------------------------------------------------------------------------------------------------------------------------
# (a) inference
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(R.CASES))
def test_inference_on_both_sides_of_the_gate(name, dt):
    from mamba_asr_amd import fused
    case, enc, x, ref = _case(name)
    dtype = DTYPES[dt]
    encg, xg = _on_gpu(enc), x.to(DEV)
    assert all(fused.supports(l) for l in encg.layers) == case.supports

    def run():
        with torch.no_grad():
            if case.supports:
                return fused.encoder_forward(encg, xg, dtype=dtype, streams=1)
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
                return encg(xg)[0]
    out, names, gemms = _logged(run)
    r = _ratio(out, ref["out"], **R.INFER_TOL[dtype])
    RATIOS[("infer", name, dt)] = r
    print(f"{name} {dt}: worst error / allowance {r:.3f}; launches {dict(names)}; library GEMMs {gemms}")
    assert (case.flip in names) == getattr(case, dt), (case.gate, dict(names))
    want_gemms = R.library_gemms(case, dtype)
    if want_gemms is not None:
        assert gemms == want_gemms * case.layers, (gemms, want_gemms)
        scans = names["cm_scan_cl_fwd"]
        assert scans == case.layers                              # one scan launch per layer, both directions (folded or not)
    assert r <= 1.0, f"{name} {dt}: {r:.3f} x the allowance ({case.gate})"


# ------------------------------------------------------------------------------------------------------------------------
# (b) the autograd route
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(R.CASES))
def test_training_route_on_both_sides_of_the_gate(name, dt):
    case, enc, x, ref = _case(name)
    dtype = DTYPES[dt]
    encg = _on_gpu(enc)                                          # eval mode, grad enabled: the autograd path with dropout off
    xg = x.to(DEV).requires_grad_(True)
    w = ref["w"].float().to(DEV)

    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
            out = encg(xg)[0]
        (out.float() * w).sum().backward()
        return out
    out, names, _ = _logged(run)
    grads = {k: p.grad for k, p in encg.named_parameters() if p.grad is not None}
    assert set(grads) == set(ref["grads"]), sorted(set(grads) ^ set(ref["grads"]))
    stats = {"out": (out, ref["out"]), "dx": (xg.grad, ref["dx"]), **{k: (grads[k], ref["grads"][k]) for k in grads}}
    l2 = {k: _rel_l2(g, r) for k, (g, r) in stats.items()}
    worst = max(l2, key=l2.get)
    ratio = l2[worst] / TRAIN_L2[dt]
    if dt == "fp32":
        elem = {k: float((g.detach().double().cpu() - r).abs().max() / r.abs().max().clamp_min(1e-30)) for k, (g, r) in stats.items()}
        ratio = max(ratio, max(elem.values()) / TRAIN_ELEM_FP32)
    RATIOS[("train", name, dt)] = ratio
    print(f"{name} {dt}: worst relative L2 {l2[worst]:.2e} ({worst}); worst / allowance {ratio:.3f}; launches {dict(names)}")
    want = R.train_kernels(case, dtype)
    got = {k: k in names for k in R.BWD_KERNELS}
    assert got == want, (case.gate, dict(names))
    bad = {k: f"{v:.2e}" for k, v in l2.items() if v > TRAIN_L2[dt]}
    assert not bad, bad
    if dt == "fp32":
        bad = {k: f"{v:.2e}" for k, v in elem.items() if v > TRAIN_ELEM_FP32}
        assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# (c) the causal cases, whole and streamed
# ------------------------------------------------------------------------------------------------------------------------
CAUSAL = [n for n, c in R.CASES.items() if c.causal and c.supports]


def _streams(case, dtype):
    """forward_streaming covers the layer: the row-group scan carries the state (fused.py:738, rows_mode)."""
    return case.dt_rank <= 16 or (case.dt_rank <= 32 and dtype == torch.bfloat16)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", CAUSAL)
def test_causal_whole_and_streamed(name, dt):
    from mamba_asr_amd import fused
    case, enc, x, ref = _case(name)
    dtype = DTYPES[dt]
    encg, xg = _on_gpu(enc), x.to(DEV)
    tol = R.INFER_TOL[dtype]
    with torch.no_grad():
        whole = fused.encoder_forward(encg, xg, dtype=dtype, streams=1)
        assert _ratio(whole, ref["out"], **tol) <= 1.0
        for chunk in (5, 14):
            ctx = encg.make_streaming_context(batch_size=x.shape[0], dtype=dtype)
            if not _streams(case, dtype):
                with pytest.raises(NotImplementedError, match="outside the streamed routes"):
                    encg.forward_streaming(xg[:, :chunk], ctx)
                continue
            outs = [encg.forward_streaming(xg[:, t0:t0 + chunk].contiguous(), ctx)[0] for t0 in range(0, x.shape[1], chunk)]
            r = _ratio(torch.cat(outs, dim=1), ref["out"], **tol)
            RATIOS[(f"stream{chunk}", name, dt)] = r
            print(f"{name} {dt} chunks of {chunk}: worst error / allowance {r:.3f}")
            assert r <= 1.0


def test_forward_streaming_refuses_what_it_documents():
    """A bidirectional encoder: ValueError (build it with causal=True).  A causal layer outside fused.supports (kernel_size 32):
    NotImplementedError.  Training mode or grad enabled: RuntimeError."""
    _, enc, x, _ = _case("expand2")
    encg = _on_gpu(enc)
    with pytest.raises(ValueError, match="bidirectional encoder cannot be streamed"):
        encg.make_streaming_context(batch_size=3)
    _, enc, x, _ = _case("k32_causal")
    encg, xg = _on_gpu(enc), x.to(DEV)
    ctx = encg.make_streaming_context(batch_size=3, dtype=torch.float32)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="outside the fused path"):
        encg.forward_streaming(xg[:, :5], ctx)
    _, enc, x, _ = _case("causal_expand1")
    encg, xg = _on_gpu(enc), x.to(DEV)
    ctx = encg.make_streaming_context(batch_size=3, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="inference path"):
        encg.forward_streaming(xg[:, :5], ctx)


# ------------------------------------------------------------------------------------------------------------------------
# (d) the kernels at the limits the gates allow: 65 rows (one 64-token tile and one row), fp64 on the kernel's own bf16 operands
# ------------------------------------------------------------------------------------------------------------------------
ROWS = 65
SENTINEL = -7.0


def _close(got, want, rtol, atol):
    torch.testing.assert_close(got.detach().double().cpu(), want.detach().double().cpu(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("K", [128, 256, 2048, 8192])
def test_mixer_tail_at_every_projection_width(K):
    """cm_ln_pw_glu_mix, out_proj K wide: test_mixer_tail_gpu.py's bound -- within 1.5 x the max abs error of the two-launch route
    (torch.mm + cm_ln_pw_glu) against fp64 with y not rounded.  K 128: one k-chunk; 8192: the entry point's last value (a layer
    with E = 4096 unfolded; the layer gates stop at 4096)."""
    from mamba_asr_amd import ops
    D = 256
    g = torch.Generator().manual_seed(K)
    r = lambda *s: torch.randn(*s, generator=g)
    x, ycat = r(ROWS, D), r(ROWS, K).bfloat16()
    wo, w = (r(D, K) * (K ** -0.5)).bfloat16(), (r(2 * D, D) * 0.05).bfloat16()
    bias, ln = r(2 * D) * 0.1, (1.0 + 0.1 * r(D), 0.1 * r(D), 1e-5)
    want_x = x.double() + ycat.double() @ wo.double().t()
    pw = torch.nn.functional.layer_norm(want_x, (D,), ln[0].double(), ln[1].double(), ln[2]) @ w.double().t() + bias.double()
    want_g = pw[:, :D] * torch.sigmoid(pw[:, D:])
    xd, yd, wod = x.to(DEV), ycat.to(DEV), wo.to(DEV)
    lnd, wp, bd = (ln[0].to(DEV), ln[1].to(DEV), ln[2]), ops.PackedWeight(w.to(DEV)), bias.to(DEV)
    xo_p, xo_m = torch.empty_like(xd), torch.empty_like(xd)
    g_p = ops.ln_pw_glu(xd, torch.mm(yd, wod.t()), 1.0, lnd, wp, bd, x_out=xo_p)
    g_m = ops.ln_pw_glu(xd, None, 1.0, lnd, wp, bd, x_out=xo_m, ycat=yd, out_w=ops.PackedWeight(wod))
    torch.cuda.synchronize()
    err = lambda t, want: float((t.double().cpu() - want).abs().max())
    e = dict(pair=(err(xo_p, want_x), err(g_p, want_g)), mix=(err(xo_m, want_x), err(g_m, want_g)))
    print(f"K {K}: max|err| vs fp64 x_out two launches {e['pair'][0]:.3e}, one kernel {e['mix'][0]:.3e}; gated {e['pair'][1]:.3e}, {e['mix'][1]:.3e}")
    assert bool(torch.isfinite(xo_m).all()) and bool(torch.isfinite(g_m.float()).all())
    assert e["mix"][0] <= 1.5 * e["pair"][0] and e["mix"][1] <= 1.5 * e["pair"][1]


def test_mixer_tail_refuses_the_first_width_past_its_limit():
    from mamba_asr_amd import ops
    D, K = 256, 8320
    x, ycat = torch.randn(ROWS, D, device=DEV), torch.randn(ROWS, K, device=DEV).bfloat16()
    wp, wo = ops.PackedWeight(torch.randn(2 * D, D, device=DEV).bfloat16()), ops.PackedWeight(torch.randn(D, K, device=DEV).bfloat16())
    xo, out = torch.full_like(x, SENTINEL), torch.full((ROWS, D), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.ln_pw_glu(x, None, 1.0, (torch.ones(D, device=DEV), torch.zeros(D, device=DEV), 1e-5), wp, torch.zeros(2 * D, device=DEV), x_out=xo,
                      ycat=ycat, out_w=wo, out=out)
    torch.cuda.synchronize()
    assert bool((xo == SENTINEL).all()) and bool((out == SENTINEL).all())


def _ffn_operands(hidden=1024):
    g = torch.Generator(device="cpu").manual_seed(hidden)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    x = rn(ROWS, 256, scale=2.0) + 0.5
    w1, b1 = rn(hidden, 256, scale=256 ** -0.5).bfloat16(), rn(hidden, scale=0.1)
    w2, b2 = rn(256, hidden, scale=hidden ** -0.5).bfloat16(), rn(256, scale=0.1)
    ln = lambda: (1.0 + 0.1 * rn(256), 0.1 * rn(256), 1e-5)
    return rn, x, w1, b1, w2, b2, ln(), ln()


@pytest.mark.parametrize("pdim", [256, 512, 4096])
@pytest.mark.parametrize("layout", [16, 32])
def test_ffn_fused_projection_at_every_width(pdim, layout):
    """cm_ffn_fused's projection epilogue at 2E = 256 (below any layer), 512 (expand 1) and 4096 (expand 8, the last value):
    test_hip_modules.py::test_ffn_fused_projection_epilogue's comparison and bound."""
    from mamba_asr_amd import ops
    rn, x, w1, b1, w2, b2, pre, n2 = _ffn_operands()
    wp, bp = rn(pdim, 256, scale=1 / 16).bfloat16(), rn(pdim, scale=0.1)
    xa, xb = x.clone(), x.clone()
    w1, w2 = ops.PackedWeight(w1, layout), ops.PackedWeight(w2, layout)
    _, h = ops.ffn_fused(xa, pre, w1, b1, w2, b2, alpha=0.5, norm2=n2)
    _, xz = ops.ffn_fused(xb, pre, w1, b1, w2, b2, alpha=0.5, norm2=n2, proj_w=ops.PackedWeight(wp, layout), proj_b=bp)
    assert torch.equal(xa, xb) and xz.shape == (ROWS, pdim) and xz.dtype == torch.bfloat16
    _close(xz.float(), h.double() @ wp.double().t() + bp.double(), rtol=8e-3, atol=8e-3)


def test_ffn_fused_refuses_the_first_widths_past_its_limits():
    """hidden 2304 (entry point, CM_EUNSUPPORTED) and a 4352-wide projection (the wrapper, before the native call): the residual
    rows and a sentinel-filled projection output stay as they were."""
    from mamba_asr_amd import ops
    rn, x, w1, b1, w2, b2, pre, n2 = _ffn_operands(2304)
    x0 = x.clone()
    h = torch.full((ROWS, 256), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.ffn_fused(x, pre, ops.PackedWeight(w1), b1, ops.PackedWeight(w2), b2, alpha=0.5, norm2=n2, h_out=h)
    torch.cuda.synchronize()
    assert torch.equal(x, x0) and bool((h == SENTINEL).all())         # the in-place residual rows and h are as they were
    rn, x, w1, b1, w2, b2, pre, n2 = _ffn_operands()
    out = torch.full((ROWS, 4352), SENTINEL, dtype=torch.bfloat16, device=DEV)
    x1 = x.clone()
    with pytest.raises(RuntimeError, match="up to 4096"):
        ops.ffn_fused(x, pre, w1, b1, w2, b2, alpha=0.5, norm2=n2, proj_w=ops.PackedWeight(rn(4352, 256).bfloat16()), proj_out=out)
    torch.cuda.synchronize()
    assert torch.equal(x, x1) and bool((out == SENTINEL).all())


def _conv_operands(e, rw, ndir):
    gen = torch.Generator().manual_seed(e + rw)
    xz = torch.randn(1, ROWS, 2 * e, generator=gen).bfloat16().to(DEV)
    w = [torch.randn(e, 4, generator=gen).to(DEV) * 0.5 for _ in range(ndir)]
    b = [torch.randn(e, generator=gen).to(DEV) * 0.1 for _ in range(ndir)]
    wx = [(torch.randn(rw, e, generator=gen) * 0.1).bfloat16().to(DEV) for _ in range(ndir)]
    return xz[:, :, :e], w, b, wx


@pytest.mark.parametrize("e,rw", [(32, 48), (32, 64), (2048, 48), (1248, 64), (2048, 64)])
def test_conv_xproj_at_the_narrowest_and_widest_mixer(e, rw):
    """cm_conv_xproj and cm_conv_xproj_uni at E = 32 (one 32-channel group) and at the last width of each row width: 2048 with 48-wide
    rows (expand 8), 1248 with 64-wide rows (16 < dt_rank <= 32: both directions' tile pair fills the 80 KiB, conv_xproj.hip:364).
    (2048, 64): cm_conv_xproj refuses and leaves its outputs alone -- the layer gates mirror it (ops.conv_xproj_supported) --
    while the one-direction kernel runs.  test_hip_ops.py::test_conv_xproj's comparisons and bounds: u bit-equal to cm_conv_cl_fwd's,
    itself within (1.6e-2, 1e-2) of the fp64 conv; x_dbl rows within (1.6e-2, 2e-2) of fp64 on the bf16 u and weights."""
    from mamba_asr_amd import ops
    from oracle import conmamba_oracle as O
    x, w, b, wx = _conv_operands(e, rw, 2)
    assert ops.conv_xproj_supported(e, rw - 32) == ((e, rw) != (2048, 64)) and ops.conv_xproj_supported(e, rw - 32, ndir=1)
    rf, rb = ops.conv_cl_fwd(x, w[0], b[0], w[1], b[1], True)
    if (e, rw) == (2048, 64):
        ucat = torch.full((1, ROWS, 2 * e), SENTINEL, dtype=torch.bfloat16, device=DEV)
        xdbl = torch.full((1, ROWS, 2 * rw), SENTINEL, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError, match="code -2.*too wide"):
            ops.conv_xproj(x, w[0], b[0], w[1], b[1], ops.PackedWeight(wx[0]), ops.PackedWeight(wx[1]), out_f=ucat[:, :, :e], out_b=ucat[:, :, e:], xdbl=xdbl)
        torch.cuda.synchronize()
        assert bool((ucat == SENTINEL).all()) and bool((xdbl == SENTINEL).all())
        xdbl = torch.cat([rf.float() @ wx[0].float().t(), rb.float() @ wx[1].float().t()], dim=-1)      # the route the gate falls back to
    else:
        ucat = torch.zeros(1, ROWS, 2 * e, dtype=torch.bfloat16, device=DEV)
        xdbl = ops.conv_xproj(x, w[0], b[0], w[1], b[1], ops.PackedWeight(wx[0]), ops.PackedWeight(wx[1]), out_f=ucat[:, :, :e], out_b=ucat[:, :, e:])
        assert torch.equal(ucat[:, :, :e], rf) and torch.equal(ucat[:, :, e:], rb)
    assert xdbl.shape == (1, ROWS, 2 * rw)
    xt = x.float().cpu().transpose(1, 2)
    _close(rf, O.causal_conv1d(xt, w[0].cpu(), b[0].cpu(), True, work_dtype=torch.float64).transpose(1, 2), 1.6e-2, 1e-2)
    _close(rb, O.causal_conv1d(xt.flip(-1), w[1].cpu(), b[1].cpu(), True, work_dtype=torch.float64).flip(-1).transpose(1, 2), 1.6e-2, 1e-2)
    for i, u in enumerate((rf, rb)):
        _close(xdbl[:, :, rw * i:rw * (i + 1)], u.double() @ wx[i].double().t(), 1.6e-2, 2e-2)
    # one direction, no carried rows
    u1 = torch.zeros(1, ROWS, e, dtype=torch.bfloat16, device=DEV)
    xd1 = ops.conv_xproj_uni(x, w[0], b[0], ops.PackedWeight(wx[0]), out=u1)
    assert torch.equal(u1, rf) and xd1.shape == (1, ROWS, rw)
    _close(xd1, rf.double() @ wx[0].double().t(), 1.6e-2, 2e-2)


def test_conv_xproj_refuses_the_first_width_past_its_limit():
    from mamba_asr_amd import ops
    e, rw = 2080, 48
    x, w, b, wx = _conv_operands(e, rw, 2)
    ucat = torch.full((1, ROWS, 2 * e), SENTINEL, dtype=torch.bfloat16, device=DEV)
    xdbl = torch.full((1, ROWS, 2 * rw), SENTINEL, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.conv_xproj(x, w[0], b[0], w[1], b[1], ops.PackedWeight(wx[0]), ops.PackedWeight(wx[1]), out_f=ucat[:, :, :e], out_b=ucat[:, :, e:], xdbl=xdbl)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.conv_xproj_uni(x, w[0], b[0], ops.PackedWeight(wx[0]), out=ucat[:, :, :e], xdbl=xdbl[:, :, :rw].contiguous())
    torch.cuda.synchronize()
    assert bool((ucat == SENTINEL).all()) and bool((xdbl == SENTINEL).all())


@pytest.mark.parametrize("e", [300, 68, 70])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_channel_mode_scan_off_the_vector_width(e, dt):
    """cm_scan_cl_fwd's state-split kernel at E = 300 (expand 1.5 at d_model 200), 68 and 70.  The loader's vector is 16 bytes: 8
    channels in bf16, 4 in fp32.  300 and 68 are multiples of 4 and not of 8, so they take the element path in bf16 only (in fp32
    they are whole vectors); 70 takes it in both dtypes.  Both directions in one launch:
    test_hip_ops.py::test_scan_channels_last_two_directions's comparison and bounds."""
    from mamba_asr_amd import ops
    from oracle import conmamba_oracle as O
    dtype = DTYPES[dt]
    b, l = 1, ROWS
    gen = torch.Generator().manual_seed(e)
    xz = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    z = xz[:, :, e:]
    dirs, refs = [], []
    ycat = torch.zeros(b, l, 2 * e, dtype=dtype, device=DEV)
    for i, rev in enumerate((False, True)):
        u = torch.randn(b, l, e, generator=gen).to(dtype)
        dl = (torch.randn(b, l, e, generator=gen) * 0.5).to(dtype)
        A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
        Bm, Cm = torch.randn(16, b, l, generator=gen), torch.randn(16, b, l, generator=gen)
        D, bias = torch.randn(e, generator=gen), torch.randn(e, generator=gen) - 1
        f = (lambda t: t.flip(-1)) if rev else (lambda t: t)
        tr = lambda t: t.float().transpose(1, 2)
        ref = O.selective_scan(f(tr(u)), f(tr(dl)), A, f(Bm.permute(1, 0, 2)), f(Cm.permute(1, 0, 2)), D, f(tr(z)), bias, True,
                               work_dtype=torch.float64)
        refs.append(f(ref).transpose(1, 2))
        gB, gC = ops.alloc_bc(16, b, l, DEV), ops.alloc_bc(16, b, l, DEV)
        gB.copy_(Bm), gC.copy_(Cm)
        dirs.append(dict(u=u.to(DEV), delta=dl.to(DEV), A=A.to(DEV), B=gB, C=gC, D=D.to(DEV), delta_bias=bias.to(DEV),
                         out=ycat[:, :, i * e:(i + 1) * e], reverse=rev))
    ops.scan_cl_fwd(dirs, z=xz.to(DEV)[:, :, e:], delta_softplus=True)
    tol = (2e-4, 5e-5) if dtype == torch.float32 else (1.6e-2, 1e-2)
    _close(ycat[:, :, :e], refs[0], *tol)
    _close(ycat[:, :, e:], refs[1], *tol)


def test_channel_mode_scan_refuses_a_17_row_dt_projection():
    """The in-kernel dt_proj of the state-split kernel stops at dt_rank 16 (fused._scan_dirs hands larger ranks over as a delta tensor)."""
    from mamba_asr_amd import ops
    b, l, e, rank = 1, ROWS, 64, 17
    feat = ops.alloc_bc(rank + 32, b, l, DEV)
    feat.copy_(torch.randn(rank + 32, b, l))
    out = torch.full((b, l, e), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="code -2"):
        ops.scan_cl_fwd([dict(u=torch.randn(b, l, e, device=DEV), A=-torch.ones(e, 16, device=DEV), B=feat[rank:rank + 16], C=feat[rank + 16:],
                              D=None, delta_bias=None, dt_low=feat[:rank], dt_weight=torch.randn(e, rank, device=DEV), out=out)])
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_add_layernorm_at_its_last_width_and_past_it():
    """cm_add_layernorm at 1024 columns (test_row_kernels_fp64.py's fp32 bound: rtol 2e-3, atol 2e-4 x max(1, max|ref|)); 1032 raises
    and leaves x_out and out alone."""
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(1024)
    for dim in (1024, 1032):
        x, y = torch.randn(ROWS, dim, generator=g) * 1.5 + 0.3, (torch.randn(ROWS, dim, generator=g) * 2.0).bfloat16()
        n2 = (1.0 + 0.3 * torch.randn(dim, generator=g), 0.2 * torch.randn(dim, generator=g), 1e-5)
        xo = torch.full((ROWS, dim), SENTINEL, device=DEV)
        out = torch.full((ROWS, dim), SENTINEL, device=DEV)
        call = lambda: ops.add_layernorm(x.to(DEV), y.to(DEV), 0.5, norm2=(n2[0].to(DEV), n2[1].to(DEV), n2[2]), x_out=xo, out_dtype=torch.float32, out=out)
        if dim > 1024:
            with pytest.raises(RuntimeError, match="code -2"):
                call()
            torch.cuda.synchronize()
            assert bool((xo == SENTINEL).all()) and bool((out == SENTINEL).all())
            continue
        call()
        r = x.double() + 0.5 * y.double()
        want = torch.nn.functional.layer_norm(r, (dim,), n2[0].double(), n2[1].double(), n2[2])
        _close(xo, r, 2e-3, 2e-4 * max(1.0, float(r.abs().max())))
        _close(out, want, 2e-3, 2e-4 * max(1.0, float(want.abs().max())))


def test_zz_print_worst_ratios():
    """Per section, case and dtype: the worst error / allowance of (a), (b) and (c) -- the table of the module docstring.  Nothing
    is asserted against these numbers."""
    for (section, name, dt), r in sorted(RATIOS.items()):
        print(f"RATIO {section:9s} {name:18s} {dt}  {r:.3f}")
