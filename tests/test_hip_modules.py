"""GPU parity of the module / operator API (mamba_asr_amd.modules.*) against golden vectors produced by the
reference's own classes (tests/golden/make_golden.py): BiMamba-v2 mixer, fused inner op, ConmambaEncoderLayer,
2-layer ConmambaEncoder, MambaDecoderLayer — forward and gradients, fp32.  Tolerance: rtol 2e-3 / atol 2e-4
(fp32 kernels with v_exp/v_log/v_rcp approximations + rocBLAS GEMMs vs torch-CPU fp32)."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}


def close(a, b, rtol=2e-3, atol=2e-4):
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol * scale)


def _params(g, prefix):
    return {k[len(prefix):]: v for k, v in g.items() if k.startswith(prefix)}


def test_bimamba_v2_forward_backward(golden):
    from mamba_asr_amd.modules.mamba.bimamba import Mamba
    g = golden("g3_bimamba")
    m = Mamba(144, d_state=16, d_conv=4, expand=2, bimamba_type="v2")
    m.load_state_dict(_params(g, "d144_p."), strict=True)
    m = m.to(DEV)
    x = g["d144_x"].to(DEV).requires_grad_(True)
    y = m(x)
    close(y, g["d144_y"])
    names = [k for k, _ in m.named_parameters()]
    grads = torch.autograd.grad(y, [x] + [p for _, p in m.named_parameters()], g["d144_dy"].to(DEV))
    close(grads[0], g["d144_dx"])
    for k, gk in zip(names, grads[1:]):
        close(gk, g[f"d144_g.{k}"], rtol=3e-3, atol=3e-4)
    # no-grad path: two-stream issue of the directions gives the same numbers
    with torch.no_grad():
        close(m(g["d144_x"].to(DEV)), g["d144_y"])


def test_inner_fn_no_out_proj(golden):
    from mamba_asr_amd.modules.mamba.selective_scan_interface import mamba_inner_fn_no_out_proj
    g = golden("g3_bimamba")
    p = {k: v.to(DEV) for k, v in _params(g, "d144_p.").items()}
    xz = g["d144_inner_xz"].to(DEV).requires_grad_(True)
    A = -torch.exp(p["A_log"].float())
    oz = mamba_inner_fn_no_out_proj(xz, p["conv1d.weight"], p["conv1d.bias"], p["x_proj.weight"], p["dt_proj.weight"],
                                    A, None, None, p["D"].float(), delta_bias=p["dt_proj.bias"].float(),
                                    delta_softplus=True)
    close(oz, g["d144_inner_out"])
    (dxz,) = torch.autograd.grad(oz, xz, g["d144_inner_dout"].to(DEV))
    close(dxz, g["d144_inner_dxz"])
    # reverse_time == flip . op . flip (what the reference does with copies, bimamba.py:237,253)
    oz_r = mamba_inner_fn_no_out_proj(xz.detach().flip(-1).contiguous(), p["conv1d.weight"], p["conv1d.bias"],
                                      p["x_proj.weight"], p["dt_proj.weight"], A, None, None, p["D"].float(),
                                      delta_bias=p["dt_proj.bias"].float(), delta_softplus=True, reverse_time=True)
    close(oz_r.flip(-1), g["d144_inner_out"])


def _encoder(g):
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    enc = ConmambaEncoder(num_layers=2, d_model=80, d_ffn=192, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG))
    enc.load_state_dict(_params(g, "p."), strict=True)
    return enc.to(DEV)


def test_encoder_layer_and_stack(golden):
    g = golden("g4_encoder")
    enc = _encoder(g).eval()
    x = g["x"].to(DEV)
    with torch.no_grad():
        close(enc.layers[0](x), g["y_layer0"])
        out, second = enc(x)
        assert second is None
        close(out, g["y_enc"])


def test_encoder_layer_gradients(golden):
    g = golden("g4_encoder")
    enc = _encoder(g).train()          # dropout p = 0
    x = g["x"].to(DEV).requires_grad_(True)
    y = enc.layers[0](x)
    named = list(enc.layers[0].named_parameters())
    grads = torch.autograd.grad(y, [x] + [p for _, p in named], g["dy_layer0"].to(DEV))
    close(grads[0], g["dx_layer0"], rtol=3e-3, atol=3e-4)
    for (k, _), gk in zip(named, grads[1:]):
        close(gk, g["g.layers.0." + k], rtol=5e-3, atol=5e-4)


def test_decoder_layer(golden):
    from mamba_asr_amd.modules.Conmamba import MambaDecoderLayer
    g = golden("g4_decoder_layer")
    dec = MambaDecoderLayer(d_model=64, d_ffn=128, activation=nn.ReLU, dropout=0.0, normalize_before=True,
                            mamba_config=dict(CFG))
    dec.load_state_dict(_params(g, "p."), strict=True)
    dec = dec.to(DEV).eval()
    with torch.no_grad():
        out, a, b = dec(g["tgt"].to(DEV), g["memory"].to(DEV))
    assert a is None and b is None
    close(out, g["out"])


def test_shared_mamba_config_is_restored():
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoderLayer
    cfg = dict(CFG)
    ConmambaEncoderLayer(32, 64, mamba_config=cfg)
    assert cfg == CFG                              # 'bidirectional' popped and restored (reference Conmamba.py:579-591)


def test_bf16_autocast_encoder_close_to_fp32(golden):
    g = golden("g4_encoder")
    enc = _encoder(g).eval()
    x = g["x"].to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out, _ = enc(x)
    # bf16 tolerance stated in SURVEY §8d: rtol 3e-2 / atol 5e-2 on encoder output
    torch.testing.assert_close(out.float().cpu(), g["y_enc"], rtol=3e-2, atol=5e-2)


def test_fused_encoder_matches_reference_golden(golden):
    """The fused channels-last inference path (mamba_asr_amd.fused) against the reference's 2-layer encoder."""
    from mamba_asr_amd import fused
    g = golden("g4_encoder")
    enc = _encoder(g).eval()
    x = g["x"].to(DEV)
    with torch.no_grad():
        out = fused.encoder_forward(enc, x, dtype=torch.float32)
        close(out, g["y_enc"])
        out2, _ = enc(x)                      # module entry point dispatches to the fused path in eval/no-grad
        close(out2, g["y_enc"])
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out3, _ = enc(x)
    torch.testing.assert_close(out3.float().cpu(), g["y_enc"], rtol=3e-2, atol=5e-2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_channels_last_elementwise_ops(dtype):
    from mamba_asr_amd import ops
    from oracle import conmamba_oracle as O
    gen = torch.Generator().manual_seed(11)
    b, l, e = 2, 70, 96
    tol = dict(rtol=1e-4, atol=1e-4) if dtype == torch.float32 else dict(rtol=2e-2, atol=2e-2)
    # conv, both directions
    x = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    wf, bf_, wb, bb = (torch.randn(e, 4, generator=gen), torch.randn(e, generator=gen), torch.randn(e, 4, generator=gen),
                       torch.randn(e, generator=gen))
    yf, yb = ops.conv_cl_fwd(x.to(DEV)[:, :, :e], wf.to(DEV), bf_.to(DEV), wb.to(DEV), bb.to(DEV))
    xt = x[:, :, :e].float().transpose(1, 2)
    rf = O.causal_conv1d(xt, wf, bf_, True, work_dtype=torch.float64).transpose(1, 2)
    rb = O.causal_conv1d(xt.flip(-1), wb, bb, True, work_dtype=torch.float64).flip(-1).transpose(1, 2)
    torch.testing.assert_close(yf.float().cpu(), rf.float(), **tol)
    torch.testing.assert_close(yb.float().cpu(), rb.float(), **tol)
    # add + two LayerNorms
    d = 144
    xr = torch.randn(5, 7, d, generator=gen)
    y = torch.randn(5, 7, d, generator=gen).to(dtype)
    g1, b1, g2, b2 = (torch.randn(d, generator=gen) for _ in range(4))
    xo = torch.empty_like(xr).to(DEV)
    _, out = ops.add_layernorm(xr.to(DEV), y.to(DEV), 0.5, norm1=(g1.to(DEV), b1.to(DEV), 1e-5),
                               norm2=(g2.to(DEV), b2.to(DEV), 1e-6), x_out=xo, out_dtype=dtype)
    r1 = torch.nn.functional.layer_norm(xr + 0.5 * y.float(), (d,), g1, b1, 1e-5)
    r2 = torch.nn.functional.layer_norm(r1, (d,), g2, b2, 1e-6)
    torch.testing.assert_close(xo.cpu(), r1, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.float().cpu(), r2, **tol)
    # GLU -> depthwise conv 31 -> LN -> GELU
    dd = 80
    inp = torch.randn(2, 45, 2 * dd, generator=gen).to(dtype)
    w, bs = torch.randn(dd, 1, 31, generator=gen) * 0.2, torch.randn(dd, generator=gen)
    lg, lb = torch.randn(dd, generator=gen), torch.randn(dd, generator=gen)
    got = ops.glu_dwconv_ln_gelu(inp.to(DEV), w.to(DEV), bs.to(DEV), lg.to(DEV), lb.to(DEV), 1e-5)
    ref = torch.nn.functional.glu(inp.float().transpose(1, 2), dim=1)
    ref = torch.nn.functional.conv1d(ref, w, bs, padding=15, groups=dd).transpose(1, 2)
    ref = torch.nn.functional.gelu(torch.nn.functional.layer_norm(ref, (dd,), lg, lb, 1e-5))
    torch.testing.assert_close(got.float().cpu(), ref, **tol)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fused_frontend_and_encoder_match_unfused_and_oracle(dtype):
    """ConMambaASR.encode: native inference path == module-by-module path == CPU oracle (fp32)."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs, samples_for_frames
    from oracle import conmamba_oracle as O
    cfg = ASRConfig("tiny", d_model=64, d_ffn=128, num_encoder_layers=2, n_fft=400, seed=5)
    model = ConMambaASR(cfg).to(DEV).eval()
    wavs, lens = synthetic_wavs(2, samples_for_frames(203), 9, DEV)
    with torch.no_grad():
        model.calibrate(wavs, lens)                                         # fills the normaliser statistics
        feats = model.features(wavs, lens)
        ref = model.Transformer.encode(model.CNN(feats), lens)               # module path (fp32)
        got = fused.asr_encode(model, wavs, lens, dtype=dtype)
    assert got.shape == ref.shape == (2, 51, 64)
    if dtype == torch.float32:
        close(got, ref, rtol=2e-3, atol=2e-4)
        p = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
        want = O.asr_encode(p, wavs.cpu(), lens.cpu(), 2, p["normalize.glob_mean"], p["normalize.glob_std"], n_fft=400)
        close(got, want, rtol=5e-3, atol=1e-3)
    else:
        torch.testing.assert_close(got.cpu(), ref.cpu(), rtol=3e-2, atol=5e-2)


@pytest.mark.parametrize("rows,hidden,addend,n1,n2,hdt", [
    (64, 256, False, False, True, torch.bfloat16),
    (1000, 1024, False, False, True, torch.bfloat16),      # ragged last tile, FFN 1 of a layer (h = norm1)
    (333, 1024, True, True, False, None),                  # FFN 2 of a layer: addend, closing norm2, no h
    (130, 512, True, True, True, torch.float32),           # last layer: + the encoder's final norm, fp32 out
])
@pytest.mark.parametrize("layout", [16, 32, -32])             # -32: layout 32 with 32-token workgroups
def test_ffn_fused_kernel(rows, hidden, addend, n1, n2, hdt, layout):
    """cm_ffn_fused vs an fp32 restatement with the kernel's rounding points (bf16 GEMM operands, fp32 accumulate); both matrix
    instructions (layout 16: 16x16x32 tiles, csrc/ffn_fused.hip; 32: 32x32x16, csrc/ffn_fused32.hip)."""
    from mamba_asr_amd import ops
    g = torch.Generator(device="cpu").manual_seed(rows + hidden)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    x = rn(rows, 256, scale=2.0) + 0.5
    add = rn(rows, 256).bfloat16() if addend else None
    w1, b1 = rn(hidden, 256, scale=256 ** -0.5).bfloat16(), rn(hidden, scale=0.1)
    w2, b2 = rn(256, hidden, scale=hidden ** -0.5).bfloat16(), rn(256, scale=0.1)
    ln = lambda: (1.0 + 0.1 * rn(256), 0.1 * rn(256), 1e-5)
    pre, nn1, nn2 = ln(), (ln() if n1 else None), (ln() if n2 else None)
    # reference
    xin = x + (0.7 * add.float() if addend else 0.0)
    LN = lambda t, p_: torch.nn.functional.layer_norm(t, (256,), p_[0], p_[1], p_[2])
    hn = LN(xin, pre).bfloat16().float()
    hid = torch.nn.functional.gelu(hn @ w1.float().t() + b1).bfloat16().float()
    r = xin + 0.5 * (hid @ w2.float().t() + b2)
    if n1:
        r = LN(r, nn1)
    want_h = None if hdt is None else (LN(r, nn2) if n2 else r)
    # kernel
    d = lambda t: None if t is None else t.to(DEV)
    dn = lambda p_: None if p_ is None else (p_[0].to(DEV), p_[1].to(DEV), p_[2])
    xg = x.to(DEV)
    tokens = {16: None, 32: 64, -32: 32}[layout]
    layout = abs(layout)
    xo, h = ops.ffn_fused(xg, dn(pre), ops.PackedWeight(d(w1), layout), d(b1), ops.PackedWeight(d(w2), layout), d(b2), alpha=0.5, addend=d(add), add_scale=0.7, norm1=dn(nn1),
                          norm2=dn(nn2), want_h=hdt is not None, h_dtype=hdt or torch.bfloat16, tokens=tokens)
    assert xo.data_ptr() == xg.data_ptr()
    torch.testing.assert_close(xo.cpu(), r, rtol=2e-3, atol=4e-3)
    assert (xo.cpu() - r).abs().mean() < 3e-4
    if hdt is not None:
        assert h.dtype == hdt
        tol = dict(rtol=2e-3, atol=4e-3) if hdt == torch.float32 else dict(rtol=1e-2, atol=2e-2)
        torch.testing.assert_close(h.float().cpu(), want_h, **tol)


@pytest.mark.parametrize("rows,pdim,bias", [(64, 1024, False), (1000, 1024, True), (37, 256, False), (200, 2048, True)])
@pytest.mark.parametrize("layout", [16, 32, -32])
def test_ffn_fused_projection_epilogue(rows, pdim, bias, layout):
    """cm_ffn_fused with proj_w: the Linear that consumes h (the BiMamba in_proj, reference bimamba.py:192-200) inside the
    kernel == the kernel's own bf16 h through an fp32 matmul with the same bf16 weight; the stream output is unchanged."""
    from mamba_asr_amd import ops
    g = torch.Generator(device="cpu").manual_seed(rows + pdim)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    x = rn(rows, 256, scale=2.0) + 0.5
    w1, b1 = rn(1024, 256, scale=256 ** -0.5).bfloat16(), rn(1024, scale=0.1)
    w2, b2 = rn(256, 1024, scale=1024 ** -0.5).bfloat16(), rn(256, scale=0.1)
    ln = lambda: (1.0 + 0.1 * rn(256), 0.1 * rn(256), 1e-5)
    pre, n2 = ln(), ln()
    wp, bp = rn(pdim, 256, scale=1 / 16).bfloat16(), (rn(pdim, scale=0.1) if bias else None)
    xa, xb = x.clone(), x.clone()
    tokens = {16: None, 32: 64, -32: 32}[layout]
    layout = abs(layout)
    w1, w2 = ops.PackedWeight(w1, layout), ops.PackedWeight(w2, layout)
    _, h = ops.ffn_fused(xa, pre, w1, b1, w2, b2, alpha=0.5, norm2=n2, tokens=tokens)
    _, xz = ops.ffn_fused(xb, pre, w1, b1, w2, b2, alpha=0.5, norm2=n2, proj_w=ops.PackedWeight(wp, layout), proj_b=bp, tokens=tokens)
    assert torch.equal(xa, xb) and xz.shape == (rows, pdim) and xz.dtype == torch.bfloat16
    want = h.float() @ wp.float().t() + (bp if bias else 0.0)
    torch.testing.assert_close(xz.float(), want, rtol=8e-3, atol=8e-3)
    out = torch.empty(rows, pdim, dtype=torch.bfloat16, device=DEV)
    _, xz2 = ops.ffn_fused(x.clone(), pre, w1, b1, w2, b2, alpha=0.5, norm2=n2, proj_w=ops.PackedWeight(wp, layout), proj_b=bp, proj_out=out, tokens=tokens)
    assert xz2.data_ptr() == out.data_ptr() and torch.equal(out, xz)


@pytest.mark.parametrize("batch,seqlen", [(2, 100), (3, 37), (1, 1000)])
def test_ln_pw_glu_kernel_and_pregated_dwconv(batch, seqlen):
    """cm_ln_pw_glu (residual add + LayerNorm + pointwise conv + GLU) vs torch fp32 on the same bf16-rounded operands,
    and cm_glu_dwconv_ln_gelu fed with its D-wide gated output (glu_done) vs the same kernel fed the 2D-wide tensor."""
    from mamba_asr_amd import ops
    F = torch.nn.functional
    g = torch.Generator(device="cpu").manual_seed(seqlen)
    rows, D = batch * seqlen, 256
    x = torch.randn(rows, D, generator=g)
    y = (torch.randn(rows, D, generator=g) * 0.5).bfloat16()
    ln = (1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g), 1e-5)
    w = (torch.randn(2 * D, D, generator=g) / 16).bfloat16()
    bias = torch.randn(2 * D, generator=g) * 0.1
    r = x + y.float()
    h = F.layer_norm(r, (D,), ln[0], ln[1], ln[2]).bfloat16().float()
    pw = h @ w.float().t() + bias
    want = pw[:, :D] * torch.sigmoid(pw[:, D:])
    xg = x.to(DEV)
    got = ops.ln_pw_glu(xg, y.to(DEV), 1.0, (ln[0].to(DEV), ln[1].to(DEV), ln[2]), ops.PackedWeight(w.to(DEV)), bias.to(DEV))
    torch.testing.assert_close(xg.cpu(), r, rtol=1e-6, atol=1e-6)                  # residual stream updated in place
    torch.testing.assert_close(got.float().cpu(), want, rtol=1.6e-2, atol=1e-2)
    assert (got.float().cpu() - want).abs().mean() < 1e-3
    # depthwise stage: pre-gated input == 2D-wide input whose GLU reproduces it
    dw_w, dw_b = torch.randn(D, 31, generator=g) / 6, torch.randn(D, generator=g) * 0.1
    ln2 = (1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g))
    gl = got.view(batch, seqlen, D)
    wide = torch.cat([gl.float(), torch.full_like(gl, 40.0, dtype=torch.float32)], dim=-1).bfloat16()       # sigmoid(40) == 1
    a = ops.glu_dwconv_ln_gelu(gl, dw_w.to(DEV), dw_b.to(DEV), ln2[0].to(DEV), ln2[1].to(DEV), 1e-5, glu_done=True)
    b_ = ops.glu_dwconv_ln_gelu(wide, dw_w.to(DEV), dw_b.to(DEV), ln2[0].to(DEV), ln2[1].to(DEV), 1e-5)
    assert torch.equal(a, b_)
    ref = F.conv1d(gl.float().cpu().transpose(1, 2), dw_w[:, None], dw_b, padding=15, groups=D).transpose(1, 2)
    ref = F.gelu(F.layer_norm(ref, (D,), ln2[0], ln2[1], 1e-5))
    torch.testing.assert_close(a.float().cpu(), ref, rtol=1.6e-2, atol=1e-2)


@pytest.mark.parametrize("D", [256, 512])
@pytest.mark.parametrize("batch,seqlen", [(2, 100), (3, 37), (1, 1000), (2, 31), (1, 1)])
def test_dwconv_rows_kernel(D, batch, seqlen):
    """cm_glu_dwconv_ln_gelu's 32-step row kernel (bf16, dim 256 / 512; csrc/elementwise_cl.hip dwconv_rows_kernel): GLU ->
    depthwise conv 31 ('same') -> LayerNorm -> GELU (reference Conmamba.py:120-160) vs torch fp32 on the same bf16 inputs,
    with and without the transposed tap copy, pre-gated and not, and against the 16-step kernel it replaces."""
    from mamba_asr_amd import ops, _native
    F = torch.nn.functional
    g = torch.Generator(device="cpu").manual_seed(seqlen + D)
    inp = torch.randn(batch, seqlen, 2 * D, generator=g).bfloat16()
    w, bs = torch.randn(D, 31, generator=g) / 6, torch.randn(D, generator=g) * 0.1
    lg, lb = 1.0 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    gated = (inp[..., :D].float() * torch.sigmoid(inp[..., D:].float())).bfloat16()
    ref = F.conv1d(gated.float().transpose(1, 2), w[:, None], bs, padding=15, groups=D).transpose(1, 2)
    ref = F.gelu(F.layer_norm(ref, (D,), lg, lb, 1e-5))
    dev = lambda t: t.to(DEV)
    wt = w.t().contiguous()
    a = ops.glu_dwconv_ln_gelu(dev(inp), dev(w), dev(bs), dev(lg), dev(lb), 1e-5)
    b_ = ops.glu_dwconv_ln_gelu(dev(inp), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, weight_t=dev(wt))
    c = ops.glu_dwconv_ln_gelu(dev(gated), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, weight_t=dev(wt), glu_done=True)
    assert torch.equal(a, b_)
    torch.testing.assert_close(a.float().cpu(), ref, rtol=1.6e-2, atol=1e-2)
    torch.testing.assert_close(c.float().cpu(), ref, rtol=1.6e-2, atol=1e-2)
    assert (c.float().cpu() - ref).abs().mean() < 1.5e-3
    old = ops.glu_dwconv_ln_gelu(dev(gated), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, weight_t=dev(wt), glu_done=True,
                                 variant=1)                   # the 16-step kernel
    torch.testing.assert_close(c.float(), old.float(), rtol=8e-3, atol=2e-3)       # fp32 sums in a different order, one bf16 rounding
    # the module's closing Linear in the same kernel (dim 256) == the kernel's bf16 activations through a fp32 matmul
    lw, lbias = (torch.randn(D, D, generator=g) / 16).bfloat16(), torch.randn(D, generator=g) * 0.1
    if D == 256:
        y = ops.glu_dwconv_ln_gelu(dev(gated), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, weight_t=dev(wt), glu_done=True,
                                   lin_w=ops.PackedWeight(dev(lw)), lin_b=dev(lbias))
        want = c.float().cpu() @ lw.float().t() + lbias
        torch.testing.assert_close(y.float().cpu(), want, rtol=8e-3, atol=4e-3)
        y2 = ops.glu_dwconv_ln_gelu(dev(inp), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, lin_w=ops.PackedWeight(dev(lw)), lin_b=dev(lbias))
        assert torch.equal(y, y2)
    else:
        with pytest.raises(RuntimeError, match="dim 256"):
            ops.glu_dwconv_ln_gelu(dev(gated), dev(w), dev(bs), dev(lg), dev(lb), 1e-5, glu_done=True,
                                   lin_w=ops.PackedWeight(dev(lw)), lin_b=dev(lbias))


@pytest.mark.parametrize("batch,frames", [(2, 401), (3, 130), (1, 4001), (2, 37), (70, 64)])
def test_cnn_front_kernel(batch, frames):
    """cm_cnn_front (both CNN blocks, intermediate kept in LDS) against (a) a torch fp32 restatement of
    ConvolutionFrontEnd (reflect 'same' padding, stride 2, LayerNorm over (freq, channel), LeakyReLU) with the block-1
    output rounded to bf16 where the kernel rounds it, and (b) the two-kernel path cm_cnn_block1 + cm_cnn_block2.
    Ragged step counts (last tile partial, chunk boundaries), many one-chunk utterances (batch 70: 70 chunks on 70 workgroups; the
    persistent loop's second trip, more chunks than the 256 workgroups, is tests/test_front_end_edges.py's)."""
    from mamba_asr_amd import ops
    F = torch.nn.functional
    g = torch.Generator(device="cpu").manual_seed(batch * 1000 + frames)
    feats = torch.randn(batch, frames, 80, generator=g)
    w1, b1 = torch.randn(64, 1, 3, 3, generator=g) / 3, torch.randn(64, generator=g) * 0.1
    g1, be1 = 1.0 + 0.1 * torch.randn(40, 64, generator=g), 0.1 * torch.randn(40, 64, generator=g)
    w2 = (torch.randn(32, 64, 3, 3, generator=g) * (64 * 9) ** -0.5).bfloat16()
    b2 = torch.randn(32, generator=g) * 0.1
    g2, be2 = 1.0 + 0.1 * torch.randn(20, 32, generator=g), 0.1 * torch.randn(20, 32, generator=g)
    # torch restatement
    x = F.pad(feats[:, None], (1, 1, 1, 1), mode="reflect")
    y = F.conv2d(x, w1, b1, stride=2).permute(0, 2, 3, 1)                                   # (B, T1, 40, 64)
    y = F.leaky_relu(F.layer_norm(y, (40, 64), g1, be1, 1e-5), 0.01).bfloat16().float()
    y = F.pad(y.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="reflect")
    z = F.conv2d(y, w2.float(), b2, stride=2).permute(0, 2, 3, 1)                           # (B, T2, 20, 32)
    t2 = z.shape[1]
    ref = F.leaky_relu(F.layer_norm(z.reshape(batch, t2, 640), (640,), g2.reshape(-1), be2.reshape(-1), 1e-5), 0.01)
    d = lambda t: t.to(DEV)
    w2o = w2.permute(0, 2, 3, 1).contiguous()
    got = ops.cnn_front(d(feats), d(w1), d(b1), d(g1), d(be1), 1e-5, d(w2o), d(b2), d(g2), d(be2), 1e-5, 0.01)
    assert got.shape == (batch, t2, 640) and got.dtype == torch.bfloat16
    torch.testing.assert_close(got.float().cpu(), ref, rtol=1.6e-2, atol=2e-2)
    assert (got.float().cpu() - ref).abs().mean() < 2e-3
    y1 = ops.cnn_block1(d(feats), d(w1), d(b1), d(g1), d(be1), 1e-5, 0.01, out_dtype=torch.bfloat16, pad_out=1)
    two = ops.cnn_block2(y1, d(w2o), d(b2), d(g2), d(be2), 1e-5, 0.01)
    torch.testing.assert_close(got.float(), two.float(), rtol=1.6e-2, atol=2e-2)
    assert (got.float() - two.float()).abs().mean() < 1e-3


@pytest.mark.parametrize("batch,t_in,f_in", [(2, 42, 42), (3, 37, 42), (1, 9, 22), (2, 11, 9)])
def test_cnn_block2_kernel(batch, t_in, f_in):
    """cm_cnn_block2 (implicit-GEMM conv 64->32 3x3 s2 + LayerNorm + LeakyReLU) vs torch conv2d/layer_norm in fp32 on the
    same bf16-rounded operands; ragged last tiles and frequency widths that do not fill a 16-position MFMA tile."""
    from mamba_asr_amd import ops
    g = torch.Generator(device="cpu").manual_seed(batch * 100 + t_in)
    y1 = torch.randn(batch, t_in, f_in, 64, generator=g).bfloat16()
    w = (torch.randn(32, 64, 3, 3, generator=g) * (64 * 9) ** -0.5).bfloat16()
    bias = torch.randn(32, generator=g) * 0.1
    t2, f2 = (t_in - 3) // 2 + 1, (f_in - 3) // 2 + 1
    ln_g, ln_b = 1.0 + 0.1 * torch.randn(f2, 32, generator=g), 0.1 * torch.randn(f2, 32, generator=g)
    ref = torch.nn.functional.conv2d(y1.float().permute(0, 3, 1, 2), w.float(), bias, stride=2).permute(0, 2, 3, 1)
    ref = torch.nn.functional.layer_norm(ref.reshape(batch, t2, f2 * 32), (f2 * 32,), ln_g.reshape(-1), ln_b.reshape(-1), 1e-5)
    ref = torch.nn.functional.leaky_relu(ref, 0.01)
    got = ops.cnn_block2(y1.to(DEV), w.permute(0, 2, 3, 1).contiguous().to(DEV), bias.to(DEV), ln_g.to(DEV), ln_b.to(DEV), 1e-5, 0.01)
    assert got.shape == (batch, t2, f2 * 32) and got.dtype == torch.bfloat16
    torch.testing.assert_close(got.float().cpu(), ref, rtol=1e-2, atol=1e-2)
    assert (got.float().cpu() - ref).abs().mean() < 2e-3


def test_layernorm_low_out_is_bit_identical_under_autocast(monkeypatch):
    """The encoder layer's projection-feeding LayerNorms store the autocast dtype themselves (RowsLayerNorm.low_out): the
    GEMMs see the same bf16 operands as with torch's fp32 LayerNorm output + cast, so the layer's forward output and its
    gradients are bit-identical with the switch off."""
    from mamba_asr_amd import sb_compat
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoderLayer
    torch.manual_seed(9)
    layer = ConmambaEncoderLayer(d_model=256, d_ffn=512, kernel_size=31, activation=nn.GELU, bias=True, dropout=0.0,
                                 causal=False, mamba_config=dict(CFG)).to(DEV).train()
    assert layer.norm1.norm.low_out and layer.ffn_module1[0].low_out and not layer.norm2.norm.low_out
    x0 = torch.randn(2, 50, 256, device=DEV)
    res = []
    for flag in (False, True):
        monkeypatch.setattr(sb_compat, "LN_LOW_OUT", flag)
        x = x0.clone().requires_grad_(True)
        layer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = layer(x)
        y.float().square().mean().backward()
        res.append((y.detach().clone(), x.grad.clone(), layer.ffn_module1[0].weight.grad.clone(), layer.norm1.norm.bias.grad.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_ffn_fused_rejects_unsupported():
    from mamba_asr_amd import ops
    x = torch.zeros(8, 128, device=DEV)
    w1 = torch.zeros(256, 128, device=DEV, dtype=torch.bfloat16)
    w2 = torch.zeros(128, 256, device=DEV, dtype=torch.bfloat16)
    v = lambda n: torch.zeros(n, device=DEV)
    with pytest.raises(RuntimeError, match="d_model must be 256"):
        ops.ffn_fused(x, (v(128), v(128), 1e-5), w1, v(256), w2, v(128))


def test_fused_ffn_layer_path_matches_library_path(monkeypatch):
    """Encoder forward with the feed-forward modules on cm_ffn_fused == the library-GEMM fused path and the fp32 path."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(5)
    enc = ConmambaEncoder(num_layers=3, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    x = torch.randn(3, 90, 256, device=DEV)
    with torch.no_grad():
        monkeypatch.setattr(fused, "USE_FUSED_FFN", False)
        ref = fused.encoder_forward(enc, x, dtype=torch.bfloat16)
        ref32 = fused.encoder_forward(enc, x, dtype=torch.float32)
        monkeypatch.setattr(fused, "USE_FUSED_FFN", True)
        got = fused.encoder_forward(enc, x, dtype=torch.bfloat16)
    torch.testing.assert_close(got.cpu(), ref32.cpu(), rtol=3e-2, atol=5e-2)
    torch.testing.assert_close(got.cpu(), ref.cpu(), rtol=3e-2, atol=5e-2)
    # the fused path rounds less (no bf16 FFN output): it must not be further from fp32 than the library path
    assert (got - ref32).abs().mean() <= 1.2 * (ref - ref32).abs().mean()


@pytest.mark.parametrize("mode", ["join", "pair", "free"])
def test_multi_stream_encoder_matches_single_stream(monkeypatch, mode):
    """CM_STREAMS=3: the batch as three parts on three HIP streams ('join': scan once per layer on the whole batch
    between a join and a fork; 'pair': a scan per part, one at a time; 'free': independent parts) gives exactly the
    single-stream result (utterances are
    independent through the encoder; every kernel is deterministic), eagerly and under hipGraph capture."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(11)
    enc = ConmambaEncoder(num_layers=3, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    x = torch.randn(17, 75, 256, device=DEV)                   # 17 utterances: uneven parts (6, 5, 6)
    monkeypatch.setattr(fused, "STREAM_MODE", mode)
    with torch.no_grad():
        ref = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=1)
        got = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=3)
        torch.cuda.synchronize()
        assert torch.equal(got, ref)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=3)          # warm-up outside capture
        torch.cuda.current_stream().wait_stream(side)
        with torch.cuda.graph(graph):
            out = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=3)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)


def test_native_gemm_layer_path_matches_library_path(monkeypatch):
    """Encoder forward with every projection on cm_gemm_bf16 (fused epilogues) == the library-GEMM fused path."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(3)
    enc = ConmambaEncoder(num_layers=2, d_model=256, d_ffn=512, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    x = torch.randn(2, 70, 256, device=DEV)
    with torch.no_grad():
        monkeypatch.setattr(fused, "USE_NATIVE_GEMM", False)
        ref = fused.encoder_forward(enc, x, dtype=torch.bfloat16)
        ref32 = fused.encoder_forward(enc, x, dtype=torch.float32)
        monkeypatch.setattr(fused, "USE_NATIVE_GEMM", True)
        got = fused.encoder_forward(enc, x, dtype=torch.bfloat16)
    torch.testing.assert_close(got.cpu(), ref32.cpu(), rtol=3e-2, atol=5e-2)
    torch.testing.assert_close(got.cpu(), ref.cpu(), rtol=3e-2, atol=5e-2)


def test_ctc_loss_matches_oracle_within_1e3():
    """North-star parity figure: CTC loss of the full path (wav -> Fbank -> CNN -> ConMamba encoder -> ctc_lin ->
    log-softmax -> CTC) on the GPU vs the CPU oracle, fp32: |delta| <= 1e-3; bf16 autocast delta is reported."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs, samples_for_frames
    from oracle import conmamba_oracle as O
    cfg = ASRConfig("tiny", d_model=64, d_ffn=128, num_encoder_layers=3, n_fft=400, seed=11)
    model = ConMambaASR(cfg).to(DEV).eval()
    wavs, lens = synthetic_wavs(3, samples_for_frames(400), 21, DEV)
    gen = torch.Generator().manual_seed(4)
    tokens = torch.randint(3, 31, (3, 20), generator=gen)
    tok_lens = torch.tensor([1.0, 0.8, 0.6])
    with torch.no_grad():
        model.calibrate(wavs, lens)                                        # normaliser statistics from the first batch
        p32 = model.forward_ctc(wavs, lens)
        loss32 = model.ctc_objective(p32, tokens.to(DEV), lens, tok_lens.to(DEV))
        with torch.autocast("cuda", dtype=torch.bfloat16):
            pbf = model.forward_ctc(wavs, lens)
        lossbf = model.ctc_objective(pbf.float(), tokens.to(DEV), lens, tok_lens.to(DEV))
    p = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    enc = O.asr_encode(p, wavs.cpu(), lens.cpu(), 3, p["normalize.glob_mean"], p["normalize.glob_std"], n_fft=400)
    logp = torch.log_softmax(torch.nn.functional.linear(enc, p["ctc_lin.w.weight"], p["ctc_lin.w.bias"]), -1)
    ref = O.ctc_loss_batchmean(logp, tokens, lens.cpu(), tok_lens)
    d32, dbf = abs(float(loss32) - float(ref)), abs(float(lossbf) - float(ref))
    print(f"CTC loss: oracle {float(ref):.5f}  gpu fp32 {float(loss32):.5f} (|delta| {d32:.2e})  gpu bf16 {float(lossbf):.5f} (|delta| {dbf:.2e})")
    assert d32 <= 1e-3
    assert dbf <= 5e-2 * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unimamba_step_reproduces_forward(dtype):
    """Stateful single-step decode (reference bimamba.py:320-365): feeding a sequence token by token
    through UniMamba.step (cm_causal_conv1d_update + cm_selective_state_update, states from allocate_inference_cache)
    reproduces the full-sequence forward of the same mixer."""
    from mamba_asr_amd.modules.mamba.bimamba import UniMamba
    torch.manual_seed(4)
    m = UniMamba(d_model=64, d_state=16, d_conv=4, expand=2).to(DEV).eval()
    x = torch.randn(3, 21, 64, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.bfloat16):
        full = m(x)
        conv_state, ssm_state = m.allocate_inference_cache(3)
        outs = []
        for t in range(x.shape[1]):
            o, conv_state, ssm_state = m.step(x[:, t:t + 1], conv_state, ssm_state)
            outs.append(o)
        stepped = torch.cat(outs, dim=1)
    tol = dict(rtol=2e-4, atol=2e-5) if dtype == torch.float32 else dict(rtol=3e-2, atol=3e-2)
    torch.testing.assert_close(stepped.float(), full.float(), **tol)
    assert conv_state.shape == (3, 128, 4) and ssm_state.shape == (3, 128, 16) and ssm_state.abs().max() > 0
