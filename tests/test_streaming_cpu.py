"""Streaming the causal ConMamba encoder: what can be checked without a GPU -- the fp64 reference the GPU tests use against the
REFERENCE's own causal encoder (golden g_causal_large), the streaming interface, and the two new C entry points' declarations
and refusals (every check is made before anything is launched, so host memory is enough)."""
import ctypes as ct
import os
import re

import pytest
import torch
import torch.nn as nn

import streaming_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3


def test_streaming_ref_matches_the_reference_causal_encoder(golden):
    """tests/streaming_ref.py (fp64, composed from the oracle) against the reference's ConmambaEncoder(causal=True): the bounds
    test_oracle_golden.py holds the oracle to on g4_large.  Also prefix-causal: the first 37 frames do not see the rest."""
    want = golden("g_causal_large")["y_enc"]
    got = R.causal_large_ref()
    print(f"streaming_ref vs reference: max|diff| {(got.float() - want).abs().max():.3e}, mean|y| {want.abs().mean():.3f}")
    torch.testing.assert_close(got.float(), want, rtol=1e-3, atol=1e-4)
    enc, x = R.causal_large()
    torch.testing.assert_close(R.causal_encoder(enc.state_dict(), x[:, :37], 2), got[:, :37], rtol=1e-9, atol=1e-9)


def test_reference_state_dict_keys_load_strict():
    """The causal encoder has the unidirectional mixer's keys only (what the reference's causal encoder saves)."""
    enc, _ = R.causal_large()
    keys = set(enc.state_dict())
    assert "layers.0.mamba.A_log" in keys and not any("_b." in k or "A_b_log" in k or k.endswith("D_b") for k in keys)


def test_make_streaming_context_shapes_and_reset():
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoderLayerStreamingContext, ConmambaEncoderStreamingContext
    enc, _ = R.causal_large()
    ctx = enc.make_streaming_context(None, batch_size=3, dtype=torch.bfloat16)
    assert isinstance(ctx, ConmambaEncoderStreamingContext) and len(ctx.layers) == 2 and ctx.batch_size == 3
    for l in ctx.layers:
        assert isinstance(l, ConmambaEncoderLayerStreamingContext)
        assert l.ssm_state.shape == (3, 512, 16) and l.ssm_state.dtype == torch.float32
        assert l.conv_state.shape == (3, 3, 512) and l.conv_state.dtype == torch.bfloat16
        assert l.dw_state.shape == (3, 30, 256) and l.dw_state.dtype == torch.bfloat16
        assert not l.ssm_state.any() and not l.conv_state.any() and not l.dw_state.any()
        for t in (l.ssm_state, l.conv_state, l.dw_state):
            t.fill_(1.0)
    assert enc.make_streaming_context("ignored", batch_size=1).layers[0].dw_state.dtype == torch.float32
    ctx.reset(rows=[1])
    for l in ctx.layers:
        for t in (l.ssm_state, l.conv_state, l.dw_state):
            assert not t[1].any() and bool(t[0].all()) and bool(t[2].all())
    ctx.reset()
    assert not any(t.any() for l in ctx.layers for t in (l.ssm_state, l.conv_state, l.dw_state))


def test_forward_streaming_refuses_a_bidirectional_encoder_and_a_wrong_batch():
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    bi = ConmambaEncoder(num_layers=1, d_model=32, d_ffn=64, activation=nn.GELU, causal=False, mamba_config=dict(R.CFG)).eval()
    enc, x = R.causal_large()
    ctx = enc.make_streaming_context(batch_size=4)
    with torch.no_grad():
        with pytest.raises(ValueError):
            bi.forward_streaming(torch.zeros(4, 8, 32), ctx)
        with pytest.raises(ValueError):
            bi.make_streaming_context(batch_size=4)
        with pytest.raises(ValueError):
            enc.forward_streaming(x[:3, :8], ctx)
    with pytest.raises(RuntimeError):                              # needs no grad
        enc.forward_streaming(x[:, :8], ctx)
    with torch.no_grad(), pytest.raises(RuntimeError):             # needs eval mode
        enc.train().forward_streaming(x[:, :8], ctx)


def test_asr_config_causal_builds_the_streamable_model():
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    from mamba_asr_amd.modules.TransformerASR import EncoderWrapper, TransformerASRStreamingContext
    from mamba_asr_amd.modules.mamba.bimamba import Mamba as BiMamba, UniMamba
    assert ASRConfig("x").causal is False
    model = ConMambaASR(ASRConfig("c", d_model=64, d_ffn=128, num_encoder_layers=2, n_fft=400, causal=True)).eval()
    for layer in model.Transformer.encoder.layers:
        assert isinstance(layer.mamba, UniMamba) and layer.convolution_module.causal and layer.convolution_module.padding == 30
        assert fused.supports(layer)
    plain = ConMambaASR(ASRConfig("p", d_model=64, d_ffn=128, num_encoder_layers=1, n_fft=400))
    assert isinstance(plain.Transformer.encoder.layers[0].mamba, BiMamba) and fused.supports(plain.Transformer.encoder.layers[0])
    ctx = model.Transformer.make_streaming_context(None, encoder_kwargs=dict(batch_size=2))
    assert isinstance(ctx, TransformerASRStreamingContext) and len(ctx.encoder_context.layers) == 2
    assert len(EncoderWrapper(model.Transformer).make_streaming_context(None, dict(batch_size=2)).encoder_context.layers) == 2
    assert ctx.encoder_context.batch_size == 2
    assert hasattr(model, "encode_streaming") and hasattr(model.Transformer, "encode_streaming")
    assert hasattr(EncoderWrapper(model.Transformer), "forward_streaming")


def test_new_symbols_are_declared_and_the_abi_is_still_12():
    from mamba_asr_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    assert re.search(r"^int cm_conv_xproj_uni\(const cm_conv_xproj_uni_args \*args\);", hdr, re.M)
    assert re.search(r"^int cm_glu_dwconv_ln_gelu_causal\(const cm_glu_dwconv_causal_args \*args\);", hdr, re.M)
    for name in ("cm_conv_xproj_uni", "cm_glu_dwconv_ln_gelu_causal"):
        assert name in {s[0] for s in N.SYMBOLS} and hasattr(N.lib(), name)
    assert re.search(r"^#define CM_ABI_VERSION 12$", hdr, re.M) and N.ABI_VERSION == 12 and N.lib().cm_abi_version() == 12
    # the existing structs are untouched: the causal one is the 'same' one plus two pointers
    assert ct.sizeof(N.GluDwconvCausalArgs) == ct.sizeof(N.GluDwconvArgs) + 16


def _host(nbytes=1 << 16):
    buf = torch.zeros(nbytes // 4 + 64)
    return buf, (buf.data_ptr() + 255) // 256 * 256                # 256-byte aligned host memory: nothing may be launched on it


def test_conv_xproj_uni_refuses_before_launching():
    from mamba_asr_amd import _native as N
    keep, p = _host()

    def call(**kw):
        a = N.ConvXprojUniArgs()
        a.batch, a.seqlen, a.dim, a.width, a.dt_pad = 2, 8, 64, 4, 16
        a.x, a.weight, a.wx, a.y, a.xdbl = p, p + 4096, p + 8192, p + 16384, p + 24576
        a.x_hist, a.x_hist_out = p + 32768, p + 36864
        a.x_bs, a.x_ts, a.y_bs, a.y_ts, a.xdbl_bs, a.xdbl_ts = 8 * 128, 128, 8 * 64, 64, 8 * 48, 48
        for k, v in kw.items():
            setattr(a, k, v)
        return N.lib().cm_conv_xproj_uni(ct.byref(a))

    assert N.lib().cm_conv_xproj_uni(None) == EINVAL
    for null in ("x", "weight", "wx", "y", "xdbl"):
        assert call(**{null: None}) == EINVAL, null
    assert call(seqlen=0) == EINVAL and call(batch=0) == EINVAL
    assert call(width=3) == EUNSUPPORTED and call(dim=48) == EUNSUPPORTED and call(dim=4096) == EUNSUPPORTED
    assert call(dt_pad=8) == EUNSUPPORTED
    assert call(x=p + 2) == EALIGN and call(x_hist=p + 32768 + 4) == EALIGN and call(x_hist_out=p + 36864 + 2) == EALIGN
    assert call(x_ts=126) == EALIGN and call(wx=p + 8192 + 8) == EALIGN
    assert call(x_hist_out=p + 32768) == EINVAL                                    # aliasing x_hist
    assert call(x_hist_out=p + 32768 + 2 * 3 * 64 * 2 - 8) == EINVAL               # overlapping its tail
    assert b"x_hist" in N.lib().cm_last_error()


def test_glu_dwconv_causal_refuses_before_launching():
    from mamba_asr_amd import _native as N
    keep, p = _host(1 << 18)

    def call(**kw):
        a = N.GluDwconvCausalArgs()
        a.batch, a.seqlen, a.dim, a.ksize, a.io_dtype, a.glu_done = 1, 4, 64, 31, N.CM_F32, 1
        a.in_, a.weight, a.bias, a.ln_g, a.ln_b, a.eps, a.out = p, p + 8192, p + 20480, p + 24576, p + 28672, 1e-5, p + 32768
        a.hist, a.hist_out = p + 65536, p + 98304
        for k, v in kw.items():
            setattr(a, k, v)
        return N.lib().cm_glu_dwconv_ln_gelu_causal(ct.byref(a))

    assert N.lib().cm_glu_dwconv_ln_gelu_causal(None) == EINVAL
    for null in ("in_", "weight", "ln_g", "ln_b", "out"):
        assert call(**{null: None}) == EINVAL, null
    assert call(seqlen=0) == EINVAL
    assert call(ksize=15) == EUNSUPPORTED and call(ksize=33) == EUNSUPPORTED and call(dim=63) == EUNSUPPORTED
    assert call(io_dtype=N.CM_F16) == EUNSUPPORTED
    assert call(hist=p + 65536 + 8) == EALIGN and call(hist_out=p + 98304 + 2) == EALIGN
    assert call(hist_out=p + 65536) == EINVAL                                      # aliasing hist
    assert call(hist_out=p + 65536 + 30 * 64 * 4 - 16) == EINVAL                   # overlapping its tail
    assert b"hist" in N.lib().cm_last_error()
    # the Linear epilogue belongs to the bf16 rows kernel at dim 256
    assert call(lin_w=p, lin_b=p) == EUNSUPPORTED
