"""The causal ConMamba encoder on the fused kernels, whole utterances and streamed chunk by chunk (GPU).  2 layers, d_model 256,
d_ffn 1024, input g_causal.x (4, 96, 256): against the REFERENCE's causal encoder (golden g_causal_large) and the fp64
composition tests/streaming_ref.py (held to that golden in tests/test_streaming_cpu.py).

Bounds (tests/test_seqpar.py's): bf16 fused route vs the golden rtol 3e-2, atol 5e-2; fp32 vs fp64 rtol 2e-3, atol 5e-4; the same
kernels with other edges mean|diff| < 2e-3, max < 6e-2."""
import pytest
import torch

import streaming_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CHUNKINGS = [(96,), (16,) * 6, (1, 2, 3, 5, 29, 31, 25), (40, 56)]
IDS = ["whole", "16x6", "ragged", "40_56"]
LAYER = ["cm_ffn_fused", "cm_conv_xproj_uni", "cm_scan_cl_fwd", "cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu_causal", "cm_ffn_fused"]


@pytest.fixture(scope="module")
def case():
    from mamba_asr_amd import fused
    enc, x = R.causal_large()
    enc, x = enc.to("cuda"), x.to("cuda")
    with torch.no_grad():
        whole = {dt: fused.encoder_forward(enc, x, dtype=dt, streams=1) for dt in (BF16, torch.float32)}
    return enc, x, whole


def stream(enc, x, chunks, dtype, ctx=None):
    ctx = enc.make_streaming_context(None, batch_size=x.shape[0], dtype=dtype) if ctx is None else ctx
    outs, t0 = [], 0
    with torch.no_grad():
        for n in chunks:
            out, none = enc.forward_streaming(x[:, t0:t0 + n], ctx)
            assert none is None and out.shape == (x.shape[0], n, x.shape[2]) and out.dtype == torch.float32
            outs.append(out)
            t0 += n
    assert t0 == x.shape[1]
    return torch.cat(outs, dim=1)


def test_causal_whole_utterance_bf16_vs_reference_golden(case, golden):
    enc, x, whole = case
    want = golden("g_causal_large")["y_enc"]
    err = (whole[BF16].cpu() - want).abs()
    print(f"fused causal bf16 vs reference: max|diff| {err.max():.3e} mean {err.mean():.3e}")
    torch.testing.assert_close(whole[BF16].cpu(), want, rtol=3e-2, atol=5e-2)
    # ConmambaEncoder.forward in eval mode without grad takes the same route
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        out, _ = enc(x)
    assert torch.equal(out, whole[BF16])


def test_causal_whole_utterance_fp32_vs_fp64(case):
    enc, x, whole = case
    want = R.causal_large_ref()
    err = (whole[torch.float32].double().cpu() - want).abs()
    print(f"fused causal fp32 vs fp64: max|diff| {err.max():.3e}")
    torch.testing.assert_close(whole[torch.float32].double().cpu(), want, rtol=2e-3, atol=5e-4)
    # prefix-causal on the kernels: frames 0..36 do not see the rest
    from mamba_asr_amd import fused
    with torch.no_grad():
        pre = fused.encoder_forward(enc, x[:, :37].contiguous(), dtype=torch.float32, streams=1)
    torch.testing.assert_close(pre, whole[torch.float32][:, :37], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("chunks", CHUNKINGS, ids=IDS)
def test_streamed_bf16_native_route(case, golden, chunks):
    enc, x, whole = case
    got = stream(enc, x, chunks, BF16)
    torch.testing.assert_close(got.cpu(), golden("g_causal_large")["y_enc"], rtol=3e-2, atol=5e-2)
    err = (got - whole[BF16]).abs()
    print(f"streamed bf16 {chunks} vs whole-utterance fused: torch.equal {torch.equal(got, whole[BF16])}, "
          f"max|diff| {err.max():.3e} mean {err.mean():.3e}")
    assert err.mean() < 2e-3 and err.max() < 6e-2


@pytest.mark.parametrize("chunks", CHUNKINGS, ids=IDS)
def test_streamed_fp32_generic_route(case, chunks):
    enc, x, whole = case
    got = stream(enc, x, chunks, torch.float32)
    err = (got.double().cpu() - R.causal_large_ref()).abs()
    print(f"streamed fp32 {chunks} vs fp64: max|diff| {err.max():.3e}; vs whole-utterance fused fp32: "
          f"max|diff| {(got - whole[torch.float32]).abs().max():.3e}")
    torch.testing.assert_close(got.double().cpu(), R.causal_large_ref(), rtol=2e-3, atol=5e-4)


def test_streamed_bf16_generic_route_with_the_switch_off(case, golden, monkeypatch):
    """CM_STREAM_NATIVE=0: the prepend-history route in bf16, the A/B partner of the native route."""
    from mamba_asr_amd import fused
    enc, x, whole = case
    monkeypatch.setattr(fused, "USE_STREAM_NATIVE", False)
    got = stream(enc, x, (16,) * 6, BF16)
    torch.testing.assert_close(got.cpu(), golden("g_causal_large")["y_enc"], rtol=3e-2, atol=5e-2)


def test_slots_are_independent(case):
    """After chunk 2 slot 1 is reset and fed a new utterance: its outputs are that utterance's, the other slots do not notice."""
    enc, x, whole = case
    S = R._synth()
    new = S.synth_input("g_causal.new", (1, 64, 256), 256).to("cuda")
    plain = stream(enc, x, (16,) * 6, BF16)                                     # no reset
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    outs = []
    with torch.no_grad():
        for i in range(6):
            if i == 2:
                ctx.reset(rows=[1])
            chunk = x[:, 16 * i:16 * i + 16].clone()
            if i >= 2:
                chunk[1] = new[0, 16 * (i - 2):16 * (i - 2) + 16]
            outs.append(enc.forward_streaming(chunk, ctx)[0])
    got = torch.cat(outs, dim=1)
    for slot in (0, 2, 3):
        assert torch.equal(got[slot], plain[slot]), f"slot {slot} changed"
    assert torch.equal(got[1, :32], plain[1, :32])
    # the same utterance in slot 1 of a fresh context beside other streams: the same kernels, so bit for bit
    beside = x[:, :64].clone()
    beside[1] = new[0]
    fresh = stream(enc, beside, (16,) * 4, BF16)
    assert torch.equal(got[1, 32:], fresh[1]), "the reset left something of the old utterance in slot 1"
    # and streamed alone (one stream: other launch shapes)
    alone = stream(enc, new, (16,) * 4, BF16)
    err = (got[1, 32:] - alone[0]).abs()
    print(f"slot 1 after reset vs the utterance streamed alone: torch.equal {torch.equal(got[1, 32:], alone[0])}, max|diff| {err.max():.3e}")
    assert err.mean() < 2e-3 and err.max() < 6e-2


def test_route_of_a_streamed_bf16_chunk(case, monkeypatch):
    """One streamed chunk is twelve native launches: no library GEMM inside a layer, no torch.cat of history rows."""
    from mamba_asr_amd import fused, ops
    enc, x, whole = case
    calls = {"gemm": 0, "cat": 0}

    def counted(name, key):
        real = getattr(fused, name) if key == "gemm" else torch.cat

        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f

    for name in ("_out_proj", "_in_proj", "_ffn"):
        monkeypatch.setattr(fused, name, counted(name, "gemm"))
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    with torch.no_grad():
        enc.forward_streaming(x[:, :16], ctx)                                   # caches, packed weights
    monkeypatch.setattr(torch, "cat", counted("cat", "cat"))
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            enc.forward_streaming(x[:, 16:32], ctx)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    print("launches of one streamed bf16 chunk:", names)
    assert names == LAYER * 2, names
    assert calls == {"gemm": 0, "cat": 0}, calls


def test_asr_encode_streaming_other_width_fp32():
    """ConMambaASR(ASRConfig(causal=True)) at d_model 64 (the generic route at another width): encode_streaming over the CNN front
    end's rows against the fp64 reference on the same rows, and against Transformer.encode on the whole utterance."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    model = ConMambaASR(ASRConfig("c", d_model=64, d_ffn=128, num_encoder_layers=2, n_fft=400, causal=True, seed=5)).to("cuda").eval()
    rows = torch.randn(3, 50, 20, 32, generator=torch.Generator().manual_seed(9)).to("cuda")      # (B, T, F, C) as the CNN leaves them
    ctx = model.Transformer.make_streaming_context(None, dict(batch_size=3))
    outs, t0 = [], 0
    with torch.no_grad():
        for n in (7, 1, 30, 12):
            outs.append(model.encode_streaming(rows[:, t0:t0 + n], ctx))
            t0 += n
        whole = model.Transformer.encode(rows)
        src = model.Transformer._prep_src(rows)
    got = torch.cat(outs, dim=1)
    sd = {k[len("encoder."):]: v for k, v in model.Transformer.state_dict().items() if k.startswith("encoder.")}
    want = R.causal_encoder(sd, src, 2)
    torch.testing.assert_close(got.double().cpu(), want, rtol=2e-3, atol=5e-4)
    torch.testing.assert_close(got, whole, rtol=2e-3, atol=5e-4)
