"""The streamed front end (fused.frontend_streaming) on the CPU: the host arithmetic of what a call returns, the generic
torch route against the whole-utterance Fbank + ConvolutionFrontEnd, the causal top_db clamp where it binds, and the refusals of
the Python layer and of the three C entry points (host pointers, nothing launched).

The bound of the fp32 comparisons is rtol 1e-5, atol 1e-5: the project's bound for the same fp32 operations in another order
(tests/test_streaming_encoder_gpu.py::test_causal_whole_utterance_fp32_vs_fp64).  torch.stft on [history | chunk] and on the whole
utterance runs the same per-frame FFT; the CNN blocks see the same rows in batches of another size."""
import ctypes as C

import pytest
import torch

HOP, NFFT = 160, 512
S0 = 6093
SAMPLES = (6093, 6253, 6413, 6573)                       # T = 39, 40, 41, 42: every residue of T mod 4


def chunkings(s):
    return ((s,), (640,) * 9 + (s - 5760,), (1, 735, 1, 159, 160, 161, 2000, 513, s - 3730))


def totals(s):
    t = 1 + s // HOP
    t1 = (t + 1) // 2
    return t, t1, (t1 + 1) // 2


_MODEL = {}


def model():
    """The front end of the CTC-large configuration behind a one-layer encoder, fp32 on the CPU, calibrated on the test signal."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs
    if not _MODEL:
        m = ConMambaASR(ASRConfig("front", d_model=64, d_ffn=128, num_encoder_layers=1, causal=True, seed=5)).eval()
        wav, lens = synthetic_wavs(2, S0, 3, "cpu")
        m.calibrate(wav, lens)
        _MODEL["m"] = m
    return _MODEL["m"]


def whole(m, wav, causal=False):
    with torch.no_grad():
        feats = m.compute_features(wav, causal_top_db=causal)
        return m.CNN((feats - m.normalize.glob_mean) / m.normalize.glob_std).flatten(2)


def streamed(m, wav, chunks, dtype=torch.float32):
    from mamba_asr_amd import fused
    assert sum(chunks) == wav.shape[1]
    ctx = fused.FrontEndStreamingContext(wav.shape[0], wav.device, dtype)
    outs, pos = [], 0
    for i, n in enumerate(chunks):
        outs.append(fused.frontend_streaming(m, wav[:, pos:pos + n], ctx, last=i == len(chunks) - 1))
        pos += n
    return outs


def test_rows_ready_at_the_look_ahead_edges():
    """Row r is final once 640 r + 736 samples have arrived (frame 4r + 3 ends at 160 (4r + 3) + 256)."""
    from mamba_asr_amd import fused
    assert [fused.frontend_rows_ready(n, NFFT, HOP) for n in (735, 736, 1375, 1376)] == [0, 1, 1, 2]
    assert [fused.frontend_frames_ready(n, NFFT, HOP) for n in (0, 255, 256, 415, 416)] == [0, 0, 1, 1, 2]
    for r in range(40):
        assert fused.frontend_rows_ready(640 * r + 735, NFFT, HOP) == r and fused.frontend_rows_ready(640 * r + 736, NFFT, HOP) == r + 1


@pytest.mark.parametrize("s", SAMPLES)
def test_row_counts_sum_to_the_utterance(s):
    """Host arithmetic alone (the context's counters): every call returns rows_ready(after) - rows_ready(before), the finish the
    rest, T2 in all; a call may return none."""
    from mamba_asr_amd import fused
    t, _, t2 = totals(s)
    assert t == {6093: 39, 6253: 40, 6413: 41, 6573: 42}[s] and fused.frontend_rows_total(s, HOP) == t2
    m = model()
    wav = torch.zeros(1, s)
    for chunks in chunkings(s):
        outs = streamed(m, wav, chunks)
        seen, total = 0, 0
        for n, o in zip(chunks[:-1], outs[:-1]):
            seen += n
            assert o.shape == (1, fused.frontend_rows_ready(seen, NFFT, HOP) - total, 640)
            total += o.shape[1]
        assert total + outs[-1].shape[1] == t2


def test_generic_route_equals_the_whole_utterance():
    """B = 2, S = 6093, three chunkings with zero-frame and zero-row calls, odd boundaries and a boundary one sample either side of a
    hop: the streamed rows are the whole-utterance rows (for this signal neither clamp binds: asserted)."""
    from mamba_asr_amd.asr import synthetic_wavs
    m = model()
    wav, _ = synthetic_wavs(2, S0, 3, "cpu")
    with torch.no_grad():
        feats = m.compute_features(wav)
    assert float(feats.max() - feats.min()) < m.compute_features.top_db
    ref = whole(m, wav)
    zero_calls = 0
    for chunks in chunkings(S0):
        outs = streamed(m, wav, chunks)
        zero_calls += sum(o.shape[1] == 0 for o in outs)
        got = torch.cat(outs, dim=1)
        print(f"chunks {chunks}: rows per call {[o.shape[1] for o in outs]}, max|err| {float((got - ref).abs().max()):.3e}")
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
    assert zero_calls >= 4


def quiet_then_loud(s=S0):
    from mamba_asr_amd.asr import synthetic_wavs
    wav, _ = synthetic_wavs(2, s, 3, "cpu")
    wav[:, :3000] *= 1e-5
    return wav


def test_causal_clamp_that_binds():
    """First 3000 samples scaled by 1e-5: the utterance clamp lifts the quiet frames to max - 80 dB, the causal one leaves them (their
    floor is their own past's maximum - 80).  The streamed route is Fbank(causal_top_db=True); the difference to the default path
    lies in the quiet part only.  With the quiet part at the end the loudest frame comes first and both definitions coincide."""
    m = model()
    wav = quiet_then_loud()
    ref_causal, ref_default = whole(m, wav, causal=True), whole(m, wav, causal=False)
    for chunks in chunkings(S0)[1:]:
        got = torch.cat(streamed(m, wav, chunks), dim=1)
        torch.testing.assert_close(got, ref_causal, rtol=1e-5, atol=1e-5)
    diff = (ref_causal - ref_default).abs().amax(dim=(0, 2))                 # per row; row r reads samples 640 r - 736 .. 640 r + 736
    quiet_rows = [r for r in range(diff.numel()) if 640 * r + 736 <= 3000]
    loud_rows = [r for r in range(diff.numel()) if 640 * r - 736 >= 3000]
    assert quiet_rows and loud_rows
    assert float(diff[quiet_rows].min()) > 1e-3, diff                        # a hundred times the comparison's tolerance: really different
    torch.testing.assert_close(ref_causal[:, loud_rows], ref_default[:, loud_rows], rtol=1e-5, atol=1e-5)
    flipped = wav.flip(1).contiguous()                                        # loud first, quiet at the end
    with torch.no_grad():
        db = m.compute_features(flipped)
        pre = m.compute_features(flipped, causal_top_db=True)
    assert torch.equal(db.amin(dim=(1, 2)), db.amax(dim=(1, 2)) - 80.0)       # the clamp binds here too, in both utterances
    assert torch.equal(pre, db)                                               # ... and the two definitions give the same features
    got = torch.cat(streamed(m, flipped, chunkings(S0)[2]), dim=1)
    torch.testing.assert_close(got, whole(m, flipped), rtol=1e-5, atol=1e-5)


def test_fbank_causal_flag_default_is_untouched():
    from mamba_asr_amd.asr import synthetic_wavs
    m = model()
    wav, _ = synthetic_wavs(2, 3000, 4, "cpu")
    with torch.no_grad():
        assert torch.equal(m.compute_features(wav), m.compute_features(wav, causal_top_db=False))
        assert torch.equal(m.compute_features(wav), m.compute_features(wav, causal_top_db=True))      # 50 dB of range: neither binds


def test_python_refusals():
    from mamba_asr_amd import fused
    m = model()
    ctx = fused.FrontEndStreamingContext(2, "cpu", torch.float32)
    with pytest.raises(NotImplementedError, match="lock step"):
        ctx.reset(rows=[0])
    with pytest.raises(ValueError, match="batch = 2"):
        fused.frontend_streaming(m, torch.zeros(3, 100), ctx)
    for s in (0, 3, 4 * HOP - 1):                                             # T = 1, 1, 4
        ctx.reset()
        with pytest.raises(RuntimeError, match="at least 5 frames"):
            fused.frontend_streaming(m, torch.zeros(2, s), ctx, last=True)
    ctx.reset()
    assert fused.frontend_streaming(m, torch.zeros(2, 4 * HOP), ctx, last=True).shape == (2, 2, 640)       # T = 5
    with pytest.raises(RuntimeError, match="finished"):
        fused.frontend_streaming(m, torch.zeros(2, 10), ctx)
    ctx.reset()
    assert fused.frontend_streaming(m, torch.zeros(2, 0), ctx).shape == (2, 0, 640) and ctx.samples == 0
    full = m.make_streaming_context(2)
    assert full.frontend.batch_size == 2 and full.encoder.encoder_context.batch_size == 2
    with torch.no_grad():
        assert m.encode_wav_streaming(torch.zeros(2, 700), full).shape == (2, 0, 64)      # no row ready: the encoder is not called
    full.reset()
    assert full.frontend.samples == 0


def _host():
    host = (C.c_char * 8192)()
    return host, (C.addressof(host) + 63) // 64 * 64


def test_stream_entry_points_reject_without_launching():
    """cm_fbank_wav_stream / cm_fbank_finish_stream / cm_cnn_front_stream: NULL tensors and inconsistent counts -> CM_EINVAL (-1), a
    history written over the one that is read -> -1, another n_fft / filter count / bin or channel count -> CM_EUNSUPPORTED (-2), a
    misaligned table -> CM_EALIGN (-3).  Host pointers: a launch would fault."""
    import mamba_asr_amd._native as N
    lib = N.lib()
    _keep, base = _host()
    a = N.FbankStreamArgs()
    a.batch, a.n_mels, a.n_fft, a.hop, a.n, a.consumed, a.total, a.f0, a.nf = 2, 80, 512, 160, 1377, 2015, -1, 11, 9
    for f in ("chunk", "hist", "window", "twiddle", "band_lo", "band_hi", "band_off", "band_w", "db", "fmax", "umax", "feat_hist"):
        setattr(a, f, base)
    a.hist_out, a.feat_hist_out, a.chunk_bs, a.amin, a.top_db = base + 4096, base + 6144, 1377, 1e-10, 80.0
    assert lib.cm_fbank_wav_stream(None) == -1 and lib.cm_fbank_finish_stream(None) == -1 and lib.cm_cnn_front_stream(None) == -1
    for field, bad, rc in (("chunk", None, -1), ("hist", None, -1), ("hist_out", None, -1), ("hist_out", base, -1), ("hist_out", base + 4092, -1),
                           ("db", None, -1), ("fmax", None, -1), ("band_w", None, -1), ("n_fft", 400, -2), ("n_mels", 129, -2), ("hop", 161, -2),
                           ("window", base + 4, -3), ("twiddle", base + 4, -3), ("nf", 10, -1), ("f0", 10, -1), ("total", 3000, -1), ("n", -1, -1)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.cm_fbank_wav_stream(C.byref(a)) == rc, (field, bad, lib.cm_last_error())
        assert b"fbank_wav_stream" in lib.cm_last_error()
        setattr(a, field, good)
    for field, bad, rc in (("db", None, -1), ("fmax", None, -1), ("umax", None, -1), ("nf", 0, -1), ("n_fft", 400, -2), ("n_mels", 129, -2),
                           ("feat_hist_out", base, -1), ("feat_hist_out", base + 8 * 80 * 4 * 2 - 4, -1), ("feat_hist_out", None, -1), ("std", base, -1)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.cm_fbank_finish_stream(C.byref(a)) == rc, (field, bad, lib.cm_last_error())
        assert b"fbank_finish_stream" in lib.cm_last_error()
        setattr(a, field, good)
    c = N.CnnFrontStreamArgs()
    c.batch, c.F, c.C1, c.C2, c.f0, c.nf, c.r0, c.nr, c.T_total = 2, 80, 64, 32, 11, 9, 2, 3, -1
    for f in ("feats", "feat_hist", "w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "out"):
        setattr(c, f, base)
    for field, bad, rc in (("feats", None, -1), ("out", None, -1), ("w2", None, -1), ("F", 81, -2), ("C1", 32, -2), ("C2", 64, -2),
                           ("w2", base + 8, -3), ("ln1_g", base + 4, -3), ("nr", 0, -1), ("nr", 4, -1), ("r0", 1, -1), ("feat_hist", None, -1),
                           ("T_total", 4, -1), ("T_total", 21, -1)):
        good = getattr(c, field)
        setattr(c, field, bad)
        assert lib.cm_cnn_front_stream(C.byref(c)) == rc, (field, bad, lib.cm_last_error())
        assert b"cnn_front_stream" in lib.cm_last_error()
        setattr(c, field, good)


def test_ops_refuse_cpu_tensors():
    from mamba_asr_amd import ops
    z = torch.zeros
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.fbank_wav_stream(z(2, 10), z(2, 512), z(2, 512), 0, 0, 0, torch.hamming_window(400), 512, 160, z(257, 80))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.fbank_finish_stream(z(2, 3, 80), z(2, 3), z(2), 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.cnn_front_stream(z(2, 9, 80), None, 0, 0, 1, z(64, 1, 3, 3), z(64), z(40, 64), z(40, 64), 1e-5, z(32, 3, 3, 64, dtype=torch.bfloat16),
                             z(32), z(20, 32), z(20, 32), 1e-5)
