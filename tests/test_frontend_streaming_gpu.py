"""The streamed front end on the device (cm_fbank_wav_stream, cm_fbank_finish_stream, cm_cnn_front_stream).

Bit-exactness.  A frame of cm_fbank_wav_stream and a row of cm_cnn_front_stream are the same statements of the same kernel templates
as cm_fbank_wav / cm_cnn_front, so the streamed rows must be torch.equal to the whole-utterance kernels' whenever the causal and the
per-utterance top_db clamp coincide.  asr.synthetic_wavs has under 64 dB of range before the clamp: both clamps are the identity.
Every test that relies on this asserts max - min < top_db on the whole-utterance features first.

Where the causal clamp binds the references are the fp64 restatements of tests/test_front_end_edges.py with the causal floor applied
in fp64, under that file's bounds: check_fbank (rtol 1e-4, atol 2e-3 dB / min(std)) and check_front (cm_cnn_front's two conditions)."""
import dataclasses

import numpy as np
import pytest
import torch

import guard_bands as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
HOP, NFFT = 160, 512
SAMPLES = (6093, 6253, 6413, 6573)                       # T = 39, 40, 41, 42
LONG = 48007                                             # 301 frames, 76 rows: past cm_fbank_wav's 16-frame tile and cm_cnn_front's 16-tile chunk


def chunkings(s):
    if s == LONG:
        return ((s,), (10240,) * 4 + (s - 40960,))
    return ((s,), (640,) * 9 + (s - 5760,), (1, 735, 1, 159, 160, 161, 2000, 513, s - 3730))


_CACHE = {}


def model():
    """The front end of CONFIGS["conmamba_large_ctc"] behind one causal encoder layer (the encoder is not run here), calibrated."""
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR, synthetic_wavs
    if "m" not in _CACHE:
        m = ConMambaASR(dataclasses.replace(CONFIGS["conmamba_large_ctc"], name="front", num_encoder_layers=1, causal=True)).to(DEV).eval()
        m.calibrate(*synthetic_wavs(3, SAMPLES[0], 3, DEV))
        assert m.normalize.glob_mean.numel() == 80
        _CACHE["m"] = m
    return _CACHE["m"]


def cnn_rows(m, feats):
    from mamba_asr_amd import fused, ops
    c = fused._frontend_cache(m, BF16)
    b0 = m.CNN.blocks[0]
    n0 = b0.norm.norm
    return ops.cnn_front(feats, b0.conv.weight, b0.conv.bias, n0.weight, n0.bias, n0.eps, c["w2_ohwi"], c["b2f"], c["ln2"][0], c["ln2"][1],
                         c["ln2"][2], 0.01)


def whole_features(m, wav, norm=True):
    from mamba_asr_amd import ops
    fb = m.compute_features
    stats = (m.normalize.glob_mean, m.normalize.glob_std) if norm else (None, None)
    return ops.fbank_from_wav(wav, fb.window, fb.n_fft, fb.hop, fb.fbank, fb.amin, fb.top_db, *stats)


def reference(s, seed=3):
    """(wav, rows of the whole-utterance kernels), computed once per length; the clamp's precondition is asserted here."""
    from mamba_asr_amd.asr import synthetic_wavs
    if ("ref", s, seed) not in _CACHE:
        m = model()
        wav, _ = synthetic_wavs(3, s, seed, DEV)
        raw = whole_features(m, wav, norm=False)
        rng = float((raw.amax(dim=(1, 2)) - raw.amin(dim=(1, 2))).max())
        assert rng < m.compute_features.top_db - 10.0, rng           # neither clamp binds: the whole-utterance kernels are the reference
        _CACHE["ref", s, seed] = (wav, cnn_rows(m, whole_features(m, wav)))
    return _CACHE["ref", s, seed]


def streamed(m, wav, chunks, dtype=BF16):
    from mamba_asr_amd import fused
    assert sum(chunks) == wav.shape[1]
    ctx = fused.FrontEndStreamingContext(wav.shape[0], wav.device, dtype)
    outs, pos = [], 0
    for i, n in enumerate(chunks):
        outs.append(fused.frontend_streaming(m, wav[:, pos:pos + n], ctx, last=i == len(chunks) - 1))
        pos += n
    return outs


@pytest.mark.parametrize("s", SAMPLES + (LONG,))
def test_bit_exact_against_the_whole_utterance_kernels(s):
    """Every chunking, zero-frame and zero-row calls and odd boundaries included: the concatenated rows are cm_fbank_wav ->
    cm_fbank_finish -> cm_cnn_front on the whole utterance, bit for bit."""
    from mamba_asr_amd import fused
    m = model()
    wav, ref = reference(s)
    t2 = fused.frontend_rows_total(s, HOP)
    assert ref.shape == (3, t2, 640) and ref.dtype == BF16
    for chunks in chunkings(s):
        outs = streamed(m, wav, chunks)
        got = torch.cat(outs, dim=1)
        assert got.dtype == BF16 and got.shape == ref.shape, (chunks, got.shape)
        G.assert_same_bits(got, ref, f"S = {s}, chunks {chunks}")


def quiet_then_loud():
    from mamba_asr_amd.asr import synthetic_wavs
    wav, _ = synthetic_wavs(3, SAMPLES[0], 3, "cpu")
    wav[:, :3000] *= 1e-5
    return wav


def stream_features(m, wav):
    """The causal features of the whole utterance by the two Fbank stream kernels in one call."""
    from mamba_asr_amd import fused, ops
    fb, (b, s) = m.compute_features, wav.shape
    hist, spare = torch.zeros(b, 512, device=DEV), torch.zeros(b, 512, device=DEV)
    t = 1 + s // HOP
    db, fmax = ops.fbank_wav_stream(wav, hist, spare, 0, 0, t, fb.window, NFFT, HOP, fb.fbank, fb.amin, total=s)
    umax = torch.full((b,), float("-inf"), device=DEV)
    return ops.fbank_finish_stream(db, fmax, umax, 0, fb.top_db, *fused._front_norm(m, 80, wav.device))


def test_causal_clamp_on_the_device():
    """Quiet (x 1e-5) for 3000 samples, then loud: the two clamps differ in the quiet part.  All chunkings give the same bits; the
    features meet check_fbank against the fp64 STFT restatement with the causal floor applied in fp64; the rows meet check_front
    against the fp64 CNN restatement on those features."""
    from test_front_end_edges import check_fbank, check_front, front_64, stft_power64
    m = model()
    wav = quiet_then_loud()
    fb = m.compute_features
    power = torch.from_numpy(np.stack([stft_power64(w.numpy(), fb.win) for w in wav]))                # (B, T, 257) fp64
    db = 10.0 * torch.log10(torch.clamp(power @ fb.fbank.double().cpu(), min=float(np.float32(fb.amin))))
    floor = db.amax(-1).cummax(dim=1).values[..., None] - fb.top_db
    # every utterance spans more than top_db: the per-utterance clamp would lift the quiet frames, the causal floor (their own past's
    # maximum - 80 dB) leaves them where they are.  (The causal floor lifting values: test_loud_then_digital_silence_...)
    assert float((db.amax(dim=(1, 2)) - db.amin(dim=(1, 2))).min()) > fb.top_db + 10.0
    mean, std = m.normalize.glob_mean.double().cpu(), m.normalize.glob_std.double().cpu()
    ref_feats = (torch.maximum(db, floor) - mean) / std
    feats = stream_features(m, wav.to(DEV))
    check_fbank(feats, ref_feats, atol=2e-3 / float(std.min()))
    rows = [torch.cat(streamed(m, wav.to(DEV), chunks), dim=1) for chunks in chunkings(SAMPLES[0])]
    for r in rows[1:]:
        G.assert_same_bits(r, rows[0], "chunkings of the quiet-then-loud signal")
    b0, b1 = m.CNN.blocks
    cpu = lambda t: t.detach().float().cpu()
    w = dict(w1=cpu(b0.conv.weight), b1=cpu(b0.conv.bias), g1=cpu(b0.norm.norm.weight), be1=cpu(b0.norm.norm.bias),
             w2=cpu(b1.conv.weight).to(BF16), b2=cpu(b1.conv.bias), g2=cpu(b1.norm.norm.weight), be2=cpu(b1.norm.norm.bias))
    check_front("streamed, causal clamp binding", rows[0], front_64(feats.double().cpu(), w))
    assert not torch.equal(rows[0], cnn_rows(m, whole_features(m, wav.to(DEV))))                     # the utterance clamp gives other rows


def test_loud_then_digital_silence_equals_the_default_kernels():
    """Loud for 3000 samples, then zeros: silent frames sit exactly on floor_db = -100 dB, both clamps lift them to the same
    max - 80 dB (the loudest frame lies in front of them), and no loud value is under either floor: torch.equal."""
    from mamba_asr_amd.asr import synthetic_wavs
    m = model()
    wav, _ = synthetic_wavs(3, SAMPLES[0], 7, DEV)
    wav[:, 3000:] = 0.0
    raw = whole_features(m, wav, norm=False)
    assert torch.equal(raw.amin(dim=(1, 2)), raw.amax(dim=(1, 2)) - 80.0)                           # the clamp binds
    first_silent = (3000 + m.compute_features.win // 2 + HOP - 1) // HOP                            # frames from here on have zeros only under the 400-sample window
    assert bool((raw[:, first_silent:] == raw.amax(dim=(1, 2))[:, None, None] - 80.0).all())         # ... and sit on the floor
    # the two clamps coincide iff no value in front of the utterance's loudest frame lies under max - 80 dB (behind it the
    # prefix maximum is the maximum): the frames in front of the silence span under 70 dB
    loud = raw[:, :first_silent]
    assert int(raw.amax(-1).argmax(1).max()) < first_silent and float((loud.amax(dim=(1, 2)) - loud.amin(dim=(1, 2))).max()) < 70.0
    ref = cnn_rows(m, whole_features(m, wav))
    for chunks in chunkings(SAMPLES[0])[1:]:
        G.assert_same_bits(torch.cat(streamed(m, wav, chunks), dim=1), ref, f"loud then silence, chunks {chunks}")


def test_batch_independence():
    """Stream 1 of a 3-stream context gives the bits it gives alone."""
    m = model()
    wav, _ = reference(SAMPLES[1])
    chunks = chunkings(SAMPLES[1])[2]
    three = torch.cat(streamed(m, wav, chunks), dim=1)
    alone = torch.cat(streamed(m, wav[1:2].contiguous(), chunks), dim=1)
    G.assert_same_bits(alone[0], three[1], "stream 1 alone against stream 1 of 3")


def test_route(monkeypatch):
    """A steady-state native call is the three stream kernels, with no torch.cat and no torch.stft; a call with no ready row launches
    no CNN kernel; CM_STREAM_FRONT_NATIVE=0 (the module flag) takes the generic route, within cm_cnn_front's bound of the native one."""
    from mamba_asr_amd import fused, ops
    from test_front_end_edges import check_front
    m = model()
    wav, ref = reference(SAMPLES[0])
    calls = {"cat": 0, "stft": 0}

    def counted(name):
        real = getattr(torch, name)

        def f(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return f

    ctx = fused.FrontEndStreamingContext(3, DEV, BF16)
    fused.frontend_streaming(m, wav[:, :1280], ctx)                                   # caches, tables
    monkeypatch.setattr(torch, "cat", counted("cat"))
    monkeypatch.setattr(torch, "stft", counted("stft"))
    ops.LAUNCH_LOG = []
    try:
        out = fused.frontend_streaming(m, wav[:, 1280:2080], ctx)                     # frames 7 .. 11, rows 1 and 2
        steady = [e[0] for e in ops.LAUNCH_LOG]
        del ops.LAUNCH_LOG[:]
        none = fused.frontend_streaming(m, wav[:, 2080:2240], ctx)                    # frame 12: row 3 needs frame 15
        no_row = [e[0] for e in ops.LAUNCH_LOG]
        del ops.LAUNCH_LOG[:]
        fused.frontend_streaming(m, wav[:, 2240:2250], ctx)                           # no frame: the samples go to the history
        no_frame = [e[0] for e in ops.LAUNCH_LOG]
        del ops.LAUNCH_LOG[:]
        nothing = fused.frontend_streaming(m, wav[:, 2250:2250], ctx)
        no_sample = [e[0] for e in ops.LAUNCH_LOG]
        torch.cuda.synchronize()
    finally:
        ops.LAUNCH_LOG = None
    print("steady:", steady, "no row:", no_row, "no frame:", no_frame, "no sample:", no_sample)
    assert out.shape == (3, 2, 640) and none.shape == (3, 0, 640) and nothing.shape == (3, 0, 640) and (ctx.frames, ctx.rows) == (13, 3)
    assert steady == ["cm_fbank_wav_stream", "cm_fbank_finish_stream", "cm_cnn_front_stream"], steady
    assert no_row == ["cm_fbank_wav_stream", "cm_fbank_finish_stream"] and no_frame == ["cm_fbank_wav_stream"] and no_sample == [], (no_row, no_frame, no_sample)
    G.assert_same_bits(out, ref[:, 1:3], "rows 1 and 2")
    assert calls == {"cat": 0, "stft": 0}, calls
    monkeypatch.setattr(fused, "USE_STREAM_FRONT_NATIVE", False)
    ops.LAUNCH_LOG = []
    try:
        generic = torch.cat(streamed(m, wav, chunkings(SAMPLES[0])[0]), dim=1)     # one call: its chunk logic is the CPU file's subject
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert calls["stft"] > 0 and not any(n.endswith("_stream") for n in names), names
    check_front("generic route against the native one", generic, ref.double().cpu())


def _state(m, wav, n0):
    """The native context after n0 samples, as plain tensors."""
    from mamba_asr_amd import fused
    ctx = fused.FrontEndStreamingContext(wav.shape[0], DEV, BF16)
    fused.frontend_streaming(m, wav[:, :n0], ctx)
    return ctx


@pytest.mark.parametrize("last", [False, True])
@pytest.mark.parametrize("n", [1377, 1])
def test_guard_bands(n, last):
    """One mid-stream and one finish call after 2015 samples (the next sample completes frame 11 and with it row 2), n = 1377 and
    n = 1: outputs and both new histories are views of sentinel buffers, the chunk and both histories views of NaN buffers.  The
    guarded launch has the plain one's bits, is finite, and writes nothing outside its views."""
    from mamba_asr_amd import fused, ops
    m = model()
    wav, _ = reference(SAMPLES[0])
    n0 = 2015
    ctx = _state(m, wav, n0)
    assert (ctx.frames, ctx.rows) == (11, 2)
    fb, b = m.compute_features, wav.shape[0]
    total = n0 + n
    t = 1 + total // HOP if last else -1
    f1 = t if last else fused.frontend_frames_ready(total, NFFT, HOP)
    r1 = fused.frontend_rows_total(total, HOP) if last else fused.frontend_rows_ready(total, NFFT, HOP)
    nf, nr = f1 - ctx.frames, r1 - ctx.rows
    assert nf >= 1 and nr >= 1
    mean, std = fused._front_norm(m, 80, wav.device)
    c = fused._frontend_cache(m, BF16)
    b0 = m.CNN.blocks[0]
    n0_ = b0.norm.norm

    def run(L):
        chunk = L.cols(wav[:, n0:total], align=4)
        hist, fhist = L.flat(ctx.samp_hist, rows=1), L.flat(ctx.feat_hist, rows=8)
        hist_out = L.out("hist_out", (b, 512), torch.float32)
        db = L.out("db", (b, nf, 80), torch.float32, contiguous=True)
        fmax = L.out("fmax", (b, nf), torch.float32)
        umax = L.out("umax", (b,), torch.float32, fill=ctx.umax)
        fhist_out = L.out("feat_hist_out", (b, 8, 80), torch.float32, contiguous=True)
        out = L.out("out", (b, nr, 640), BF16, contiguous=True)
        ops.fbank_wav_stream(chunk, hist, hist_out, n0, ctx.frames, nf, fb.window, NFFT, HOP, fb.fbank, fb.amin, total=total if last else -1,
                             bufs=dict(db=db, fmax=fmax))
        ops.fbank_finish_stream(db, fmax, umax, ctx.frames, fb.top_db, mean, std, fhist, fhist_out)
        ops.cnn_front_stream(db, fhist, ctx.frames, ctx.rows, nr, b0.conv.weight, b0.conv.bias, n0_.weight, n0_.bias, n0_.eps, c["w2_ohwi"],
                             c["b2f"], c["ln2"][0], c["ln2"][1], c["ln2"][2], 0.01, t_total=t, out=out)

    plain = G.two_step(run, DEV)
    want = fused.frontend_streaming(m, wav[:, n0:total], ctx, last=last)              # the route itself gives these bits
    G.assert_same_bits(plain["out"], want, "ops-level launch against fused.frontend_streaming")
    G.assert_same_bits(plain["hist_out"], ctx.samp_hist, "sample history")
    G.assert_same_bits(plain["feat_hist_out"], ctx.feat_hist, "feature history")


def test_end_to_end_wav_to_hypotheses():
    """A 2-layer causal ConMambaASR in bf16: encode_wav_streaming over 640-sample chunks has the row counts of the host arithmetic and
    meets the streaming encoder's bound against model.encode on the whole utterance (not bit-equal: the src Linear is a library GEMM);
    log_probs_wav_streaming feeds StreamingCTCBeamSearcher.step on every call, the zero-row call included."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamSearcher
    s = SAMPLES[0]
    model_ = ConMambaASR(ASRConfig("e2e", causal=True, num_encoder_layers=2)).to(DEV).eval()
    wav, lens = synthetic_wavs(2, s, 3, DEV)
    chunks = chunkings(s)[1]
    searcher = StreamingCTCBeamSearcher(blank_index=0, vocab_list=["<b>"] + [f"t{i}" for i in range(1, 31)], max_frames=64, beam_size=8)
    state = searcher.make_state(2, DEV)
    state.reset()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        model_.calibrate(wav, lens)
        whole = model_.encode(wav, lens)
        ctx = model_.make_streaming_context(2)
        outs, pos, seen = [], 0, 0
        for i, n in enumerate(chunks):
            last = i == len(chunks) - 1
            outs.append(model_.encode_wav_streaming(wav[:, pos:pos + n], ctx, last=last))
            pos += n
            want = (fused.frontend_rows_total(pos, HOP) if last else fused.frontend_rows_ready(pos, NFFT, HOP)) - seen
            assert outs[-1].shape == (2, want, 256), (i, outs[-1].shape, want)
            seen += want
        assert outs[0].shape[1] == 0 and seen == whole.shape[1]
        err = (torch.cat(outs, dim=1).float() - whole.float()).abs()
        print(f"encode_wav_streaming against encode: mean|err| {float(err.mean()):.3e}, max|err| {float(err.max()):.3e}")
        assert float(err.mean()) < 2e-3 and float(err.max()) < 6e-2
        assert bool(torch.isfinite(whole).all()) and float(whole.float().std()) > 0.1                # a real output (the final LayerNorm's scale)
        ctx.reset()
        pos, fed = 0, 0
        for i, n in enumerate(chunks):
            lp = model_.log_probs_wav_streaming(wav[:, pos:pos + n], ctx, last=i == len(chunks) - 1)
            pos += n
            searcher.step(lp.float(), state)
            fed += lp.shape[1]
            hyps = searcher.hypotheses(state)
            assert len(hyps) == 2
        assert all(len(h) >= 1 for h in hyps) and fed == whole.shape[1] and state.fed == [fed, fed]
