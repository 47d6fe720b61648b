"""The streamed front end with every slot at its own pace on the device (cm_fbank_wav_stream_slots, cm_fbank_finish_stream_slots,
cm_cnn_front_stream_slots), and waveform to text on top of it.

Bit-exactness as in tests/test_frontend_streaming_gpu.py, whose model, signals and references are used here: asr.synthetic_wavs has
under 64 dB of range (asserted there, in reference()), so the streamed rows must be torch.equal to cm_fbank_wav -> cm_fbank_finish ->
cm_cnn_front on the whole utterance, and to the lock-step native context run on the stream alone.  In every call the samples of
wav_chunk[b] at and past n_valid[b] are NaN, and the buffer around wav_chunk is NaN."""
import pytest
import torch

import guard_bands as G
import test_frontend_streaming_gpu as FG

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
S = (6093, 6413, FG.LONG)                                 # 48007: past the 16-frame tile and the 16-tile seam
NAN = float("nan")


def chunk_buffer(wavs, pos, n):
    """(B, max n) inside a NaN buffer: NaN rows around, NaN columns behind, NaN behind every slot's n[b]."""
    B, w = len(wavs), max(n)
    buf = torch.full((B + 2, w + 64), NAN, device=DEV)
    view = buf[1:B + 1, :w]
    for b in range(B):
        view[b, :n[b]] = wavs[b][pos[b]:pos[b] + n[b]]
    return view


def drive(m, ctx, wavs, chunks, start=None, restart=None):
    """Slot b takes chunks[b] one per call from call start[b] on, its last chunk with last[b]; ``restart`` = (call, slot, wav, chunks).
    -> per slot the concatenated rows."""
    from mamba_asr_amd import fused
    B = len(wavs)
    wavs, chunks, start = list(wavs), [list(c) for c in chunks], list(start or [0] * B)
    pos, k, outs, call = [0] * B, [0] * B, [[] for _ in range(B)], 0
    while any(k[b] < len(chunks[b]) for b in range(B)):
        if restart is not None and call == restart[0]:
            _, slot, wav, ch = restart
            ctx.reset(rows=[slot])
            wavs[slot], chunks[slot], pos[slot], k[slot], outs[slot] = wav, list(ch), 0, 0, []
        live = [call >= start[b] and k[b] < len(chunks[b]) for b in range(B)]
        n = [chunks[b][k[b]] if live[b] else 0 for b in range(B)]
        last = [live[b] and k[b] == len(chunks[b]) - 1 for b in range(B)]
        rows, row_lens = fused.frontend_streaming_slots(m, chunk_buffer(wavs, pos, n), n, ctx, last=last)
        assert rows.shape == (B, max(row_lens), 640) and rows.dtype == BF16
        for b in range(B):
            assert not bool(rows[b, row_lens[b]:].any())
            if live[b]:
                outs[b].append(rows[b, :row_lens[b]])
                pos[b] += n[b]
                k[b] += 1
        call += 1
    return [torch.cat(o) for o in outs]


def case():
    refs = [FG.reference(s) for s in S]
    wavs = [refs[b][0][b] for b in range(3)]
    want = [refs[b][1][b] for b in range(3)]
    chunks = [FG.chunkings(S[0])[2], FG.chunkings(S[1])[1], FG.chunkings(S[2])[1]]
    return wavs, want, chunks


def test_bit_exact_against_the_whole_utterance_kernels_and_the_lock_step_context():
    from mamba_asr_amd import fused
    m = FG.model()
    wavs, want, chunks = case()
    ctx = fused.SlotFrontEndStreamingContext(3, DEV, BF16)
    assert fused.frontend_streaming_native(m, ctx)
    got = drive(m, ctx, wavs, chunks)
    for b in range(3):
        alone = torch.cat(FG.streamed(m, wavs[b][None], chunks[b]), dim=1)[0]
        print(f"slot {b} (S = {S[b]}, {len(chunks[b])} calls): {got[b].shape[0]} rows; torch.equal to the whole-utterance kernels "
              f"{torch.equal(got[b], want[b])}, to the lock-step context alone {torch.equal(got[b], alone)}")
        assert got[b].shape == want[b].shape and torch.equal(got[b], want[b]), b
        assert torch.equal(got[b], alone), b
    assert ctx.finished == [True] * 3 and ctx.samples == list(S)


def test_a_slot_reset_and_reused_equals_its_second_utterance_alone():
    from mamba_asr_amd import fused
    m = FG.model()
    wavs, want, chunks = case()
    wav2, want2 = FG.reference(6253)[0][1], FG.reference(6253)[1][1]
    ctx = fused.SlotFrontEndStreamingContext(3, DEV, BF16)
    # slot 0 is stopped in mid-utterance before call 4 and starts the second utterance; slot 1 starts 2 calls late
    got = drive(m, ctx, wavs, chunks, start=[0, 2, 0], restart=(4, 0, wav2, FG.chunkings(6253)[1]))
    assert torch.equal(got[0], want2), "the reset left something of the first utterance in slot 0"
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), "a neighbour noticed the reset"


def test_launch_counts():
    """3 launches; 2 when no slot has a row; 1 when no slot has a frame; none when nothing arrived and no slot ends."""
    from mamba_asr_amd import fused, ops
    m = FG.model()
    wavs, _, _ = case()
    ctx = fused.SlotFrontEndStreamingContext(3, DEV, BF16)

    def call(n, last=False):
        pos = list(ctx.samples)
        ops.LAUNCH_LOG = []
        try:
            rows, lens = fused.frontend_streaming_slots(m, chunk_buffer(wavs, pos, n), n, ctx, last=last)
            torch.cuda.synchronize()
            return [e[0] for e in ops.LAUNCH_LOG], list(lens)
        finally:
            ops.LAUNCH_LOG = None
    assert call([100, 0, 255]) == (["cm_fbank_wav_stream_slots"], [0, 0, 0])
    assert call([200, 10, 0]) == (["cm_fbank_wav_stream_slots", "cm_fbank_finish_stream_slots"], [0, 0, 0])
    assert call([0, 0, 0]) == ([], [0, 0, 0])
    names, lens = call([1000, 0, 481])
    assert names == ["cm_fbank_wav_stream_slots", "cm_fbank_finish_stream_slots", "cm_cnn_front_stream_slots"] and lens == [1, 0, 1]
    names, lens = call([0, 0, 5357], last=[False, False, True])                # nothing arrives for two slots, the third ends
    assert len(names) == 3 and lens[:2] == [0, 0] and lens[2] == fused.frontend_rows_total(6093, FG.HOP) - 1


def test_guard_bands_at_1377_1_0():
    """Second call of three streams with n_valid = (1377, 1, 0): the five outputs (sample history, dB rows, frame maxima, feature
    history, rows) inside sentinels, the inputs inside NaN and NaN behind n_valid; the same bits as the plain launches."""
    from mamba_asr_amd import fused, ops
    m = FG.model()
    fb = m.compute_features
    wavs, _, _ = case()
    ctx = fused.SlotFrontEndStreamingContext(3, DEV, BF16)
    first = [700, 900, 333]
    fused.frontend_streaming_slots(m, chunk_buffer(wavs, [0, 0, 0], first), first, ctx)           # histories and umax non-trivial
    n = [1377, 1, 0]
    plan, _ = fused._slot_plan(m, ctx, chunk_buffer(wavs, first, n), n, False)
    nf_max, nr_max = max(p[4] for p in plan), max(p[6] for p in plan)
    assert nf_max > 0 and nr_max > 0 and plan[2][4] == 0
    host = torch.tensor(plan, dtype=torch.int32)
    table = (host, host.to(DEV))
    mean, std = fused._front_norm(m, 80, DEV)
    c = fused._frontend_cache(m, BF16)
    b0 = m.CNN.blocks[0]
    n0 = b0.norm.norm
    umax0 = ctx.umax.clone()

    def run(L):
        chunk = chunk_buffer(wavs, first, n)
        bufs = dict(db=L.out("db", (3, nf_max, 80), torch.float32, fill=0.0, rows=16, contiguous=True),
                    fmax=L.out("fmax", (3, nf_max), torch.float32, fill=0.0, rows=16, contiguous=True))
        db, fmax = ops.fbank_wav_stream(chunk, L.flat(ctx.samp_hist, 1), L.out("samp_hist_out", (3, 512), torch.float32, rows=1, contiguous=True),
                                        0, 0, nf_max, fb.window, fb.n_fft, fb.hop, fb.fbank, fb.amin, bufs=bufs, plan=table)
        umax = L.out("umax", (3,), torch.float32, fill=umax0, rows=64, contiguous=True)
        feat_hist = L.flat(ctx.feat_hist, 8)
        ops.fbank_finish_stream(db, fmax, umax, 0, fb.top_db, L.vec(mean), L.vec(std), feat_hist,
                                L.out("feat_hist_out", (3, 8, 80), torch.float32, rows=8, contiguous=True), n_fft=fb.n_fft, plan=table)
        ops.cnn_front_stream(db, feat_hist, 0, 0, nr_max, b0.conv.weight, b0.conv.bias, n0.weight, n0.bias, n0.eps, c["w2_ohwi"], c["b2f"],
                             c["ln2"][0], c["ln2"][1], c["ln2"][2], 0.01, out=L.out("out", (3, nr_max, 640), BF16, fill=0.0, rows=4, contiguous=True),
                             plan=table)
    outs = G.two_step(run, DEV)
    # and they are what the public call returns
    rows, lens = fused.frontend_streaming_slots(m, chunk_buffer(wavs, first, n), n, ctx)
    assert list(lens) == [p[6] for p in plan] and torch.equal(rows, outs["out"])
    assert torch.equal(ctx.samp_hist, outs["samp_hist_out"]) and torch.equal(ctx.feat_hist, outs["feat_hist_out"]) and torch.equal(ctx.umax, outs["umax"])


def test_end_to_end_wav_to_hypotheses_per_slot():
    """2 layers, bf16: three utterances of different lengths through log_probs_wav_slots in 640-sample calls; slot 1 starts 5 calls
    late, slot 2 is reused for a second utterance.  The hypotheses of every utterance are those of log_probs_wav_streaming on it alone
    at batch 1: the same number, the same text rank by rank, the scores within 6e-2 -- the bound
    tests/test_frontend_streaming_gpu.py::test_end_to_end_wav_to_hypotheses uses for the encoder rows, because the src Linear is a
    library GEMM."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamSearcher
    model = ConMambaASR(ASRConfig("e2e_slots", causal=True, num_encoder_layers=2)).to(DEV).eval()
    lengths = {"a": 6093, "b": 4800, "c": 3333, "d": 5120}
    wavs = {k: synthetic_wavs(1, s, 20 + i, DEV)[0][0] for i, (k, s) in enumerate(lengths.items())}
    vocab = ["<b>"] + [f"t{i}" for i in range(1, 31)]
    mk = lambda: StreamingCTCBeamSearcher(blank_index=0, vocab_list=vocab, max_frames=64, beam_size=8, topk=4)
    cut = lambda s: [640] * (s // 640) + ([s % 640] if s % 640 else [])
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        model.calibrate(*synthetic_wavs(2, 6093, 3, DEV))
        want = {}
        for k, w in wavs.items():                                               # every utterance alone, lock step, batch 1
            searcher, ctx = mk(), model.make_streaming_context(1)
            state = searcher.make_state(1, DEV)
            state.reset()
            ch, pos = cut(lengths[k]), 0
            for i, n in enumerate(ch):
                searcher.step(model.log_probs_wav_streaming(w[None, pos:pos + n], ctx, last=i == len(ch) - 1).float(), state)
                pos += n
            want[k] = searcher.hypotheses(state)[0]
        searcher, ctx = mk(), model.make_streaming_context(3, per_slot=True)
        state = searcher.make_state(3, DEV)
        state.reset()
        queue = [[("a", n) for n in cut(lengths["a"])], [(None, 0)] * 5 + [("b", n) for n in cut(lengths["b"])],
                 [("c", n) for n in cut(lengths["c"])] + [("d", n) for n in cut(lengths["d"])]]
        pos, got, fed = {k: 0 for k in wavs}, {}, {k: 0 for k in wavs}
        for i in range(max(len(q) for q in queue)):
            call = [q[i] if i < len(q) else (None, 0) for q in queue]
            reset = None
            if call[2][0] == "d" and pos["d"] == 0:                             # slot 2 starts its second utterance with this call
                got["c"] = searcher.hypotheses(state, rows=[2])[0]
                ctx.reset(rows=[2])
                reset = [2]
            n = [c[1] for c in call]
            last = [k is not None and pos[k] + c == lengths[k] for k, c in call]
            live = {k: wavs[k] for k, _ in call if k}
            buf = chunk_buffer([live.get(k, wavs["a"]) for k, _ in call], [pos.get(k, 0) for k, _ in call], n)
            lp, row_lens = model.log_probs_wav_slots(buf, n, ctx, last=last)
            searcher.step(lp.float(), state, lengths=row_lens, reset=reset)
            for (k, c), r in zip(call, row_lens):
                if k:
                    pos[k] += c
                    fed[k] += r
        hyps = searcher.hypotheses(state)
        got.update(a=hyps[0], b=hyps[1], d=hyps[2])
    from mamba_asr_amd import fused
    for k in wavs:
        assert pos[k] == lengths[k] and fed[k] == fused.frontend_rows_total(lengths[k], FG.HOP)
        print(f"utterance {k}: {len(got[k])} / {len(want[k])} hypotheses; best '{got[k][0].text}' {got[k][0].score:.4f} / alone {want[k][0].score:.4f}")
        assert len(got[k]) == len(want[k]) >= 1, k
        for rank, (g_, w_) in enumerate(zip(got[k], want[k])):
            assert g_.text == w_.text, (k, rank)
            assert abs(g_.score - w_.score) < 6e-2, (k, rank, g_.score, w_.score)
