"""The streamed front end with every slot at its own pace (fused.frontend_streaming_slots) on the CPU: the host
arithmetic of the per-slot row counts, the generic torch route against the lock-step context run on each stream alone, the refusals
of the Python layer, and those of the three per-slot C entry points (host pointers, nothing launched).

Bound of the fp32 comparison: rtol 1e-5, atol 1e-5, the project's bound for the same fp32 operations at another batch size
(tests/test_frontend_streaming_cpu.py)."""
import ctypes as C

import pytest
import torch

import test_frontend_streaming_cpu as FC

HOP, NFFT = FC.HOP, FC.NFFT
S = (6093, 6253, 6573)


def slot_chunkings():
    """Per slot its own chunking: 640-sample calls; odd boundaries; and one with zero-sample, zero-frame and zero-row calls."""
    return [FC.chunkings(S[0])[1], FC.chunkings(S[1])[2], (0, 255, 1, 0, 480, 0, 640, 159, S[2] - 1535)]


def signals(seed=3):
    from mamba_asr_amd.asr import synthetic_wavs
    return [synthetic_wavs(1, s, seed + i, "cpu")[0][0] for i, s in enumerate(S)]


def drive(m, ctx, wavs, chunks, restart=None):
    """Feed slot b the chunks[b] of wavs[b], one per call, its last chunk with last[b]; a slot that is through idles.  ``restart``:
    (call, slot, wav, chunks): before that call the slot is reset and starts over on another signal.  -> (per slot the list of its
    row tensors, per call the row_lens list)."""
    from mamba_asr_amd import fused
    B = len(wavs)
    wavs, chunks = list(wavs), [list(c) for c in chunks]
    pos, k, outs, lens = [0] * B, [0] * B, [[] for _ in range(B)], []
    call = 0
    while any(k[b] < len(chunks[b]) for b in range(B)):
        if restart is not None and call == restart[0]:
            _, slot, wav, ch = restart
            ctx.reset(rows=[slot])
            wavs[slot], chunks[slot], pos[slot], k[slot], outs[slot] = wav, list(ch), 0, 0, []
        n = [chunks[b][k[b]] if k[b] < len(chunks[b]) else 0 for b in range(B)]
        last = [k[b] == len(chunks[b]) - 1 for b in range(B)]
        buf = torch.full((B, max(n)), float("nan"))
        for b in range(B):
            buf[b, :n[b]] = wavs[b][pos[b]:pos[b] + n[b]]
        rows, row_lens = fused.frontend_streaming_slots(m, buf, n, ctx, last=last)
        assert rows.shape == (B, max(row_lens), 640) and row_lens.dev.tolist() == list(row_lens)
        for b in range(B):
            assert not bool(rows[b, row_lens[b]:].any()), "rows at and past row_lens[b] must be zeros"
            if k[b] < len(chunks[b]):
                outs[b].append(rows[b, :row_lens[b]])
                pos[b] += n[b]
                k[b] += 1
            else:
                assert row_lens[b] == 0
        lens.append(list(row_lens))
        call += 1
    return outs, lens


def test_row_lens_are_the_lock_step_arithmetic_per_slot():
    from mamba_asr_amd import fused
    m = FC.model()
    chunks = slot_chunkings()
    assert [sum(c) for c in chunks] == list(S)
    ctx = fused.SlotFrontEndStreamingContext(3, "cpu", torch.float32)
    outs, lens = drive(m, ctx, signals(), chunks)
    for b, s in enumerate(S):
        seen, pos = 0, 0
        for i, n in enumerate(chunks[b]):
            pos += n
            want = (fused.frontend_rows_total(pos, HOP) if i == len(chunks[b]) - 1 else fused.frontend_rows_ready(pos, NFFT, HOP)) - seen
            assert lens[i][b] == want == outs[b][i].shape[0], (b, i, lens[i][b], want)
            seen += want
        assert seen == fused.frontend_rows_total(s, HOP) == FC.totals(s)[2]
        assert ctx.samples[b] == s and ctx.rows[b] == seen and ctx.frames[b] == FC.totals(s)[0] and ctx.finished[b]
    assert 0 in [l[2] for l in lens[:4]] and any(max(l) == 0 for l in lens)        # zero-row calls happened


def test_generic_route_against_lock_step_on_each_stream_alone():
    """Slots end in different calls; slot 1 is reset mid-utterance (before call 4) and restarted on another signal while the others
    go on."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import synthetic_wavs
    m = FC.model()
    chunks, wavs = slot_chunkings(), signals()
    other = synthetic_wavs(1, 6413, 11, "cpu")[0][0]
    other_chunks = FC.chunkings(6413)[2]
    ctx = fused.SlotFrontEndStreamingContext(3, "cpu", torch.float32)
    outs, _ = drive(m, ctx, wavs, chunks, restart=(4, 1, other, other_chunks))
    refs = [(wavs[0], chunks[0]), (other, other_chunks), (wavs[2], chunks[2])]
    for b, (wav, ch) in enumerate(refs):
        want = torch.cat(FC.streamed(m, wav[None], list(ch)), dim=1)[0]          # the lock-step context takes zero-sample calls too
        got = torch.cat(outs[b])
        print(f"slot {b}: {got.shape[0]} rows, max|diff| {float((got - want).abs().max()):.3e}")
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    assert ctx.finished == [True, True, True]


def test_python_refusals_leave_the_counters_alone():
    from mamba_asr_amd import fused
    m = FC.model()
    ctx = fused.SlotFrontEndStreamingContext(3, "cpu", torch.float32)
    wav = torch.randn(3, 2000, generator=torch.Generator().manual_seed(1)) * 0.1
    fused.frontend_streaming_slots(m, wav, [2000, 700, 1500], ctx, last=[True, False, False])
    state = lambda: (list(ctx.samples), list(ctx.frames), list(ctx.rows), list(ctx.finished))
    before = state()
    assert before[0] == [2000, 700, 1500] and before[3] == [True, False, False]
    with pytest.raises(ValueError, match="slot 0 has finished"):
        fused.frontend_streaming_slots(m, wav[:, :10], [10, 10, 10], ctx)
    for bad in ([11, 0, 0], [0, -1, 0]):
        with pytest.raises(ValueError, match="outside"):
            fused.frontend_streaming_slots(m, wav[:, :10], bad, ctx)
    with pytest.raises(ValueError, match="must have 3 entries"):
        fused.frontend_streaming_slots(m, wav[:, :10], [0, 0], ctx)
    with pytest.raises(ValueError, match="must have 3 entries"):
        fused.frontend_streaming_slots(m, wav[:, :10], [0, 0, 0], ctx, last=[True, False])
    with pytest.raises(ValueError, match="wav_chunk must be"):
        fused.frontend_streaming_slots(m, wav[:2, :10], [0, 0, 0], ctx)
    assert state() == before
    # a slot that ends under 5 frames: raised before any counter of ANY slot moves
    fresh = fused.SlotFrontEndStreamingContext(3, "cpu", torch.float32)
    fused.frontend_streaming_slots(m, wav[:, :300], [300, 300, 300], fresh)
    before = (list(fresh.samples), list(fresh.frames), list(fresh.rows), list(fresh.finished))
    with pytest.raises(RuntimeError, match="slot 1 ends its utterance with 3 feature frames"):
        fused.frontend_streaming_slots(m, wav[:, :500], [500, 100, 500], fresh, last=[False, True, False])
    assert (list(fresh.samples), list(fresh.frames), list(fresh.rows), list(fresh.finished)) == before
    # a finished slot idles with n_valid 0, and comes back after reset(rows)
    rows, lens = fused.frontend_streaming_slots(m, wav[:, :100], [0, 100, 100], ctx)
    assert lens[0] == 0 and ctx.samples == [2000, 800, 1600]
    ctx.reset(rows=[0])
    assert ctx.samples == [0, 800, 1600] and ctx.finished == [False, False, False]
    with pytest.raises(ValueError, match="outside a context"):
        ctx.reset(rows=[3])
    # the lock-step context keeps its contract
    with pytest.raises(NotImplementedError):
        fused.FrontEndStreamingContext(2, "cpu", torch.float32).reset(rows=[0])


def test_per_slot_asr_context():
    m = FC.model()
    ctx = m.make_streaming_context(2, dtype=torch.float32, per_slot=True)
    from mamba_asr_amd import fused
    assert isinstance(ctx.frontend, fused.SlotFrontEndStreamingContext) and ctx.encoder is not None
    ctx.frontend.samples[1] = 5
    ctx.reset(rows=[1])
    assert ctx.frontend.samples == [0, 0]
    assert isinstance(m.make_streaming_context(2, dtype=torch.float32).frontend, fused.FrontEndStreamingContext)


# ------------------------------------------------------------------------------------------------ the three C entry points
SLOTS = ("cm_fbank_wav_stream_slots", "cm_fbank_finish_stream_slots", "cm_cnn_front_stream_slots")


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    return N


def refused(native, rc, code, text):
    msg = native.lib().cm_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def host(nbytes):
    buf = C.create_string_buffer(nbytes + 256)
    return buf, (C.addressof(buf) + 255) // 256 * 256


def plan_of(rows):
    arr = (C.c_int32 * (8 * len(rows)))(*[v for r in rows for v in r])
    return arr, C.addressof(arr)


def test_six_symbols_and_the_abi(native):
    declared = {s[0]: s for s in native.SYMBOLS}
    handle = C.CDLL(native.LIB_PATH)
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12
    for name in SLOTS + ("cm_conv_xproj_uni_slots", "cm_scan_cl_fwd_slots", "cm_glu_dwconv_ln_gelu_causal_slots"):
        assert name in declared and hasattr(handle, name), name
    for name, args in zip(SLOTS, (native.FbankStreamArgs, native.FbankStreamArgs, native.CnnFrontStreamArgs)):
        assert declared[name][2] == [C.POINTER(args), C.c_void_p, C.c_void_p]


def test_fbank_slots_refusals(native):
    lib = native.lib()
    keep, base = host(1 << 16)
    a = native.FbankStreamArgs()
    a.batch, a.n_mels, a.n_fft, a.hop, a.n, a.nf = 2, 80, 512, 160, 640, 0
    a.chunk, a.chunk_bs, a.hist, a.hist_out = base, 640, base + 8192, base + 16384
    ok = [[640, 0, -1, 0, 0, 0, 0, -1], [100, 0, -1, 0, 0, 0, 0, -1]]
    pk, pp = plan_of(ok)
    for fn in (lib.cm_fbank_wav_stream_slots, lib.cm_fbank_finish_stream_slots):
        refused(native, fn(None, pp, pp), native.CM_EINVAL, "args is NULL")
        refused(native, fn(C.byref(a), None, pp), native.CM_EINVAL, "plan is NULL")
        refused(native, fn(C.byref(a), pp, None), native.CM_EINVAL, "plan is NULL")
        refused(native, fn(C.byref(a), pp + 2, pp), native.CM_EALIGN, "4-byte aligned")
    fn = lib.cm_fbank_wav_stream_slots
    a.hist_out = a.hist + 1024                                                  # inside the two slots' 4 KiB of history
    refused(native, fn(C.byref(a), pp, pp), native.CM_EINVAL, "hist_out overlaps hist")
    a.hist_out = base + 16384
    for bad, text in (([[641, 0, -1, 0, 0, 0, 0, -1], ok[1]], "above the maxima"),
                      ([ok[0], [100, 0, -1, 0, 3, 0, 0, -1]], "needs samples that have not arrived"),
                      ([ok[0], [100, 0, 50, 0, 0, 0, 0, -1]], "total must be -1 or consumed + n"),
                      ([ok[0], [-1, 0, -1, 0, 0, 0, 0, -1]], "bad sample counts")):
        bk, bp = plan_of(bad)
        refused(native, fn(C.byref(a), bp, bp), native.CM_EINVAL, text)
    refused(native, lib.cm_fbank_finish_stream_slots(C.byref(a), pp, pp), native.CM_EINVAL, "no frames")


def test_cnn_front_slots_refusals(native):
    fn = native.lib().cm_cnn_front_stream_slots
    keep, base = host(1 << 16)
    a = native.CnnFrontStreamArgs()
    a.batch, a.F, a.C1, a.C2, a.nf, a.nr = 2, 80, 64, 32, 8, 2
    a.feats, a.feat_hist, a.out = base, base + 8192, base + 16384
    a.w1 = a.ln1_g = a.ln1_b = a.w2 = a.ln2_g = a.ln2_b = base + 32768
    ok = [[0, 0, -1, 0, 8, 0, 2, -1], [0, 0, -1, 0, 0, 0, 0, -1]]
    pk, pp = plan_of(ok)
    refused(native, fn(None, pp, pp), native.CM_EINVAL, "args is NULL")
    refused(native, fn(C.byref(a), None, pp), native.CM_EINVAL, "plan is NULL")
    refused(native, fn(C.byref(a), pp, pp + 2), native.CM_EALIGN, "4-byte aligned")
    for bad, text in (([[0, 0, -1, 0, 8, 0, 3, -1], ok[1]], "above the maxima"),
                      ([[0, 0, -1, 0, 7, 0, 2, -1], ok[1]], "needs frames that have not arrived"),
                      ([ok[0], [0, 0, -1, 0, 0, 0, 1, -1]], "rows but no frames"),
                      ([[0, 0, -1, 0, 8, 0, 2, 9], ok[1]], "T_total must be f0 + nf"),
                      ([[0, 0, -1, 40, 8, 3, 2, -1], ok[1]], "reaches behind the feature history")):
        bk, bp = plan_of(bad)
        refused(native, fn(C.byref(a), bp, bp), native.CM_EINVAL, text)
    a.F = 40
    refused(native, fn(C.byref(a), pp, pp), native.CM_EUNSUPPORTED, "only 80 bins")
