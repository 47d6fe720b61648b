"""GPU checks of the streamed CTC beam search (csrc/ctc_beam_stream.hip behind ops.ctc_beam_stream and
ctc_decode.StreamingCTCBeamSearcher).  The reference is the whole-utterance kernel (ops.ctc_beam_search): fed chunk by chunk, the
search must return its bits -- tokens, lengths, counts and the float64 scores with torch.equal -- and, through it, the tests' float64
host restatement (tests/ctc_beam_ref.py) by the rule of tests/test_ctc_beam_search_gpu.py (1e-9).

SPM_VOCAB (V = 31), T = 64, blank 0; the chunkings are one chunk, 64 single frames, (1, 2, 3, 5, 29, 24) and (40, 24)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_beam_ref as R  # noqa: E402
import guard_bands as GB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
T, V = 64, 31
CHUNKINGS = {"whole": (64,), "64x1": (1,) * 64, "ragged": (1, 2, 3, 5, 29, 24), "40_24": (40, 24)}
REGIMES = {
    "peaky": (D.peaky, dict(D.RECIPE)),
    "competing": (D.competing, dict(D.RECIPE)),
    # all 31 tokens pass -9 in every frame (the minimum log-prob is about -7.4): 3100 candidates > 1024, the global-memory sort
    "global_sort": (D.competing, dict(blank_index=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-9.0, topk=5,
                                      prune_history=True)),
    # 27 to 40 of the 64 frames are skipped: chunks of length 1 made only of skipped frames, processed steps < frames
    "blank_skip": (D.peaky, dict(D.RECIPE, blank_skip_threshold=0.9)),
}


def _searcher(max_frames=T, **kw):
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamSearcher
    return StreamingCTCBeamSearcher(vocab_list=D.SPM_VOCAB, max_frames=max_frames, **kw)


def _data(gen, seeds=(0, 1, 2), frames=T):
    return torch.stack([gen(frames, V, s) for s in seeds])


def _norm(out, width=T):
    """The kernel's raw outputs on the host with everything that is no output zeroed: token positions past a hypothesis' length,
    rows past num_hyps; tokens cut (or padded) to ``width`` columns, so that (batch, topk, T) and (batch, topk, max_frames) compare."""
    tokens, tlen, scores, nh = [x.cpu().clone() for x in out[:4]]
    tok = torch.zeros(tokens.shape[0], tokens.shape[1], width, dtype=tokens.dtype)
    for b in range(tokens.shape[0]):
        for h in range(tokens.shape[1]):
            if h < nh[b]:
                n = int(tlen[b, h])
                assert 0 <= n <= min(width, tokens.shape[2])
                tok[b, h, :n] = tokens[b, h, :n]
            else:
                tlen[b, h], scores[b, h] = 0, 0.0
    return tok, tlen, scores, nh


def _whole(s, lp, lengths):
    """ops.ctc_beam_search on the whole matrix, normalised; bad_frame must be clean."""
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    tc, th, tp = s._tables(DEV)
    n = torch.tensor(list(lengths), dtype=torch.int32, device=DEV)
    out = ops.ctc_beam_search(lp.to(DEV), n, tc, th, tp, HASH_BASE, HASH_SEP, blank=s.blank_index, beam_size=s.beam_size, topk=s.topk,
                              prune_history=s.prune_history, beam_prune_logp=s.beam_prune_logp,
                              token_prune_min_logp=s.token_prune_min_logp, blank_skip_threshold=s.blank_skip_threshold)
    assert out[4].cpu().tolist() == [-1] * lp.shape[0]
    return _norm(out)


def _emit(s, state, rows=None):
    """An emit-only launch for ``rows`` (default all), normalised; slots outside ``rows`` are zeroed (their rows are not written)."""
    rows = list(range(state.batch_size)) if rows is None else rows
    out = [x.cpu().clone() for x in s._launch(state, None, [0] * state.batch_size, emit=rows)]
    for b in range(state.batch_size):
        if b not in rows:
            out[3][b] = 0
    status = out[4]
    return _norm(out), [int(status[b]) for b in rows]


def _same(got, want, rows=None):
    for name, g, w in zip(("tokens", "token_len", "scores", "num_hyps"), got, want):
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.dtype == w.dtype and torch.equal(g, w), (name, g, w)


def _feed(s, state, lp, chunks, reset=True):
    """lp (B, frames, V) on the device through step() in the given chunking."""
    t0 = 0
    for i, n in enumerate(chunks):
        s.step(lp[:, t0:t0 + n], state, reset=list(range(state.batch_size)) if reset and i == 0 else None)
        t0 += n
    assert t0 == lp.shape[1]


def _texts(hyps):
    return [[(h.text, h.score) for h in hs] for hs in hyps]


_WHOLE = {}


def _regime(name, dtype=torch.float32):
    """(searcher, log-probs on the device, the whole-utterance kernel's normalised outputs) of a regime, computed once."""
    key = (name, dtype)
    if key not in _WHOLE:
        gen, kw = REGIMES[name]
        s = _searcher(**kw)
        lp = _data(gen).to(DEV).to(dtype)
        _WHOLE[key] = (s, lp, _whole(s, lp, [T] * 3), _texts(s(lp)))
    return _WHOLE[key]


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_any_chunking_gives_the_whole_utterance_bits(regime, chunking):
    s, lp, want, want_texts = _regime(regime)
    state = s.make_state(3, DEV)
    _feed(s, state, lp, CHUNKINGS[chunking])
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    _same(got, want)
    assert _texts(s.hypotheses(state)) == want_texts          # the public read: texts and score bits of CTCBeamSearcher's call
    if regime == "global_sort":
        assert want[3].tolist() == [5, 5, 5]
    assert state.fed == [T, T, T]


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
def test_bf16_log_probs(chunking):
    s, lp, want, want_texts = _regime("competing", torch.bfloat16)
    state = s.make_state(3, DEV)
    _feed(s, state, lp, CHUNKINGS[chunking])
    _same(_emit(s, state)[0], want)
    _same(want, _whole(s, lp.float(), [T] * 3))                # bf16 rows are read as their fp32 values


def test_emit_in_mid_stream():
    import test_ctc_beam_search_gpu as W
    s = _searcher(**dict(D.RECIPE, topk=5))
    lp = _data(D.competing, seeds=(0, 1))
    dev = lp.to(DEV)
    plain = s.make_state(2, DEV)                               # the same stream without any emit in between
    _feed(s, plain, dev, CHUNKINGS["ragged"])
    state, t0 = s.make_state(2, DEV), 0
    for i, n in enumerate(CHUNKINGS["ragged"]):
        s.step(dev[:, t0:t0 + n], state, reset=[0, 1] if i == 0 else None)
        t0 += n
        got, status = _emit(s, state)
        assert status == [-1, -1]
        _same(got, _whole(s, dev, [t0, t0]))
        again, _ = _emit(s, state)
        _same(again, got)                                      # emitting twice in a row: the same bits
        hyps = s.hypotheses(state)
        for b in range(2):
            W._match(hyps[b], R.beam_search(lp[b].double().tolist(), t0, D.SPM_VOCAB, blank=0, beam_size=100, beam_prune_logp=-12.0,
                                            token_prune_min_logp=-1.2, prune_history=False, topk=5))
    assert torch.equal(state.slab, plain.slab)                 # the emits left beams and history as they were
    _same(_emit(s, state)[0], _emit(s, plain)[0])


def test_ragged_streams():
    s = _searcher(**dict(D.RECIPE, topk=3))
    frames = [64, 37, 0]
    lp = _data(D.competing, seeds=(3, 4, 5))
    state, done = s.make_state(3, DEV), [0, 0, 0]
    pattern = [(5, 3, 0), (0, 7, 0), (11, 0, 0), (1, 1, 0), (16, 9, 0)]
    i = 0
    while done != frames:
        lengths = [min(p, f - d) for p, f, d in zip(pattern[i % len(pattern)], frames, done)]
        if any(lengths):
            t = max(lengths)
            chunk = torch.full((3, t, V), float("nan"))         # rows a slot does not consume hold NaN
            for b, n in enumerate(lengths):
                chunk[b, :n] = lp[b, done[b]:done[b] + n]
            s.step(chunk.to(DEV), state, lengths=lengths, reset=[0, 1, 2] if i == 0 else None)
            done = [d + n for d, n in zip(done, lengths)]
        i += 1
    assert state.fed == frames
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    for b, n in enumerate(frames):
        alone = _whole(s, lp[b:b + 1], [n])                    # the utterance decoded alone
        _same(tuple(x[b:b + 1] for x in got), alone)
    hyps = s.hypotheses(state)
    assert _texts(hyps)[2] == [("", 0.0)]


def _run_with_reset(s, lp, second, order):
    """Three slots fed lp in 8 chunks of 8; the slot holding stream 1 is reset at chunk 3 and fed ``second`` from there.
    ``order``: which stream each slot holds."""
    state = s.make_state(3, DEV)
    for i in range(8):
        chunk = lp[:, 8 * i:8 * i + 8].clone()
        if i >= 3:
            chunk[1] = second[8 * (i - 3):8 * (i - 3) + 8]
        reset = [0, 1, 2] if i == 0 else ([order.index(1)] if i == 3 else None)
        s.step(chunk[order].to(DEV), state, reset=reset)
    return state


def test_reset_starts_a_new_utterance_in_its_slot_only():
    s = _searcher(**dict(D.RECIPE, topk=3))
    lp, second = _data(D.competing, seeds=(6, 7, 8)), D.competing(40, V, 9)
    state = _run_with_reset(s, lp, second, [0, 1, 2])
    assert state.fed == [64, 40, 64]
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    alone = s.make_state(1, DEV)                               # the second utterance streamed alone
    _feed(s, alone, second[None].to(DEV), (8,) * 5)
    _same(tuple(x[1:2] for x in got), _emit(s, alone)[0])
    _same(tuple(x[1:2] for x in got), _whole(s, second[None], [40]))
    plain = s.make_state(3, DEV)                               # no reset: slots 0 and 2 must not notice their neighbour's
    _feed(s, plain, lp.to(DEV), (8,) * 8)
    _same(got, _emit(s, plain)[0], rows=[0, 2])
    assert torch.equal(state.slab[[0, 2]], plain.slab[[0, 2]])
    order = [2, 0, 1]                                          # a permutation of the slots permutes the results
    pm, _ = _emit(s, _run_with_reset(s, lp, second, order))
    _same(pm, tuple(x[order] for x in got))


def test_nan_is_reported_per_slot_and_reset_clears_it():
    s = _searcher(max_frames=80, **dict(D.RECIPE, topk=3))
    lp = _data(D.peaky, seeds=(10, 11, 12))
    bad = lp.clone()
    bad[1, 45, 5] = float("nan")                               # absolute frame 45: frame 5 of the second chunk
    state = s.make_state(3, DEV)
    _feed(s, state, bad.to(DEV), CHUNKINGS["40_24"])
    with pytest.raises(ValueError, match=r"slot 1 hold NaN at frame 45"):
        s.hypotheses(state)
    with pytest.raises(ValueError, match=r"slot 1 hold NaN at frame 45"):
        s.hypotheses(state, rows=[2, 1])
    want = _whole(s, lp, [T] * 3)
    got, status = _emit(s, state, rows=[0, 2])
    assert status == [-1, -1]
    _same(got, want, rows=[0, 2])
    assert _texts(s.hypotheses(state, rows=[2, 0])) == [_texts(s(lp.to(DEV)))[b] for b in (2, 0)]
    # the status is sticky: the slot consumes nothing more, an emit gives no hypotheses
    before = state.slab.clone()
    s.step(lp[:, :4].to(DEV), state, lengths=[0, 4, 0])
    assert torch.equal(state.slab, before)
    got, status = _emit(s, state, rows=[1])
    assert status == [45] and got[3].tolist() == [0, 0, 0]
    # after a reset the slot decodes again
    state.reset([1])
    assert state.fed == [T, 0, T]
    s.step(lp.to(DEV), state, lengths=[0, T, 0])
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    _same(got, want)


def test_overflow_is_a_status_and_leaves_the_state_alone():
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    s = _searcher(max_frames=16, **dict(D.RECIPE, topk=3))
    lp = _data(D.competing, seeds=(13, 14), frames=20).to(DEV)
    tc, th, tp = s._tables(DEV)
    state = ops.ctc_beam_stream_state(2, s.beam_size, 16, DEV)

    def call(chunk, lengths, reset=None, emit=None):
        i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
        return ops.ctc_beam_stream(chunk, i32(lengths), state, 16, tc, th, tp, HASH_BASE, HASH_SEP, reset=i32(reset), emit=i32(emit),
                                   blank=0, beam_size=s.beam_size, topk=s.topk, prune_history=s.prune_history,
                                   beam_prune_logp=s.beam_prune_logp, token_prune_min_logp=s.token_prune_min_logp)
    # a slot never reset refuses its chunk in the same way and has nothing to emit
    out = call(lp[:, :10], [10, 10], reset=[1, 0], emit=[1, 1])
    assert out[4].cpu().tolist() == [-1, -2] and out[3].cpu().tolist()[1] == 0 and not bool(state[1].any())
    out = call(lp[:, :10], [10, 10], reset=[1, 1])
    assert out[4].cpu().tolist() == [-1, -1]
    before = state.clone()
    out = call(lp[:, 10:20], [10, 6])                          # slot 0: 10 + 10 > 16, refused; slot 1: 10 + 6 = 16, the last that fits
    torch.cuda.synchronize()
    assert out[4].cpu().tolist() == [-2, -1]
    assert torch.equal(state[0], before[0]) and not torch.equal(state[1], before[1])
    out = call(None, [0, 0], emit=[1, 1])
    assert out[4].cpu().tolist() == [-1, -1]                   # the refusal is reported by its call, not stored
    _same(_norm(out, 16), _norm_width(_whole(s, lp, [10, 16]), 16))
    out = call(lp[:, 16:17], [0, 1])                           # one frame more than the slab holds
    assert out[4].cpu().tolist()[1] == -2


def _norm_width(out, width):
    return (out[0][:, :, :width].contiguous(),) + tuple(out[1:])


def test_guard_bands_around_outputs_state_and_workspace():
    """Outputs, state slab and workspace inside sentinels, the chunk inside NaN: one call that resets, consumes and emits slots 0
    and 2 while slot 1 idles, a second that continues slot 0 from the stored state.  beam 100 x 31 tokens: the sorts run in the
    workspace."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    gen, kw = REGIMES["global_sort"]
    F = 16
    s = _searcher(max_frames=F, **kw)
    lp = _data(gen, frames=F)
    tc, th, tp = s._tables(DEV)
    nstate = int(N.lib().cm_ctc_beam_stream_state_bytes(s.beam_size, F))
    nws = 3 * 4 * 8 * 4096
    assert nstate % 16 == 0

    def call(g, state, first, t0, lengths, reset, emit):
        t = 6
        chunk = torch.full((3, t, V), float("nan"))              # NaN in every row a slot does not consume, the row after its
        for b, n in enumerate(lengths):                           # last consumed frame included; NaN rows, columns and slots around
            chunk[b, :n] = lp[b, t0:t0 + n]
        chunk = GB.poisoned(chunk.to(DEV), rows=4, left=GB.LEFT, right=GB.RIGHT, align=4)
        i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
        bufs = {"tokens": g.out("tokens", (3, s.topk, F), torch.int32, contiguous=True),
                "token_len": g.out("token_len", (3, s.topk), torch.int32, contiguous=True),
                "scores": g.out("scores", (3, s.topk), torch.float64, contiguous=True),
                "num_hyps": g.out("num_hyps", (3,), torch.int32, contiguous=True),
                "status": g.out("status", (3,), torch.int32, contiguous=True),
                "workspace": g.scratch("workspace", nws // 4, torch.float32).view(torch.uint8)}
        if first:
            state = g.scratch("state", 3 * nstate // 4, torch.float32).view(torch.uint8).view(3, nstate)
        out = ops.ctc_beam_stream(chunk, i32(lengths), state, F, tc, th, tp, HASH_BASE, HASH_SEP, reset=i32(reset), emit=i32(emit),
                                  blank=0, beam_size=s.beam_size, topk=s.topk, prune_history=s.prune_history,
                                  beam_prune_logp=s.beam_prune_logp, token_prune_min_logp=s.token_prune_min_logp, bufs=bufs)
        torch.cuda.synchronize()
        for name, (buf, _, outside) in g.items.items():
            GB.assert_untouched(buf, outside, name)
        return state, out

    g1 = GB.Guards(DEV)
    state, out = call(g1, None, True, 0, [5, 0, 3], [1, 0, 1], [1, 0, 1])
    idle = torch.full((nstate // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    assert torch.equal(state[1], idle)                           # the idle slot's slab was neither read into a result nor written
    for name, x in zip(("tokens", "token_len", "scores", "num_hyps", "status"), out):
        assert bool((x[1] == GB.sentinel_of(x.dtype)).all()), f"{name}: the idle slot's output row was written"
    assert out[4].cpu().tolist()[0::2] == [-1, -1]
    keep = [x.clone() for x in out]
    for x in keep:
        x[1] = 0
    _same(_norm(keep, F), _norm_width(_whole(s, lp, [5, 0, 3]), F), rows=[0, 2])
    g2 = GB.Guards(DEV)
    _, out = call(g2, state, False, 5, [4, 0, 0], None, [1, 0, 0])
    GB.assert_untouched(g1.items["state"][0], g1.items["state"][2], "state")
    assert torch.equal(state[1], idle)
    assert int(out[4][0]) == -1
    for name, x in zip(("tokens", "token_len", "scores", "num_hyps", "status"), out):
        assert bool((x[1:] == GB.sentinel_of(x.dtype)).all()), f"{name}: an idle slot's output row was written"
    keep = [x.clone() for x in out]
    for x in keep:
        x[1:] = 0
    _same(_norm(keep, F), _norm_width(_whole(s, lp, [9, 0, 0]), F), rows=[0])


def test_step_captured_in_a_graph():
    s = _searcher(**dict(D.RECIPE, topk=3))
    lp = _data(D.competing, seeds=(15, 16, 17)).to(DEV)
    eager = s.make_state(3, DEV)
    _feed(s, eager, lp, (8,) * 8)
    static = torch.zeros(3, 8, V, device=DEV)
    warm = s.make_state(3, DEV)                                # loads the kernel and makes the searcher's cached device constants
    warm.reset()
    s.step(static, warm)
    state = s.make_state(3, DEV)
    state.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.step(static, state)                                  # one launch, nothing uploaded, nothing read
    for i in range(8):
        static.copy_(lp[:, 8 * i:8 * i + 8])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(state.slab, eager.slab)
    _same(_emit(s, state)[0], _emit(s, eager)[0])
    _same(_emit(s, state)[0], _whole(s, lp, [T] * 3))


def test_end_to_end_with_the_streamed_encoder():
    """Causal ConMambaASR (2 layers, d_model 256, 31 outputs) in bf16, 2 streams, 48 front-end rows in chunks of 16 through
    log_probs_streaming and step: the hypotheses are CTCBeamSearcher's on the concatenation of the streamed log-probs, texts and
    score bits.  Nothing is asserted about the head GEMM (ctc_lin) being invariant to the row count: the whole-utterance side is
    fed the streamed log-probs themselves, not log-probs recomputed from a 48-row call."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    cfg = ASRConfig("c", d_model=256, d_ffn=1024, num_encoder_layers=2, n_fft=400, causal=True, output_neurons=31, seed=5)
    model = ConMambaASR(cfg).to(DEV).eval()
    rows = torch.randn(2, 48, 20, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    ctx = model.Transformer.make_streaming_context(None, dict(batch_size=2, dtype=torch.bfloat16))
    kw = dict(blank_index=0, beam_size=16, beam_prune_logp=-12.0, token_prune_min_logp=-4.0, prune_history=False, topk=3)
    s = _searcher(**kw)
    state = s.make_state(2, DEV)
    state.reset()
    lps, mid = [], None
    with torch.no_grad():
        for t0 in (0, 16, 32):
            lp = model.log_probs_streaming(rows[:, t0:t0 + 16], ctx)
            assert lp.shape == (2, 16, 31)
            s.step(lp, state)
            lps.append(lp)
            if t0 == 16:
                mid = s.hypotheses(state)
    whole = CTCBeamSearcher(vocab_list=D.SPM_VOCAB, **kw)
    cat = torch.cat(lps, dim=1)
    assert _texts(s.hypotheses(state)) == _texts(whole(cat))
    assert _texts(mid) == _texts(whole(cat[:, :32]))
    assert all(len(h) >= 1 for h in s.hypotheses(state))
