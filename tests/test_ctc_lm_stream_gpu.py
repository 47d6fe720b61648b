"""GPU checks of the streamed LM-fused CTC beam search (csrc/ctc_beam_lm_stream.hip behind ops.ctc_beam_lm_stream and
ctc_decode.StreamingCTCBeamLMSearcher).  The yardstick is the whole-utterance LM kernel (ops.ctc_beam_search_lm): fed
chunk by chunk, the search must return its bits -- tokens, lengths, counts, the float64 acoustic scores and the float64 totals
(lm_scores), all with torch.equal.  Where the tests' float64 restatement (tests/ctc_lm_ref.py) is named, the inputs are those of
tests/test_ctc_lm_gpu.py, whose own prune / rank / cut margin exceeds 1e-7 (its _ref asserts that), and the comparison is its
_match at 1e-9.

SPM_VOCAB (V = 31), T = 40, blank 0; the chunkings are one chunk, 40 single frames, (1, 2, 3, 5, 29) and (24, 16)."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_lm_data as LD  # noqa: E402
import ctc_lm_ref as LR  # noqa: E402
import guard_bands as GB  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = math.inf
T, V = 40, 31
LENGTHS = [40, 0, 29]
RICH = dict(n_words=(18, 300, 300), n_bigrams=400, n_trigrams=300)
SPARSE = dict(n_words=(3, 3, 3), n_bigrams=8, n_trigrams=4)
CHUNKINGS = {"whole": (40,), "40x1": (1,) * 40, "ragged": (1, 2, 3, 5, 29), "24_16": (24, 16)}
GLOBAL_SORT = dict(blank_index=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-9.0, topk=5, prune_history=True)
REGIMES = {
    # the inputs of test_ctc_lm_gpu.test_recipe_settings_match_restatement: (generator, settings, compared with the restatement)
    "peaky": (D.peaky, dict(D.RECIPE, topk=10), True),
    "peaky_ph": (D.peaky, dict(D.RECIPE, topk=10, prune_history=True), True),
    "competing": (D.competing, dict(D.RECIPE, topk=10), True),
    "competing_ph": (D.competing, dict(D.RECIPE, topk=10, prune_history=True), True),
    # all 31 tokens pass -9 in every frame: up to 3100 candidates > 1024, the sorts run in the workspace
    "global_sort": (D.competing, GLOBAL_SORT, False),
    # chunks of length 1 made only of skipped frames, processed steps < frames
    "blank_skip": (D.peaky, dict(D.RECIPE, topk=10, blank_skip_threshold=0.9), False),
}
NAMES = ("tokens", "token_len", "scores", "lm_scores", "num_hyps")


@pytest.fixture(scope="module")
def arpa(tmp_path_factory):
    """make(seed, **generator keywords) -> path of the generated ARPA file, written once per module."""
    root, made = tmp_path_factory.mktemp("arpa"), {}

    def make(seed, **kw):
        key = (seed, repr(sorted(kw.items())))
        if key not in made:
            made[key] = LD.make_arpa(root / f"m{len(made)}.arpa", seed=seed, **kw)[0]
        return made[key]
    return make


def _batch(gen, lengths, frames, seed):
    """tests/test_ctc_lm_gpu._batch: utterance b holds gen(lengths[b], V, seed + b), -50 behind it."""
    import test_ctc_lm_gpu as W
    return W._batch(gen, lengths, frames, V, seed)


def _searcher(path, max_frames=T, vocab_list=D.SPM_VOCAB, **kw):
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamLMSearcher
    return StreamingCTCBeamLMSearcher(vocab_list=vocab_list, kenlm_model_path=path, max_frames=max_frames, **kw)


def _whole_searcher(path, vocab_list=D.SPM_VOCAB, **kw):
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    return CTCBeamSearcher(vocab_list=vocab_list, kenlm_model_path=path, **kw)


def _lm_kw(s):
    lm = s.lm
    return dict(order=lm.order, n_words=len(lm.words), lm_bos=lm.bos if s.score_boundary else -1,
                lm_eos=lm.eos if s.score_boundary else -1, lm_unk=lm.unk, alpha=s.alpha, beta=s.beta, unk_score_offset=s.unk_score_offset,
                blank=s.blank_index, beam_size=s.beam_size, topk=s.topk, prune_history=s.prune_history, beam_prune_logp=s.beam_prune_logp,
                token_prune_min_logp=s.token_prune_min_logp, blank_skip_threshold=s.blank_skip_threshold)


def _norm(out, width=T):
    """(tokens, token_len, scores, lm_scores, num_hyps) on the host with everything that is no output zeroed, as
    tests/test_ctc_beam_stream_gpu._norm does: token positions past a hypothesis' length, rows past num_hyps; tokens cut (or padded)
    to ``width`` columns, so that (batch, topk, T) and (batch, topk, max_frames) compare."""
    tokens, tlen, scores, lms, nh = [x.cpu().clone() for x in out[:5]]
    tok = torch.zeros(tokens.shape[0], tokens.shape[1], width, dtype=tokens.dtype)
    for b in range(tokens.shape[0]):
        for h in range(tokens.shape[1]):
            if h < nh[b]:
                n = int(tlen[b, h])
                assert 0 <= n <= min(width, tokens.shape[2])
                tok[b, h, :n] = tokens[b, h, :n]
            else:
                tlen[b, h], scores[b, h], lms[b, h] = 0, 0.0, 0.0
    return tok, tlen, scores, lms, nh


def _whole(s, lp, lengths, width=T):
    """ops.ctc_beam_search_lm, the whole-utterance LM kernel, on the whole matrix with the searcher's settings, normalised."""
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    tc, th, tp = s._tables(DEV)
    n = torch.tensor(list(lengths), dtype=torch.int32, device=DEV)
    out = ops.ctc_beam_search_lm(lp.to(DEV), n, tc, th, tp, s._tok_len(DEV), HASH_BASE, HASH_SEP, s.lm.tables(DEV), **_lm_kw(s))
    assert out[5].cpu().tolist() == [-1] * lp.shape[0]
    return _norm(out, width)


def _emit(s, state, rows=None, width=T):
    """An emit-only launch for ``rows`` (default all), normalised; slots outside ``rows`` are zeroed (their rows are not written)."""
    rows = list(range(state.batch_size)) if rows is None else rows
    out = [x.cpu().clone() for x in s._launch(state, None, [0] * state.batch_size, emit=rows)]
    for b in range(state.batch_size):
        if b not in rows:
            out[4][b] = 0
    return _norm(out, width), [int(out[5][b]) for b in rows]


def _same(got, want, rows=None):
    for name, g, w in zip(NAMES, got, want):
        if rows is not None:
            g, w = g[rows], w[rows]
        assert g.dtype == w.dtype and torch.equal(g, w), (name, g, w)


def _feed(s, state, lp, lengths, chunks, reset=True, start=0):
    """lp (B, frames, V) on the device through step(): slot b consumes its frames [start, lengths[b]) in the given chunking."""
    t0 = start
    for i, n in enumerate(chunks):
        take = [min(max(x - t0, 0), n) for x in lengths]
        s.step(lp[:, t0:t0 + n], state, lengths=None if set(take) == {n} else take,
               reset=list(range(state.batch_size)) if reset and i == 0 else None)
        t0 += n
    assert t0 >= max(lengths)


def _texts(hyps):
    return [[(h.text, h.score, h.lm_score) for h in hs] for hs in hyps]


_CASES = {}


def _regime(arpa, name, dtype=torch.float32):
    """Of a regime, computed once: (streamed searcher, log-probs on the device, the whole LM kernel's normalised outputs, the
    whole-utterance searcher's hypotheses, the restatement's hypotheses per utterance or None)."""
    import test_ctc_lm_gpu as W
    key = (name, dtype)
    if key not in _CASES:
        gen, kw, restated = REGIMES[name]
        path = arpa(4, **RICH)
        s = _searcher(path, **kw)
        lp = _batch(gen, LENGTHS, T, 100).to(dtype)
        dev = lp.to(DEV)
        refs = [W._ref(s, LR.DictLM(path), lp[b], n) for b, n in enumerate(LENGTHS)] if restated else None
        _CASES[key] = (s, dev, _whole(s, dev, LENGTHS), _whole_searcher(path, **kw)(dev, lengths=LENGTHS), refs)
    return _CASES[key]


def _check_stream(arpa, regime, chunking, dtype=torch.float32):
    import test_ctc_lm_gpu as W
    s, lp, want, want_hyps, refs = _regime(arpa, regime, dtype)
    state = s.make_state(3, DEV)
    _feed(s, state, lp, LENGTHS, CHUNKINGS[chunking])
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    _same(got, want)
    hyps = s.hypotheses(state)
    assert _texts(hyps) == _texts(want_hyps)                   # the public read: texts, score and lm_score bits of CTCBeamSearcher's
    assert state.fed == LENGTHS
    assert any(h.lm_score != h.score for h in hyps[0])         # the LM is on
    assert [(h.text, h.score) for h in hyps[1]] == [("", 0.0)] and hyps[1][0].lm_score != 0.0
    if refs is not None:
        for b in range(3):
            W._match(hyps[b], refs[b])
    return got


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("regime", sorted(REGIMES))
def test_any_chunking_gives_the_whole_utterance_bits(arpa, regime, chunking):
    got = _check_stream(arpa, regime, chunking)
    if regime == "global_sort":
        assert got[4].tolist() == [5, 1, 5]
    if regime.startswith("competing"):
        assert got[4].tolist() == [10, 1, 10]


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
def test_bf16_log_probs(arpa, chunking):
    _check_stream(arpa, "competing", chunking, torch.bfloat16)
    s, lp, want, _, _ = _regime(arpa, "competing", torch.bfloat16)
    assert lp.dtype == torch.bfloat16
    _same(want, _whole(s, lp.float(), LENGTHS))                # bf16 rows are read as their fp32 values


def test_emit_in_mid_stream(arpa):
    path = arpa(4, **RICH)
    s = _searcher(path, **dict(D.RECIPE, topk=5))
    lp = _batch(D.competing, [40, 40], T, 100).to(DEV)
    plain = s.make_state(2, DEV)                               # the same stream without any emit in between
    _feed(s, plain, lp, [40, 40], CHUNKINGS["ragged"])
    state, t0 = s.make_state(2, DEV), 0
    state.reset()
    # a reset slot without frames: the one empty hypothesis, lm_score = LM("") (the </s> term alone)
    hyps = s.hypotheses(state)
    want_empty = LR.final_total(LR.DictLM(path), "", 0.0, 0.5, 1.5, -10.0, True)
    for b in range(2):
        assert [(h.text, h.score) for h in hyps[b]] == [("", 0.0)]
        assert abs(hyps[b][0].lm_score - want_empty) <= 1e-12 and hyps[b][0].lm_score != 0.0
    for n in CHUNKINGS["ragged"]:
        s.step(lp[:, t0:t0 + n], state)
        t0 += n
        got, status = _emit(s, state)
        assert status == [-1, -1]
        _same(got, _whole(s, lp, [t0, t0]))
        again, _ = _emit(s, state)
        _same(again, got)                                      # emitting twice in a row: the same bits
    assert torch.equal(state.slab, plain.slab)                 # the emits left beams, LM states and history as they were
    _same(_emit(s, state)[0], _emit(s, plain)[0])


def test_ragged_streams_reset_and_copy(arpa):
    s = _searcher(arpa(4, **RICH), **dict(D.RECIPE, topk=3))
    frames = [40, 23, 0]
    lp = _batch(D.competing, frames, T, 100).to(DEV)
    second = _batch(D.competing, [24], 24, 7)[0].to(DEV)      # the utterance slot 1 starts at frame 16 of the others
    # ragged: 40 / 23 / 0 frames through step(lengths=), in chunks of 8
    state = s.make_state(3, DEV)
    _feed(s, state, lp, frames, (8,) * 5)
    assert state.fed == frames
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    _same(got, _whole(s, lp, frames))
    for b, n in enumerate(frames):
        _same(tuple(x[b:b + 1] for x in got), _whole(s, lp[b:b + 1], [n]))       # the utterance decoded alone
    # slot 1 is reset in mid-stream and fed `second` from there; slot 0 of a two-slot copy takes over slot 0's slab at frame 16
    both = torch.full((3, T, V), float("nan"), device=DEV)     # rows a slot does not consume hold NaN
    both[0], both[1, :16], both[1, 16:] = lp[0], lp[1, :16], second
    reset_state, copy = s.make_state(3, DEV), s.make_state(2, DEV)
    for i in range(5):
        take = [8, 8, 0]
        s.step(both[:, 8 * i:8 * i + 8], reset_state, lengths=take, reset=[0, 1, 2] if i == 0 else ([1] if i == 2 else None))
        if i == 1:
            copy.slab[1].copy_(reset_state.slab[0])            # a slab row copied is a stream copied
            copy.fed = [None, 16]
        if i >= 2:                                             # the copy continues slot 0's stream in its own slot 1
            s.step(torch.stack([both[2, 8 * i:8 * i + 8], both[0, 8 * i:8 * i + 8]]), copy, lengths=[0, 8])
    assert reset_state.fed == [40, 24, 0]
    got2, status = _emit(s, reset_state)
    assert status == [-1, -1, -1]
    _same(got2, got, rows=[0, 2])                              # the neighbours did not notice
    assert torch.equal(reset_state.slab[[0, 2]], state.slab[[0, 2]])
    _same(tuple(x[1:2] for x in got2), _whole(s, second[None], [24]))            # the slot equals a fresh utterance
    got3, status = _emit(s, copy, rows=[1])
    assert status == [-1]
    _same(tuple(x[1:2] for x in got3), tuple(x[0:1] for x in got))
    assert torch.equal(copy.slab[1], state.slab[0])


SPECIALS = {
    # name: (ARPA (seed, keywords), vocabulary, searcher settings, data (_special_data), compared with the restatement) -- the
    # models, settings and inputs of tests/test_ctc_lm_gpu.py, whose margins that file asserts; no_specials has no such input
    "order1": ((53, dict(order=1, letters=["A", "B"], n_words=(1, 1, 0), n_bigrams=30, n_trigrams=60, n_more=(90, 120))), "AB", {}, "AB", True),
    "order5": ((57, dict(order=5, letters=["A", "B"], n_words=(1, 1, 0), n_bigrams=30, n_trigrams=60, n_more=(90, 120))), "AB", {}, "AB", True),
    "no_specials_exact": ((31, dict(letters=["A", "B"], n_bigrams=12, n_trigrams=10, unk=False, bos=False, eos=False)), "AB",
                          dict(beam_size=256, topk=256, alpha=0.7, beta=1.1, unk_score_offset=-3.0), "AB5", True),
    "no_specials": ((9, dict(unk=False, bos=False, eos=False, **RICH)), "SPM", dict(alpha=0.8, beta=0.5, unk_score_offset=-4.0), "C36", False),
    "boundary_off": ((9, dict(unk=True, **RICH)), "SPM", dict(alpha=0.8, beta=0.5, unk_score_offset=-4.0, score_boundary=False), "C36", True),
    "boundary_on": ((9, dict(unk=True, **RICH)), "SPM", dict(alpha=0.8, beta=0.5, unk_score_offset=-4.0), "C36", True),
    "sparse_m10": ((8, SPARSE), "SPM", dict(unk_score_offset=-10.0), "C30", True),
    "sparse_0": ((8, SPARSE), "SPM", dict(unk_score_offset=0.0), "C30", True),
}


def _special_data(kind):
    if kind == "AB":
        g = torch.Generator().manual_seed(5)
        return [12, 11], torch.log_softmax(torch.randn(2, 12, 4, generator=g) * 0.7 + torch.tensor([0.0, 0.6, 0.6, 0.6]), dim=-1)
    if kind == "AB5":
        g = torch.Generator().manual_seed(5)
        return [5, 5], torch.log_softmax(torch.randn(2, 5, 4, generator=g, dtype=torch.float64) * 1.5, -1).float()
    if kind == "C36":
        return [36, 21], _batch(D.competing, [36, 21], 36, 500)
    return [24, 30], _batch(D.competing, [24, 30], 30, 300)


@pytest.mark.parametrize("case", sorted(SPECIALS))
def test_other_orders_and_specials(arpa, case):
    import test_ctc_lm_gpu as W
    (seed, akw), vocab, kw, kind, restated = SPECIALS[case]
    path = arpa(seed, **akw)
    if vocab == "AB":
        cfg = dict(dict(blank_index=0, vocab_list=["<b>", "▁", "A", "▁B"], beam_size=64, beam_prune_logp=-INF, token_prune_min_logp=-INF,
                        prune_history=False, topk=64, alpha=0.9, beta=0.3, unk_score_offset=-2.0), **kw)
    else:
        cfg = dict(D.RECIPE, vocab_list=D.SPM_VOCAB, topk=5, **kw)
    lengths, lp = _special_data(kind)
    frames = lp.shape[1]
    s = _searcher(path, max_frames=frames, **cfg)
    assert s.lm.order == akw.get("order", 3)
    if "no_specials" in case:
        assert (s.lm.bos, s.lm.eos, s.lm.unk) == (-1, -1, -1)
    dev = lp.to(DEV)
    state = s.make_state(2, DEV)
    _feed(s, state, dev, lengths, (5,) * ((frames + 4) // 5))
    got, status = _emit(s, state, width=frames)
    assert status == [-1, -1]
    _same(got, _whole(s, dev, lengths, width=frames))
    hyps = s.hypotheses(state)
    assert _texts(hyps) == _texts(_whole_searcher(path, **cfg)(dev, lengths=lengths))
    if restated:
        lm = LR.DictLM(path)
        for b, n in enumerate(lengths):
            W._match(hyps[b], W._ref(s, lm, lp[b], n))


@pytest.mark.parametrize("prune_history", [False, True])
def test_neutral_lm_is_the_lm_free_stream(arpa, prune_history):
    """alpha = beta = unk_score_offset = 0 and no </s>: outputs and score bits of the LM-free streamed search, lm_score == score."""
    import test_ctc_beam_stream_gpu as S
    from mamba_asr_amd.ctc_decode import StreamingCTCBeamSearcher
    cfg = dict(D.RECIPE, prune_history=prune_history, topk=10)
    fused = _searcher(arpa(2, eos=False, **RICH), alpha=0.0, beta=0.0, unk_score_offset=0.0, **cfg)
    free = StreamingCTCBeamSearcher(vocab_list=D.SPM_VOCAB, max_frames=T, **cfg)
    lengths = [40, 0, 33]
    lp = torch.cat([_batch(D.competing, lengths[:2], T, 70), _batch(D.peaky, lengths[2:], T, 80)]).to(DEV)
    a, b = free.make_state(3, DEV), fused.make_state(3, DEV)
    _feed(free, a, lp, lengths, CHUNKINGS["ragged"])
    _feed(fused, b, lp, lengths, CHUNKINGS["ragged"])
    (want, _), (got, status) = S._emit(free, a), _emit(fused, b)
    assert status == [-1, -1, -1] and got[4].tolist()[0] == 10
    for name, g, w in zip(("tokens", "token_len", "scores", "num_hyps"), (got[0][:, :, :T], got[1], got[2], got[4]), want):
        assert torch.equal(g, w[:, :, :T] if name == "tokens" else w), name
    assert torch.equal(got[3], got[2])                          # lm_score == score
    assert _texts(fused.hypotheses(b)) == [[(t, sc, sc) for t, sc in hs] for hs in S._texts(free.hypotheses(a))]


def test_nan_is_reported_per_slot_and_reset_clears_it(arpa):
    s = _searcher(arpa(4, **RICH), max_frames=48, **dict(D.RECIPE, topk=3))
    lp = _batch(D.peaky, [40, 40, 40], T, 10)
    bad = lp.clone()
    bad[1, 25, 5] = float("nan")                               # absolute frame 25: frame 1 of the second chunk
    state = s.make_state(3, DEV)
    _feed(s, state, bad.to(DEV), [40] * 3, CHUNKINGS["24_16"])
    with pytest.raises(ValueError, match=r"slot 1 hold NaN at frame 25"):
        s.hypotheses(state)
    with pytest.raises(ValueError, match=r"slot 1 hold NaN at frame 25"):
        s.hypotheses(state, rows=[2, 1])
    want = _whole(s, lp, [T] * 3)
    got, status = _emit(s, state, rows=[0, 2])
    assert status == [-1, -1]
    _same(got, want, rows=[0, 2])
    # the status is sticky: the slot consumes nothing more, an emit gives no hypotheses
    before = state.slab.clone()
    s.step(lp[:, :4].to(DEV), state, lengths=[0, 4, 0])
    assert torch.equal(state.slab, before)
    got, status = _emit(s, state, rows=[1])
    assert status == [25] and got[4].tolist() == [0, 0, 0]
    # after a reset the slot decodes again
    state.reset([1])
    assert state.fed == [T, 0, T]
    s.step(lp.to(DEV), state, lengths=[0, T, 0])
    got, status = _emit(s, state)
    assert status == [-1, -1, -1]
    _same(got, want)


def _call(s, state, F, chunk, lengths, reset=None, emit=None, lm=None, bufs=None):
    """ops.ctc_beam_lm_stream with the searcher's settings, flags from host lists."""
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    tc, th, tp = s._tables(DEV)
    i32 = lambda x: None if x is None else torch.tensor(x, dtype=torch.int32, device=DEV)  # noqa: E731
    return ops.ctc_beam_lm_stream(chunk, i32(lengths), state, F, tc, th, tp, s._tok_len(DEV), HASH_BASE, HASH_SEP,
                                  s.lm.tables(DEV) if lm is None else lm, reset=i32(reset), emit=i32(emit), bufs=bufs, **_lm_kw(s))


def test_overflow_is_a_status_and_leaves_the_state_alone(arpa):
    from mamba_asr_amd import ops
    s = _searcher(arpa(4, **RICH), max_frames=16, **dict(D.RECIPE, topk=3))
    lp = _batch(D.competing, [20, 20], 20, 13).to(DEV)
    state = ops.ctc_beam_lm_stream_state(2, s.beam_size, 16, DEV)
    # a slot never reset refuses its chunk in the same way and has nothing to emit
    out = _call(s, state, 16, lp[:, :10], [10, 10], reset=[1, 0], emit=[1, 1])
    assert out[5].cpu().tolist() == [-1, -2] and out[4].cpu().tolist()[1] == 0 and not bool(state[1].any())
    out = _call(s, state, 16, lp[:, :10], [10, 10], reset=[1, 1])
    assert out[5].cpu().tolist() == [-1, -1]
    before = state.clone()
    out = _call(s, state, 16, lp[:, 10:20], [10, 6])           # slot 0: 10 + 10 > 16, refused; slot 1: 10 + 6 = 16, the last that fits
    assert out[5].cpu().tolist() == [-2, -1]
    assert torch.equal(state[0], before[0]) and not torch.equal(state[1], before[1])
    out = _call(s, state, 16, None, [0, 0], emit=[1, 1])
    assert out[5].cpu().tolist() == [-1, -1]                   # the refusal is reported by its call, not stored
    _same(_norm(out, 16), _whole(s, lp, [10, 16], width=16))
    out = _call(s, state, 16, lp[:, 16:17], [0, 1])            # one frame more than the slab holds
    assert out[5].cpu().tolist()[1] == -2


def test_guard_bands_around_outputs_state_and_workspace(arpa):
    """Outputs (lm_scores among them), the state slab with its LM block and the workspace inside sentinels, the chunk inside NaN: one
    call that resets, consumes and emits slots 0 and 2 while slot 1 idles, a second that continues slot 0 from the stored state.
    beam 100 x 31 tokens: the sorts run in the workspace."""
    import mamba_asr_amd._native as N
    F = 16
    s = _searcher(arpa(4, **RICH), max_frames=F, **GLOBAL_SORT)
    lp = _batch(D.competing, [F] * 3, F, 100)
    nstate = int(N.lib().cm_ctc_beam_lm_stream_state_bytes(s.beam_size, F))
    nws = 3 * 4 * 8 * 4096
    assert nstate % 16 == 0 and nstate > int(N.lib().cm_ctc_beam_stream_state_bytes(s.beam_size, F))
    outs = ("tokens", "token_len", "scores", "lm_scores", "num_hyps", "status")

    def call(g, state, first, t0, lengths, reset, emit):
        t = 6
        chunk = torch.full((3, t, V), float("nan"))              # NaN in every row a slot does not consume, the row after its
        for b, n in enumerate(lengths):                           # last consumed frame included; NaN rows, columns and slots around
            chunk[b, :n] = lp[b, t0:t0 + n]
        chunk = GB.poisoned(chunk.to(DEV), rows=4, left=GB.LEFT, right=GB.RIGHT, align=4)
        bufs = {"tokens": g.out("tokens", (3, s.topk, F), torch.int32, contiguous=True),
                "token_len": g.out("token_len", (3, s.topk), torch.int32, contiguous=True),
                "scores": g.out("scores", (3, s.topk), torch.float64, contiguous=True),
                "lm_scores": g.out("lm_scores", (3, s.topk), torch.float64, contiguous=True),
                "num_hyps": g.out("num_hyps", (3,), torch.int32, contiguous=True),
                "status": g.out("status", (3,), torch.int32, contiguous=True),
                "workspace": g.scratch("workspace", nws // 4, torch.float32).view(torch.uint8)}
        if first:
            state = g.scratch("state", 3 * nstate // 4, torch.float32).view(torch.uint8).view(3, nstate)
        out = _call(s, state, F, chunk, lengths, reset=reset, emit=emit, bufs=bufs)
        torch.cuda.synchronize()
        for name, (buf, _, outside) in g.items.items():
            GB.assert_untouched(buf, outside, name)
        return state, out

    g1 = GB.Guards(DEV)
    state, out = call(g1, None, True, 0, [5, 0, 3], [1, 0, 1], [1, 0, 1])
    idle = torch.full((nstate // 4,), float("nan"), dtype=torch.float32, device=DEV).view(torch.uint8)
    assert torch.equal(state[1], idle)                           # the idle slot's slab was neither read into a result nor written
    for name, x in zip(outs, out):
        assert bool((x[1] == GB.sentinel_of(x.dtype)).all()), f"{name}: the idle slot's output row was written"
    assert out[5].cpu().tolist()[0::2] == [-1, -1]
    keep = [x.clone() for x in out]
    for x in keep:
        x[1] = 0
    assert bool(torch.isfinite(keep[2]).all()) and bool(torch.isfinite(keep[3]).all())
    _same(_norm(keep, F), _whole(s, lp, [5, 0, 3], width=F), rows=[0, 2])
    g2 = GB.Guards(DEV)
    _, out = call(g2, state, False, 5, [4, 0, 0], None, [1, 0, 0])
    GB.assert_untouched(g1.items["state"][0], g1.items["state"][2], "state")
    assert torch.equal(state[1], idle)
    assert int(out[5][0]) == -1
    for name, x in zip(outs, out):
        assert bool((x[1:] == GB.sentinel_of(x.dtype)).all()), f"{name}: an idle slot's output row was written"
    keep = [x.clone() for x in out]
    for x in keep:
        x[1:] = 0
    _same(_norm(keep, F), _whole(s, lp, [9, 0, 0], width=F), rows=[0])


def test_damaged_lm_block_is_clamped(arpa):
    """Mid-stream, stored ctx values become n_entries and -5 and one plen -3 (offsets from the documented layout: header 16 B, beam
    block 80 K, then lm K f64 | ps K f64 | ctx 4 x K i32 | plen K i32).  prob / backoff are slices of NaN-filled buffers, so a
    ctx that reached lm_backoff unclamped would read a NaN next to the table -- allocated memory -- and show in the outputs.  The
    run must equal one whose slab had -1 / 0 in those places."""
    s = _searcher(arpa(4, **RICH), **dict(D.RECIPE, topk=5))
    K, n_entries = s.beam_size, int(s.lm.tables(DEV)["prob"].numel())
    lm = dict(s.lm.tables(DEV))
    pad = 64
    for name in ("prob", "backoff"):
        big = torch.full((n_entries + 2 * pad,), float("nan"), device=DEV)
        big[pad:pad + n_entries] = lm[name]
        lm[name] = big[pad:pad + n_entries]
        assert lm[name].is_contiguous() and lm[name].numel() == n_entries
    lp = _batch(D.competing, [40, 40], T, 100).to(DEV)
    clean = s.make_state(2, DEV)
    _feed(s, clean, lp, [24, 24], (24,))
    live = clean.slab[:, :4].contiguous().view(torch.int32)[:, 0].tolist()
    assert min(live) >= 4, live                                # enough live beams to damage some and leave others
    hurt, mended = clean.slab.clone(), clean.slab.clone()
    for slab, (over, under, plen) in ((hurt, (n_entries, -5, -3)), (mended, (-1, -1, 0))):
        for b in range(2):
            ctx = slab[b, 16 + 96 * K:16 + 112 * K].view(torch.int32).view(4, K)
            pl = slab[b, 16 + 112 * K:16 + 116 * K].view(torch.int32)
            nb = live[b]
            ctx[0, 0:nb:2] = over                              # every other live beam, the best one included: its unigram context
            ctx[1, 0:nb:2] = over
            ctx[0, 1:nb:4] = under
            ctx[1, 1:nb:4] = under
            pl[2] = plen
    assert not torch.equal(hurt, mended)
    outs = []
    for slab in (hurt, mended):
        out = _call(s, slab, T, lp[:, 24:40], [16, 16], emit=[1, 1], lm=lm)
        assert out[5].cpu().tolist() == [-1, -1]
        got = _norm(out)
        assert min(got[4].tolist()) >= 1
        assert bool(torch.isfinite(got[2]).all()) and bool(torch.isfinite(got[3]).all())
        outs.append(got)
    _same(outs[0], outs[1])


def test_step_captured_in_a_graph(arpa):
    s = _searcher(arpa(4, **RICH), **dict(D.RECIPE, topk=3))
    lp = _batch(D.competing, [40] * 3, T, 15).to(DEV)
    eager = s.make_state(3, DEV)
    _feed(s, eager, lp, [40] * 3, (8,) * 5)
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
    for i in range(5):
        static.copy_(lp[:, 8 * i:8 * i + 8])
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(state.slab, eager.slab)
    _same(_emit(s, state)[0], _emit(s, eager)[0])
    _same(_emit(s, state)[0], _whole(s, lp, [T] * 3))


def test_end_to_end_with_the_streamed_encoder(arpa):
    """Causal ConMambaASR (2 layers, d_model 256, 31 outputs) in bf16, 2 streams, 48 front-end rows in chunks of 16 through
    log_probs_streaming and step: the hypotheses are CTCBeamSearcher(kenlm_model_path=...)'s on the concatenation of the streamed
    log-probs, texts, score and lm_score bits, at the end and after chunk 2."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    cfg = ASRConfig("c", d_model=256, d_ffn=1024, num_encoder_layers=2, n_fft=400, causal=True, output_neurons=31, seed=5)
    model = ConMambaASR(cfg).to(DEV).eval()
    rows = torch.randn(2, 48, 20, 32, generator=torch.Generator().manual_seed(9)).to(DEV)
    ctx = model.Transformer.make_streaming_context(None, dict(batch_size=2, dtype=torch.bfloat16))
    kw = dict(blank_index=0, beam_size=16, beam_prune_logp=-12.0, token_prune_min_logp=-4.0, prune_history=False, topk=3)
    path = arpa(4, **RICH)
    s = _searcher(path, max_frames=64, **kw)
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
    whole = _whole_searcher(path, **kw)
    cat = torch.cat(lps, dim=1)
    assert _texts(s.hypotheses(state)) == _texts(whole(cat))
    assert _texts(mid) == _texts(whole(cat[:, :32]))
    assert all(len(h) >= 1 for h in s.hypotheses(state))
