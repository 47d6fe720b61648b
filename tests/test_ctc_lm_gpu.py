"""GPU checks of the LM-fused CTC beam search (csrc/ctc_beam_lm.hip behind CTCBeamSearcher(kenlm_model_path=...)) against the
tests' float64 restatement (tests/ctc_lm_ref.py), brute force and the LM-free kernel.  Every comparison with the restatement first
asserts that the restatement's own smallest prune / rank / cut margin on that input exceeds 1e-7: the fixed seeds are chosen so."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_beam_ref as R  # noqa: E402
import ctc_lm_data as LD  # noqa: E402
import ctc_lm_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu
INF = math.inf
TOL, MARGIN = 1e-9, 1e-7
RICH = dict(n_words=(18, 300, 300), n_bigrams=400, n_trigrams=300)        # many short words: prefixes hit, words score
SPARSE = dict(n_words=(3, 3, 3), n_bigrams=8, n_trigrams=4)               # most words absent


def _searcher(**kw):
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    return CTCBeamSearcher(**kw)


def _decode(s, lp, lengths):
    """The searcher on the GPU: absolute lengths."""
    return s(lp.to(torch.device("cuda:0")), lengths=lengths)


def _ref(s, lm, lp, n):
    """The restatement on the values the kernel reads (bf16 inputs widened) -> [(text, acoustic, total)]; asserts its margin."""
    hyps, margin = LR.beam_search_lm(
        lp.float().double().tolist(), n, s.vocab_list, lm, alpha=s.alpha, beta=s.beta, unk_score_offset=s.unk_score_offset,
        score_boundary=s.score_boundary, blank=s.blank_index, beam_size=s.beam_size, beam_prune_logp=s.beam_prune_logp,
        token_prune_min_logp=s.token_prune_min_logp, prune_history=s.prune_history, blank_skip_threshold=s.blank_skip_threshold,
        topk=s.topk, space_token=s.space_token, spm_token=s.spm_token)
    assert margin > MARGIN, margin
    return hyps


def _match(got, want, tol=TOL):
    """Same texts in the same order, acoustic score and total within tol; a swap only between entries whose reference totals
    differ < tol."""
    assert len(got) == len(want), (len(got), len(want))
    wmap = {t: (ac, tot) for t, ac, tot in want}
    assert {h.text for h in got} == set(wmap)
    for i, h in enumerate(got):
        assert abs(h.score - wmap[h.text][0]) <= tol, (i, h.text, h.score, wmap[h.text])
        assert abs(h.lm_score - wmap[h.text][1]) <= tol, (i, h.text, h.lm_score, wmap[h.text])
        assert h.last_lm_state is None and h.text_frames is None
        if h.text != want[i][0]:
            assert abs(wmap[h.text][1] - want[i][2]) < tol, (i, h.text, want[i][0])


def _batch(gen, lengths, T, V, seed):
    lp = torch.full((len(lengths), T, V), -50.0)
    for b, n in enumerate(lengths):
        if n:
            lp[b, :n] = gen(n, V, seed + b)
    return lp


def _check(s, lm, lp, lengths):
    hyps = _decode(s, lp, lengths)
    assert len(hyps) == len(lengths)
    wants = []
    for b, n in enumerate(lengths):
        wants.append(_ref(s, lm, lp[b], n))
        _match(hyps[b], wants[-1])
    return hyps, wants


@pytest.mark.parametrize("variant", [dict(unk=True, bos=True, eos=True), dict(unk=False, bos=False, eos=False)])
def test_exact_likelihood_plus_lm(tmp_path, variant):
    """Pruning off, 256 beams at T = 5, V = 4: every text is returned with (brute-force CTC likelihood, that plus LM(text))."""
    vocab = ["<b>", "▁", "A", "▁B"]
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=31, letters=["A", "B"], n_bigrams=12, n_trigrams=10, **variant)
    lm = LR.DictLM(path)
    T = 5
    lp = torch.log_softmax(torch.randn(2, T, 4, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 1.5, -1).float()
    kw = dict(alpha=0.7, beta=1.1, unk_score_offset=-3.0, score_boundary=True)
    s = _searcher(blank_index=0, vocab_list=vocab, kenlm_model_path=path, beam_size=256, beam_prune_logp=-INF,
                  token_prune_min_logp=-INF, prune_history=False, topk=256, **kw)
    hyps = _decode(s, lp, [T, T])
    for b in range(2):
        rows = lp[b].double().tolist()
        want = R.brute_force(rows, vocab)
        # 256 beams hold every (text, partial, last) here: the unlimited restatement returns the same list
        assert _ref(s, lm, lp[b], T) == LR.beam_search_lm(rows, T, vocab, lm, beam_size=10 ** 9, beam_prune_logp=-INF,
                                                          token_prune_min_logp=-INF, topk=10 ** 9, **kw)[0]
        assert {h.text for h in hyps[b]} == set(want) and len(hyps[b]) == len(want) > 40
        for h in hyps[b]:
            assert abs(h.score - want[h.text]) <= TOL, (h.text, h.score, want[h.text])
            assert abs(h.lm_score - LR.final_total(lm, h.text, want[h.text], **kw)) <= TOL, h.text
        _match(hyps[b], _ref(s, lm, lp[b], T))


@pytest.mark.parametrize("prune_history", [False, True])
def test_neutral_lm_is_the_lm_free_search(tmp_path, prune_history):
    """alpha = beta = unk_score_offset = 0 and no </s>: texts and score bits of the LM-free kernel, lm_score == score."""
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=2, eos=False, **RICH)
    cfg = dict(D.RECIPE, prune_history=prune_history)
    free = _searcher(**cfg, vocab_list=D.SPM_VOCAB, topk=10)
    fused = _searcher(**cfg, vocab_list=D.SPM_VOCAB, topk=10, kenlm_model_path=path, alpha=0.0, beta=0.0, unk_score_offset=0.0)
    lengths = [40, 0, 33]
    lp = torch.cat([_batch(D.competing, lengths[:2], 40, 31, 70), _batch(D.peaky, lengths[2:], 40, 31, 80)])
    a, b = _decode(free, lp, lengths), _decode(fused, lp, lengths)
    assert [len(x) for x in a] == [len(x) for x in b] and len(a[0]) == 10
    for ha, hb in zip(a, b):
        for x, y in zip(ha, hb):
            assert x.text == y.text and x.score == y.score and y.lm_score == y.score, (x, y)


@pytest.mark.parametrize("prune_history", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("regime", ["peaky", "competing"])
def test_recipe_settings_match_restatement(tmp_path, regime, dtype, prune_history):
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=4, **RICH)
    s = _searcher(**dict(D.RECIPE, prune_history=prune_history), vocab_list=D.SPM_VOCAB, topk=10, kenlm_model_path=path)
    assert (s.alpha, s.beta, s.unk_score_offset, s.score_boundary) == (0.5, 1.5, -10.0, True)
    lm = LR.DictLM(path)
    lengths = [40, 0, 29]
    lp = _batch(D.peaky if regime == "peaky" else D.competing, lengths, 40, 31, 100).to(dtype)
    hyps, wants = _check(s, lm, lp, lengths)
    assert [(h.text, h.score) for h in hyps[1]] == [("", 0.0)]
    assert abs(hyps[1][0].lm_score - LR.final_total(lm, "", 0.0, 0.5, 1.5, -10.0, True)) <= 1e-12 and hyps[1][0].lm_score != 0.0
    assert any(h.lm_score != h.score for h in hyps[0])
    if regime == "competing":
        assert len(hyps[0]) == 10


@pytest.mark.parametrize("prune_history", [False, True])
def test_global_sort_path(tmp_path, prune_history):
    """Beam 64 without token pruning at V = 31: 1984 candidates per frame, sorted in the workspace slab."""
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=6, **RICH)
    s = _searcher(blank_index=0, vocab_list=D.SPM_VOCAB, kenlm_model_path=path, beam_size=64, beam_prune_logp=-40.0,
                  token_prune_min_logp=-INF, prune_history=prune_history, topk=20)
    g = torch.Generator().manual_seed(17)
    lp = torch.log_softmax(torch.randn(2, 6, 31, generator=g) * 0.8, dim=-1)
    hyps, wants = _check(s, LR.DictLM(path), lp, [6, 5])
    assert len(hyps[0]) == 20


@pytest.mark.parametrize("order", [1, 2, 5])
def test_other_orders(tmp_path, order):
    """Orders 1, 2 and 5 over a two-letter alphabet, so that hypotheses hold runs of listed words and the longest n-grams hit."""
    vocab = ["<b>", "▁", "A", "▁B"]
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=52 + order, order=order, letters=["A", "B"], n_words=(1, 1, 0), n_bigrams=30,
                           n_trigrams=60, n_more=(90, 120))
    lm = LR.DictLM(path)
    assert lm.order == order
    s = _searcher(blank_index=0, vocab_list=vocab, kenlm_model_path=path, beam_size=64, beam_prune_logp=-INF,
                  token_prune_min_logp=-INF, prune_history=False, topk=64, alpha=0.9, beta=0.3, unk_score_offset=-2.0)
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn(2, 12, 4, generator=g) * 0.7 + torch.tensor([0.0, 0.6, 0.6, 0.6]), dim=-1)
    hyps, wants = _check(s, lm, lp, [12, 11])
    longest = [gram for gram in lm.prob if len(gram) == order]
    texts = [[w if w in lm.vocab else "<unk>" for w in ("<s> " + h.text).split()] for hs in hyps for h in hs]
    assert any(tuple(t[i:i + order]) in longest for t in texts for i in range(len(t))), "no n-gram of the model's order was met"


def test_unknown_words_and_prefix_misses(tmp_path):
    """An LM that lacks most words: unk_score_offset moves the winner, and both settings match the restatement."""
    path, words = LD.make_arpa(tmp_path / "m.arpa", seed=8, **SPARSE)
    lm = LR.DictLM(path)
    lengths = [24, 30]
    lp = _batch(D.competing, lengths, 30, 31, 300)
    tops = {}
    for offset in (-10.0, 0.0):
        s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, topk=5, kenlm_model_path=path, unk_score_offset=offset)
        hyps, wants = _check(s, lm, lp, lengths)
        tops[offset] = [h[0].text for h in hyps]
        assert any(w not in lm.vocab for h in hyps for w in h[0].text.split())
    assert all(x != y for x, y in zip(tops[-10.0], tops[0.0])), tops


@pytest.mark.parametrize("unk", [True, False])
def test_score_boundary_on_and_off(tmp_path, unk):
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=9, unk=unk, **RICH)
    lm = LR.DictLM(path)
    lengths = [36, 21]
    lp = _batch(D.competing, lengths, 36, 31, 500)
    got = {}
    for boundary in (True, False):
        s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, topk=5, kenlm_model_path=path, alpha=0.8, beta=0.5, unk_score_offset=-4.0,
                      score_boundary=boundary)
        got[boundary], _ = _check(s, lm, lp, lengths)
    assert all(x[0].lm_score != y[0].lm_score for x, y in zip(got[True], got[False]))


def test_nan_raises_naming_the_utterance(tmp_path):
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=4, **RICH)
    s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path)
    lp = _batch(D.peaky, [20, 20], 20, 31, 3)
    lp[1, 12, 5] = float("nan")
    with pytest.raises(ValueError, match="utterance 1"):
        _decode(s, lp, [20, 20])
    hyps = s(lp.to(torch.device("cuda:0")), torch.tensor([1.0, 0.6]))       # wav_lens: the NaN lies past n_b = 12, decoded normally
    _match(hyps[1], _ref(s, LR.DictLM(path), lp[1], 12))
