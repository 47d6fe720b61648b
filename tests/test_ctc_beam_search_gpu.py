"""GPU checks of the CTC beam search (csrc/ctc_beam.hip behind mamba_asr_amd.ctc_decode.CTCBeamSearcher) against the tests'
float64 host restatement (tests/ctc_beam_ref.py) and fp64 torch CTC."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_beam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INF = math.inf


def _searcher(**kw):
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    return CTCBeamSearcher(**kw)


def _rel(lengths, T):
    return torch.tensor([n / T for n in lengths], dtype=torch.float32)


def _ref(s, lp, n):
    return R.beam_search(lp.double().tolist(), n, s.vocab_list, blank=s.blank_index, beam_size=s.beam_size,
                         beam_prune_logp=s.beam_prune_logp, token_prune_min_logp=s.token_prune_min_logp,
                         prune_history=s.prune_history, blank_skip_threshold=s.blank_skip_threshold, topk=s.topk,
                         space_token=s.space_token, spm_token=s.spm_token)


def _match(got, want, tol=1e-9):
    """Same texts in the same order, scores within tol; a swap only between entries whose reference scores differ < tol."""
    assert len(got) == len(want), (len(got), len(want))
    wmap = dict(want)
    assert {h.text for h in got} == set(wmap)
    for i, h in enumerate(got):
        assert abs(h.score - wmap[h.text]) <= tol, (i, h.text, h.score, wmap[h.text])
        assert h.lm_score == h.score and h.last_lm_state is None and h.text_frames is None
        if h.text != want[i][0]:
            assert abs(wmap[h.text] - want[i][1]) < tol, (i, h.text, want[i][0])


def _batch(gen, lengths, T, V, seed):
    lp = torch.full((len(lengths), T, V), -50.0)
    for b, n in enumerate(lengths):
        if n:
            lp[b, :n] = gen(n, V, seed + b)
    return lp


@pytest.mark.parametrize("regime", ["peaky", "competing"])
def test_recipe_settings_match_restatement(regime):
    gen = D.peaky if regime == "peaky" else D.competing
    s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, topk=10)
    lengths = [1, 2, 17, 160, 421, 1000]
    T = max(lengths)
    lp = _batch(gen, lengths, T, 31, 100)
    hyps = s(lp.to(DEV), _rel(lengths, T))
    assert len(hyps) == len(lengths)
    for b, n in enumerate(lengths):
        _match(hyps[b], _ref(s, lp[b], n))
    if regime == "competing":
        assert len(hyps[-1]) == 10


@pytest.mark.parametrize("beam,prune_history", [(100, True), (100, False), (12, True)])
def test_all_candidates_live(beam, prune_history):
    """token_prune_min_logp = -inf: every (beam, token) pair is a candidate (beam 100 x 31 > the in-LDS capacity: the
    workspace path; beam 12: in LDS), frames skipped on a high blank, topk above the survivors, an empty utterance."""
    g = torch.Generator().manual_seed(7)
    T, V = 14, 31
    logits = torch.randn(3, T, V, generator=g) * 0.4
    logits[:, 3::4, 0] += 6.0                              # p(blank) > 0.5 on these frames: skipped under threshold 0.5
    lp = torch.log_softmax(logits, dim=-1)
    s = _searcher(blank_index=0, vocab_list=D.SPM_VOCAB, beam_size=beam, beam_prune_logp=-INF, token_prune_min_logp=-INF,
                  prune_history=prune_history, blank_skip_threshold=0.5, topk=300)
    lengths = [T, 0, 9]
    hyps = s(lp.to(DEV), _rel(lengths, T))
    for b, n in enumerate(lengths):
        want = _ref(s, lp[b], n)
        _match(hyps[b], want)
        if n:
            assert len(want) < 300
    assert [(h.text, h.score) for h in hyps[1]] == [("", 0.0)]


def test_exact_ctc_likelihood_on_gpu():
    vocab = ["<b>", "a", "b", "c"]
    T = 5
    lp = torch.log_softmax(torch.randn(2, T, 4, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 1.5, -1)
    lp32 = lp.float()
    s = _searcher(blank_index=0, vocab_list=vocab, beam_size=256, beam_prune_logp=-INF, token_prune_min_logp=-INF,
                  prune_history=False, topk=256)
    # 256 beams hold every (prefix, last label) here: the unlimited restatement agrees with the 256-beam one
    assert _ref(s, lp32[0], T) == R.beam_search(lp32[0].double().tolist(), T, vocab, beam_size=10 ** 9,
                                                beam_prune_logp=-INF, token_prune_min_logp=-INF, topk=10 ** 9)
    hyps = s(lp32.to(DEV))
    for b in range(2):
        assert len(hyps[b]) > 50
        for h in hyps[b]:
            tg = torch.tensor([vocab.index(c) for c in h.text], dtype=torch.long)
            nll = F.ctc_loss(lp32[b].double().unsqueeze(1), tg, torch.tensor([T]), torch.tensor([len(tg)]), blank=0,
                             reduction="none")
            assert abs(-nll.item() - h.score) <= 1e-12, (h.text, h.score, -nll.item())


def test_greedy_equivalence_on_model_output():
    from mamba_asr_amd import dataio
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = ASRConfig("tiny", d_model=64, d_ffn=128, num_encoder_layers=2, n_fft=400, seed=11)
    model = ConMambaASR(cfg).to(DEV).eval()
    wavs, lens = synthetic_wavs(3, samples_for_frames(320), 4, DEV)
    with torch.no_grad():
        model.calibrate(wavs, lens)
        p_ctc = model.forward_ctc(wavs, lens)
    assert p_ctc.shape[2] == 31
    s = _searcher(blank_index=0, vocab_list=D.SPM_VOCAB, beam_size=1, token_prune_min_logp=0.0, beam_prune_logp=-12.0,
                  prune_history=False)
    hyps = s(p_ctc, lens)
    greedy = dataio.ctc_greedy_decode(p_ctc, lens, blank_id=0)
    assert any(greedy)
    for b in range(3):
        assert hyps[b][0].text == s.compose(greedy[b])


def _raw(s, lp, rel):
    """The kernel's raw outputs (tokens, lengths, scores, counts) for bitwise comparisons."""
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    T = lp.shape[1]
    n = torch.tensor(s.frame_counts(T, rel, lp.shape[0]), dtype=torch.int32, device=DEV)
    tc, th, tp = s._tables(DEV)
    out = ops.ctc_beam_search(lp, n, tc, th, tp, HASH_BASE, HASH_SEP, blank=s.blank_index, beam_size=s.beam_size,
                              topk=s.topk, prune_history=s.prune_history, beam_prune_logp=s.beam_prune_logp,
                              token_prune_min_logp=s.token_prune_min_logp)
    tokens, tlen, scores, nh, bad = [x.cpu() for x in out]
    for b in range(tokens.shape[0]):                      # positions past a hypothesis' length are not outputs
        for h in range(tokens.shape[1]):
            tokens[b, h, tlen[b, h] if h < nh[b] else 0:] = 0
    return tokens, tlen, scores, nh, bad


def test_properties_bitwise():
    s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, topk=5)
    lengths = [300, 120, 300, 1, 250]
    T = 300
    lp = torch.cat([_batch(D.competing, lengths[:3], T, 31, 40), _batch(D.peaky, lengths[3:], T, 31, 50)])
    rel = _rel(lengths, T)
    bf = lp.bfloat16()
    a = _raw(s, bf.to(DEV), rel)
    up = _raw(s, bf.float().to(DEV), rel)
    for x, y in zip(a, up):
        assert torch.equal(x, y)
    full = _raw(s, lp.to(DEV), rel)
    again = _raw(s, lp.to(DEV), rel)
    for x, y in zip(full, again):
        assert torch.equal(x, y)
    for b in range(len(lengths)):
        alone = _raw(s, lp[b:b + 1].to(DEV), rel[b:b + 1])
        for x, y in zip(full, alone):
            assert torch.equal(x[b:b + 1], y)
    perm = torch.tensor([3, 0, 4, 2, 1])
    pm = _raw(s, lp[perm].to(DEV), rel[perm])
    for x, y in zip(full, pm):
        assert torch.equal(x[perm], y)


def test_nan_raises_naming_the_utterance():
    s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB)
    lp = _batch(D.peaky, [20, 20], 20, 31, 3)
    lp[1, 12, 5] = float("nan")
    with pytest.raises(ValueError, match="utterance 1"):
        s(lp.to(DEV))
    hyps = s(lp.to(DEV), _rel([20, 12], 20))             # the NaN lies past n_b: decoded normally
    _match(hyps[1], _ref(s, lp[1], 12))


def test_recipe_call_sequence_through_brain():
    """train_CTC.py:309-310 (compute_forward calls the searcher in Stage.TEST) and :411-414 (hyp[0].text.split(" "))."""
    from mamba_asr_amd import brain
    searcher = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB)
    lengths = [[200, 140], [90, 200]]
    batches = [(_batch(D.competing, ls, 200, 31, 60 + 2 * i), _rel(ls, 200)) for i, ls in enumerate(lengths)]

    class CTCBrain(brain.Brain):
        words = []

        def compute_forward(self, batch, stage):
            p_ctc, wav_lens = batch[0].to(self.device), batch[1].to(self.device)
            p_tokens = None
            if stage == brain.Stage.TEST:
                p_tokens = searcher(p_ctc, wav_lens)
            return p_ctc, wav_lens, p_tokens

        def compute_objectives(self, predictions, batch, stage):
            p_ctc, wav_lens, predicted_tokens = predictions
            if stage == brain.Stage.TEST:
                self.words.append([hyp[0].text.split(" ") for hyp in predicted_tokens])
            return p_ctc.new_zeros(())

    br = CTCBrain(modules={}, hparams={}, run_opts={"device": "cuda:0"})
    br.evaluate(batches)
    assert len(br.words) == 2
    for (lp, rel), words, ls in zip(batches, br.words, lengths):
        for b, n in enumerate(ls):
            assert words[b] == _ref(searcher, lp[b], n)[0][0].split(" ")


def test_benchmark_shape():
    s = _searcher(**D.RECIPE, vocab_list=D.SPM_VOCAB)
    B, T = 64, 1000
    lp = torch.stack([(D.competing if b % 2 == 0 else D.peaky)(T, 31, 900 + b) for b in range(B)])
    hyps = s(lp.to(DEV))
    assert len(hyps) == B and all(len(h) == 1 for h in hyps)
    for b in range(4):
        _match(hyps[b], _ref(s, lp[b], T))
