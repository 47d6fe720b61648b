"""S2S search on the stepped Transformer decoder without a GPU (modules/Transformer.py, s2s_decode.py): the greedy
and the beam searcher (with and without the CTC scorer) on ``decode_step`` -- the torch routes, an fp64 model -- against slow
restatements that re-run ``TransformerASR.decode`` on every whole prefix (tests/s2s_beam_ref.beam_search for the beam).

The searchers round every step's logits to fp32 before the log-softmax and sum scores in fp32, so the restatements do the same on
``decode``'s fp64 logits.  The two sides' logits differ by the stepped route's distance from the full forward (<= 1e-10,
tests/test_transformer_decoder.py), which can move an fp32 rounding by one ulp; a log-probability of magnitude below 16 then
moves by a few ulps of 2^-20.  TOL = 1e-5 per increment (10 such ulps), times the number of steps for a summed score.  The seeds
are the first from 0 upward at which every choice of the restatement is clear of that: the gap between the candidates at the
selection boundary of every step, and between consecutive final scores, is at least 100 x TOL (asserted, no step skipped).
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_prefix_ref as C  # noqa: E402
import s2s_beam_ref as R  # noqa: E402

CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
V, D, H, FFN, BOS, EOS, BEAM, W_CTC = 14, 32, 2, 48, 1, 2, 3, 0.4
U, T, MIN_RATIO, MAX_RATIO = 2, 10, 0.2, 0.6
TOL = 1e-5
GREEDY_SEED, BEAM_SEED, JOINT_SEED = 0, 0, 1        # joint: seed 0 has a final-score gap of 7.7e-4
_CASES = {}


def _case(seed):
    """-> (transformer, seq_lin, ctc_lin) in fp64 on the torch routes, encoder states (U, T, D), relative lengths"""
    if seed not in _CASES:
        from mamba_asr_amd import ops, sb_compat as sb
        from mamba_asr_amd.modules.TransformerASR import TransformerASR
        torch.manual_seed(seed)
        tr = TransformerASR(tgt_vocab=V, input_size=8, d_model=D, nhead=H, num_encoder_layers=1, num_decoder_layers=2, d_ffn=FFN,
                            dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="transformer",
                            attention_type="RelPosMHAXL", normalize_before=True, causal=False, mamba_config=dict(CFG))
        seq_lin, ctc_lin = sb.Linear(input_size=D, n_neurons=V), sb.Linear(input_size=D, n_neurons=V)
        with torch.no_grad():
            for p in list(tr.decoder.parameters()) + list(seq_lin.parameters()) + list(ctc_lin.parameters()):
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
            seq_lin.w.weight.mul_(4.0)                            # sharper token distributions: clearer choices
            ctc_lin.w.weight.mul_(4.0)
        tr.decoder.attn_fn, tr.decoder.xattn_fn, tr.decoder.initial_capacity = ops.attn_step_torch, ops.xattn_step_torch, 2
        enc = torch.randn(U, T, D, dtype=torch.float64)
        _CASES[seed] = (tr.double().eval(), seq_lin.double().eval(), ctc_lin.double().eval(), enc, torch.tensor([1.0, 0.7]))
    return _CASES[seed]


def _limits(wav_lens):
    enc_lens = [round(T * r) for r in wav_lens.tolist()]
    return enc_lens, [int(MIN_RATIO * e) for e in enc_lens], int(MAX_RATIO * max(enc_lens))


def _att(tr, seq_lin, enc, enc_lens, u, prefix):
    """The decoder's fp32 log-probabilities after ``prefix`` (a list starting with <bos>), from decode() on the whole prefix with
    the padded memory frames of utterance u masked."""
    with torch.no_grad():
        pred, _ = tr.decode(torch.tensor([prefix]), enc[u:u + 1], torch.tensor([enc_lens[u]]))
        return torch.log_softmax(seq_lin(pred)[0, -1].float(), dim=-1)


def _args():
    return dict(bos_index=BOS, eos_index=EOS, min_decode_ratio=MIN_RATIO, max_decode_ratio=MAX_RATIO)


def test_greedy_search_equals_decode_on_every_whole_prefix():
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher
    tr, seq_lin, _, enc, wav_lens = _case(GREEDY_SEED)
    enc_lens, floors, cap = _limits(wav_lens)
    poisoned = enc.clone()
    poisoned[1, enc_lens[1]:] = float("nan")                      # the searcher hands enc_lens to init_decode_state: never read
    hyps, lengths, scores, log_probs = S2SGreedySearcher(modules=[tr, seq_lin], **_args())(poisoned, wav_lens)
    assert bool(torch.isfinite(scores).all())
    gap = float("inf")
    for u in range(U):
        prefix, total, incs = [BOS], np.float32(0), []
        for t in range(cap):
            lp = _att(tr, seq_lin, enc, enc_lens, u, prefix)
            if floors[u] > t:
                lp[EOS] = float("-inf")
            top = torch.topk(lp, 2).values
            gap = min(gap, float(top[0] - top[1]))
            c = int(lp.argmax())
            total = np.float32(total + np.float32(lp[c]))
            incs.append(float(lp[c]))
            if c == EOS:
                break
            prefix.append(c)
        print(f"utterance {u}: {hyps[u]} / restatement {prefix[1:]}, score {float(scores[u]):.6f} / {float(total):.6f}")
        assert hyps[u] == prefix[1:] and int(lengths[u]) == len(prefix) - 1
        assert abs(float(scores[u]) - float(total)) <= TOL * len(incs)
        got = log_probs[u, :len(incs)].double()
        assert float((got - torch.tensor(incs, dtype=torch.float64)).abs().max()) <= TOL
        assert bool((log_probs[u, len(incs):] == 0).all())
    print(f"seed {GREEDY_SEED}: smallest gap between the two best tokens {gap:.3e} (needed {100 * TOL:.1e})")
    assert gap >= 100.0 * TOL, "the case must keep every choice of the restatement clear of the tolerance"


@pytest.mark.parametrize("joint", [False, True], ids=["attention_alone", "joint_ctc"])
def test_beam_three_equals_the_slow_restatement_on_decode(joint):
    from mamba_asr_amd.s2s_decode import S2SBeamSearcher
    seed = JOINT_SEED if joint else BEAM_SEED
    tr, seq_lin, ctc_lin, enc, wav_lens = _case(seed)
    enc_lens, floors, cap = _limits(wav_lens)
    kw = dict(ctc_weight=W_CTC, ctc_scorer=C.RefCTCPrefixScorer(0, EOS, np.float64)) if joint else {}
    searcher = S2SBeamSearcher(modules=[tr, seq_lin, ctc_lin], beam_size=BEAM, topk=BEAM, select_fn=R.select, **kw, **_args())
    assert searcher._init_takes_lens
    hyps, lengths, scores, log_probs = searcher(enc, wav_lens)
    with torch.no_grad():
        ctc_logp = torch.log_softmax(ctc_lin(enc).float(), dim=-1)
    ref64 = C.RefCTCPrefixScorer(0, EOS, np.float64)
    gap, final = float("inf"), float("inf")
    for u in range(U):
        states = {(): ref64.init(ctc_logp[u:u + 1], [enc_lens[u]])}

        def state(g):
            if g not in states:
                states[g] = ref64.advance(state(g[:-1]), torch.tensor([g[-1]]))
            return states[g]

        def logp(prefix):
            att = _att(tr, seq_lin, enc, enc_lens, u, prefix)
            if not joint:
                return att
            return att + W_CTC * ref64.score(state(tuple(prefix[1:])))[0].float()    # fp32: two separately rounded operations

        ranked, gaps, steps = R.beam_search(logp, V, BEAM, BOS, EOS, floors[u], cap, True, BEAM, np.float32)
        gap = min([gap] + gaps)
        final = min([final] + [float(a[1] - b[1]) for a, b in zip(ranked, ranked[1:])])
        print(f"utterance {u}: {hyps[u]} / restatement {[h[0] for h in ranked]}")
        assert len(ranked) == BEAM and hyps[u] == [h[0] for h in ranked]
        assert lengths[u].tolist() == [len(h[0]) for h in ranked]
        sdiff = max(abs(float(scores[u, i]) - float(h[1])) for i, h in enumerate(ranked))
        incs = torch.tensor([float(x) for x in ranked[0][3]], dtype=torch.float64)
        idiff = float((log_probs[u, :len(incs)].double() - incs).abs().max())
        print(f"  max|score - restatement| {sdiff:.3e}, max|increment - restatement| {idiff:.3e}")
        assert sdiff <= TOL * cap and idiff <= TOL
    print(f"seed {seed}: smallest candidate gap {gap:.3e}, smallest final-score gap {final:.3e} (needed {100 * TOL:.1e})")
    assert gap >= 100.0 * TOL and final >= 100.0 * TOL, "the case must keep every choice of the restatement clear of the tolerance"


def test_a_users_init_fn_keeps_its_one_argument_call_and_mamba_is_unchanged():
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher
    tr, seq_lin, _, enc, wav_lens = _case(GREEDY_SEED)
    seen = []

    def init_fn(enc_states):                                      # one positional argument, as before
        seen.append(enc_states.shape)
        return tr.init_decode_state(enc_states)

    searcher = S2SGreedySearcher(modules=[tr, seq_lin], init_fn=init_fn, **_args())
    assert not searcher._init_takes_lens
    all_frames = searcher(enc, wav_lens)
    masked = S2SGreedySearcher(modules=[tr, seq_lin], **_args())(enc, wav_lens)
    assert seen == [enc.shape]
    assert all_frames[0][0] == masked[0][0] and torch.equal(all_frames[2][:1], masked[2][:1])   # full-length utterance: the same
    assert not torch.equal(all_frames[2][1:], masked[2][1:])                                     # the short one sees its padding

    class Mamba:                                                  # what a TransformerASR with the Mamba decoder looks like from here
        decoder_module = "mamba"

        def init_decode_state(self, enc_states):
            return None
    assert not S2SGreedySearcher(modules=[Mamba(), seq_lin], **_args())._init_takes_lens
