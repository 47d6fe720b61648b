"""TransformerLM fusion on the GPU:
  * the stepped language model (modules/TransformerLM.py on ops.attn_step, and on ops.attn_step_torch: the CM_ATTN_STEP=0 route)
    under scripted reorders against the fp64 full forward of every row's prefix
  * S2S beam search with the CTC scorer and the LM scorer end to end against tests/s2s_beam_ref.beam_search in fp64, on the tiny
    seeded S2S model of tests/test_s2s_beam_gpu.py
"""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_prefix_ref as C  # noqa: E402
import s2s_beam_ref as R  # noqa: E402
from test_s2s_beam_gpu import E2E_SEED, _tiny_model  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
V, D, H, LAYERS, FFN = 50, 64, 2, 2, 128
W_CTC, W_LM, LM_TEMP, BEAM = 0.4, 0.6, 1.15, 3
# LM seed of the end-to-end case: the first seed from 1 upward at which the fp64 reference's own choices are clear, i.e. at every step
# of every utterance its BEAM-th and (BEAM + 1)-th candidates, and the consecutive final scores of its best 3 hypotheses, lie at
# least 100 x the tolerance apart (asserted in the test, no step skipped).  Measured on the MI355X: seed 1 has fp32 restatement error
# 7.10e-6 (tolerance 2.84e-5), smallest candidate gap 8.67e-3 and smallest final-score gap 2.92e-3 against 2.84e-3 needed.
LM_SEED = 1
_LMS = {}


def _tiny_lm(seed):
    """-> (the LM on the GPU in fp32, its fp64 copy on the host)"""
    if seed not in _LMS:
        from mamba_asr_amd.modules.TransformerLM import TransformerLM
        torch.manual_seed(seed)
        lm = TransformerLM(V, d_model=D, nhead=H, num_encoder_layers=LAYERS, d_ffn=FFN, initial_capacity=4)
        with torch.no_grad():
            for p in lm.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
        lm = lm.eval()
        _LMS[seed] = (copy.deepcopy(lm).to(DEV), copy.deepcopy(lm).double())
    return _LMS[seed]


ROWS = [[0, 0, 1, 3, 4, 5], [0, 1, 2, 3, 4, 5], [5, 4, 3, 2, 1, 0], [2, 2, 2, 0, 1, 1], [1, 0, 3, 2, 5, 4], [3, 3, 0, 0, 5, 1],
        [4, 4, 4, 4, 4, 4]]
_STEP_REF = {}


def _stepped(lm, attn_fn, autocast):
    """7 steps of 6 rows with the scripted reorders -> per step the logits (6, V) fp64 on the host, and each row's prefix"""
    from mamba_asr_amd import ops
    lm.attn_fn = attn_fn
    gen = torch.Generator().manual_seed(11)
    out, prefixes, hist = [], [[] for _ in range(6)], []
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        state = lm.init_state(6, len(ROWS))
        for t, rows in enumerate(ROWS):
            tokens = torch.randint(0, V, (6,), generator=gen)
            out.append(lm.step(tokens.to(DEV), state).double().cpu())
            prefixes = [p + [int(c)] for p, c in zip(prefixes, tokens)]
            hist.append([list(p) for p in prefixes])
            state = state.reorder(torch.tensor(rows, device=DEV))
            prefixes = [list(prefixes[i]) for i in rows]
    lm.attn_fn = ops.attn_step
    assert state.capacity == 8 and state.kc[0].dtype == (torch.bfloat16 if autocast else torch.float32)
    return out, hist


@pytest.mark.parametrize("mode", ["fp32", "autocast_bf16"])
def test_stepped_lm_matches_the_fp64_full_forward(mode):
    """Tolerance: 4 x the distance of the torch route's logits (ops.attn_step_torch in the same step) from fp64, and not less than
    one fp32 ulp at max|reference logit|."""
    from mamba_asr_amd import ops
    lm, lm64 = _tiny_lm(3)
    assert lm.attn_fn is ops.attn_step                              # the default route is the native kernel
    native, hist = _stepped(lm, ops.attn_step, mode != "fp32")
    base, hist2 = _stepped(lm, ops.attn_step_torch, mode != "fp32")
    assert hist == hist2
    if "ref" not in _STEP_REF:
        with torch.no_grad():
            _STEP_REF["ref"] = [torch.stack([lm64(torch.tensor([p]))[0, -1] for p in step]) for step in hist]
    ref = _STEP_REF["ref"]
    top = max(float(r.abs().max()) for r in ref)
    d_torch = max(float((b - r).abs().max()) for b, r in zip(base, ref))
    d_native = max(float((n - r).abs().max()) for n, r in zip(native, ref))
    tol = max(4.0 * d_torch, 2.0 ** (math.floor(math.log2(top)) - 23))
    print(f"{mode}: |native - fp64| {d_native:.3e}, |torch route - fp64| {d_torch:.3e}, tolerance {tol:.3e}, max|logit| {top:.3f}")
    assert not any(bool(torch.isnan(n).any()) for n in native)
    assert d_native <= tol


# --------------------------------------------------------------------------------------------------------------- end to end
def _reference(lm_seed):
    """-> per utterance (ranked, gaps, steps) of R.beam_search in fp64 with the CTC and the LM term in its callback, the fp32
    restatement's largest distance from fp64 over the added terms met on the way, and the case"""
    cfg, model, wavs, lens = _tiny_model(E2E_SEED)
    lm, lm64 = _tiny_lm(lm_seed)
    lm32 = copy.deepcopy(lm64).float()
    with torch.no_grad():
        enc = model.encode(wavs, lens)
        ctc_logp = torch.log_softmax(model.ctc_lin(enc).float(), dim=-1).cpu()
    T = enc.shape[1]
    enc_lens = [round(T * r) for r in lens.tolist()]
    cap = int(cfg.max_decode_ratio * max(enc_lens))
    floors = [int(cfg.min_decode_ratio * e) for e in enc_lens]
    r64, r32 = C.RefCTCPrefixScorer(0, cfg.eos_index, np.float64), C.RefCTCPrefixScorer(0, cfg.eos_index, np.float32)
    err32, out = [0.0], []
    for b in range(len(enc_lens)):
        states = {(): (r64.init(ctc_logp[b:b + 1], [enc_lens[b]]), r32.init(ctc_logp[b:b + 1], [enc_lens[b]]))}

        def state(g):
            if g not in states:
                s64, s32 = state(g[:-1])
                states[g] = (r64.advance(s64, torch.tensor([g[-1]])), r32.advance(s32, torch.tensor([g[-1]])))
            return states[g]

        def logp(prefix):
            with torch.no_grad():
                pred, _ = model.Transformer.decode(torch.tensor([prefix], device=DEV), enc[b:b + 1])
                att = torch.log_softmax(model.seq_lin(pred)[0, -1].float(), dim=-1).double().cpu()
                l64 = torch.log_softmax(lm64(torch.tensor([prefix]))[0, -1] / LM_TEMP, dim=-1)
                l32 = torch.log_softmax(lm32(torch.tensor([prefix]))[0, -1] / LM_TEMP, dim=-1)
            s64, s32 = state(tuple(prefix[1:]))
            d64, d32 = r64.score(s64)[0], r32.score(s32)[0]
            fin = torch.isfinite(d64)
            assert torch.equal(fin, torch.isfinite(d32))
            add64 = W_CTC * d64 + W_LM * l64
            add32 = (np.float32(W_CTC) * d32.float() + np.float32(W_LM) * l32).double()
            err32[0] = max(err32[0], float((add64[fin] - add32[fin]).abs().max()))
            return att + add64

        out.append(R.beam_search(logp, V, BEAM, cfg.bos_index, cfg.eos_index, floors[b], cap, True, BEAM, np.float64))
    return out, err32[0], (cfg, model, wavs, lens, lm)


def _margins(ref):
    gap = min(g for ranked, gaps, _ in ref for g in gaps)
    final = min(float(a[1] - b[1]) for ranked, _, _ in ref for a, b in zip(ranked, ranked[1:]))
    return gap, final


def test_beam_three_with_ctc_and_lm_matches_the_slow_fp64_reference():
    """Tolerance per increment: 4 x the fp32 restatement's own distance from fp64 over the added terms (the rule of
    tests/test_s2s_beam_gpu.py); a summed score gets that times the number of steps."""
    from mamba_asr_amd.s2s_decode import TransformerLMScorer
    ref, err32, (cfg, model, wavs, lens, lm) = _reference(LM_SEED)
    scorer = TransformerLMScorer(lm, temperature=LM_TEMP)
    hyps, lengths, scores, log_probs = model.transcribe_s2s(wavs, lens, ctc_weight=W_CTC, beam_size=BEAM, topk=BEAM,
                                                            lm_scorer=scorer, lm_weight=W_LM)
    plain = model.transcribe_s2s(wavs, lens, ctc_weight=W_CTC, beam_size=BEAM, topk=BEAM)
    tol = 4.0 * err32
    gap, final = _margins(ref)
    steps = log_probs.shape[1]
    print(f"LM seed {LM_SEED}: fp32 restatement error {err32:.3e}, tolerance {tol:.3e}, smallest candidate gap {gap:.3e}, "
          f"smallest final-score gap {final:.3e}, steps {steps}")
    assert err32 > 0 and all(len(ranked) == BEAM for ranked, _, _ in ref)
    assert gap >= 100.0 * tol and final >= 100.0 * tol, "the case must keep every reference choice clear of the tolerance"
    assert steps == max(s for _, _, s in ref)
    for u, (ranked, _, _) in enumerate(ref):
        print(f"utterance {u}: {hyps[u]} / reference {[h[0] for h in ranked]}")
        assert hyps[u] == [h[0] for h in ranked]
        assert lengths[u].tolist() == [len(h[0]) for h in ranked]
        sdiff = max(abs(float(scores[u, i]) - float(h[1])) for i, h in enumerate(ranked))
        incs = torch.tensor([float(x) for x in ranked[0][3]], dtype=torch.float64)
        idiff = float((log_probs[u, :len(incs)].double().cpu() - incs).abs().max())
        print(f"  max|score - reference| {sdiff:.3e} (allowed {tol * steps:.3e}), max|increment - reference| {idiff:.3e} (allowed {tol:.3e})")
        assert sdiff <= tol * steps and idiff <= tol
        assert bool((log_probs[u, len(incs):] == 0).all())
        assert float(scores[u, 0]) != float(plain[2][u, 0]), "the LM term must take part in the best hypothesis's score"


def test_lm_alone_uses_the_selection_weight():
    """Without CTC the LM log-probabilities are the selection's delta at weight lm_weight: the native and the torch selection agree."""
    from mamba_asr_amd.s2s_decode import S2SBeamSearcher, TransformerLMScorer, select_torch
    cfg, model, wavs, lens = _tiny_model(E2E_SEED)
    lm, _ = _tiny_lm(LM_SEED)
    scorer = TransformerLMScorer(lm, temperature=LM_TEMP)
    got = model.transcribe_s2s(wavs, lens, beam_size=BEAM, topk=BEAM, lm_scorer=scorer, lm_weight=W_LM)
    args = dict(bos_index=cfg.bos_index, eos_index=cfg.eos_index, min_decode_ratio=cfg.min_decode_ratio,
                max_decode_ratio=cfg.max_decode_ratio)
    other = S2SBeamSearcher(modules=[model.Transformer, model.seq_lin], beam_size=BEAM, topk=BEAM, lm_scorer=scorer, lm_weight=W_LM,
                            select_fn=select_torch, **args)
    want = model.transcribe_s2s(wavs, lens, searcher=other)
    plain = model.transcribe_s2s(wavs, lens, beam_size=BEAM, topk=BEAM)
    assert got[0] == want[0] and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
    assert not torch.equal(got[2], plain[2])
