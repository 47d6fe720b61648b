"""S2S beam search end to end on the GPU (mamba_asr_amd.s2s_decode.S2SBeamSearcher on ops.beam_select), on the tiny
seeded S2S model of tests/test_ctc_prefix_gpu.py:
  * beam 1 without length normalisation IS the greedy searcher, bit for bit, with and without the CTC term -- which holds on a real
    model only because the native selection rounds alive + (att + weight * delta) as the greedy searcher's three torch operations do
  * CM_BEAM_SELECT=0 (the torch selection) gives the native route's outputs
  * beam 3 with ctc_weight 0.4 against a slow fp64 reference: tests/s2s_beam_ref.beam_search, every hypothesis scored by the
    full-prefix TransformerASR.decode plus the fp64 host CTC scorer of tests/ctc_prefix_ref.py
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_prefix_ref as C  # noqa: E402
import s2s_beam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEG = -math.inf
W, BEAM = 0.4, 3
# Model seed of the end-to-end case: the first seed from 21 upward at which the fp64 reference's own choices are clear, i.e. at every
# step of every utterance its BEAM-th and (BEAM + 1)-th candidates, and the consecutive final scores of its best 3 hypotheses, lie
# at least 100 x the tolerance apart (asserted in the test, no step skipped).  Measured on the MI355X: seeds 21-39 miss it (21 the
# closest: candidate gap 1.06e-2 but final-score gap 9.42e-3 against 9.85e-3 needed); seed 40 has candidate gap 8.55e-3 and
# final-score gap 8.95e-3 against 6.26e-3 needed (fp32 restatement error 1.56e-5, tolerance 6.26e-5).
E2E_SEED = 40
_CASES = {}


def _tiny_model(seed):
    """The model of tests/test_ctc_prefix_gpu.py: D 128, 2 + 2 layers, V 50, three utterances of 30 / 21 / 12 encoder frames; <eos>
    biased up by 10 so that rows stop at their min_decode_ratio floor (steps 9 / 6 / 3), the cap at 7 steps."""
    if seed in _CASES:
        return _CASES[seed]
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = ASRConfig("s2s_tiny", d_model=128, d_ffn=256, num_encoder_layers=2, num_decoder_layers=2, output_neurons=50, n_fft=400,
                    seed=seed, min_decode_ratio=0.3, max_decode_ratio=0.25)
    model = ConMambaASR(cfg).to(DEV).eval()
    with torch.no_grad():
        model.seq_lin.w.bias[cfg.eos_index] += 10.0
        model.seq_lin.w.bias[cfg.bos_index] -= 10.0
    wavs, _ = synthetic_wavs(3, samples_for_frames(120), 5, DEV)
    lens = torch.tensor([1.0, 0.7, 0.4], device=DEV)
    for i, r in enumerate(lens.tolist()):
        wavs[i, int(round(r * wavs.shape[1])):] = 0.0
    with torch.no_grad():
        model.calibrate(wavs, lens)
    _CASES[seed] = (cfg, model, wavs, lens)
    return _CASES[seed]


@pytest.mark.parametrize("weight", [W, None])
def test_beam_one_is_the_greedy_searcher_bit_for_bit(weight):
    cfg, model, wavs, lens = _tiny_model(E2E_SEED)
    want = model.transcribe_s2s(wavs, lens, ctc_weight=weight)
    got = model.transcribe_s2s(wavs, lens, ctc_weight=weight, beam_size=1, length_normalization=False)
    assert got[0] == want[0] and any(len(h) for h in got[0])
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_temperature_divides_the_logits_of_the_default_step():
    from mamba_asr_amd.s2s_decode import S2SBeamSearcher
    cfg, model, wavs, lens = _tiny_model(E2E_SEED)

    def step_fn(tokens, state):
        logits = model.seq_lin(model.Transformer.decode_step(tokens, state))[:, 0].float()
        return torch.log_softmax(logits / 1.15, dim=-1), state

    explicit = S2SBeamSearcher(modules=[model.Transformer, model.seq_lin, model.ctc_lin], step_fn=step_fn, beam_size=BEAM, topk=BEAM,
                               ctc_weight=W, blank_index=cfg.blank_index, bos_index=cfg.bos_index, eos_index=cfg.eos_index,
                               min_decode_ratio=cfg.min_decode_ratio, max_decode_ratio=cfg.max_decode_ratio)
    want = model.transcribe_s2s(wavs, lens, searcher=explicit)
    got = model.transcribe_s2s(wavs, lens, ctc_weight=W, beam_size=BEAM, topk=BEAM, temperature=1.15)
    plain = model.transcribe_s2s(wavs, lens, ctc_weight=W, beam_size=BEAM, topk=BEAM)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert torch.equal(a, b)
    assert not torch.equal(got[2], plain[2]), "a temperature of 1.15 must change the scores"


_CHILD = """
import sys, torch
sys.path.insert(0, {here!r})
import test_s2s_beam_gpu as T
from mamba_asr_amd import s2s_decode
cfg, model, wavs, lens = T._tiny_model(T.E2E_SEED)
out = model.transcribe_s2s(wavs, lens, ctc_weight=T.W, beam_size=T.BEAM, topk=T.BEAM)
searcher = s2s_decode.S2SBeamSearcher(modules=[model.Transformer, model.seq_lin])
assert searcher.select_fn is s2s_decode.select_torch
torch.save([out[0]] + [t.cpu() for t in out[1:]], {path!r})
"""


def test_torch_selection_route_gives_the_native_outputs(tmp_path):
    cfg, model, wavs, lens = _tiny_model(E2E_SEED)
    want = model.transcribe_s2s(wavs, lens, ctc_weight=W, beam_size=BEAM, topk=BEAM)
    path = str(tmp_path / "child.pt")
    env = dict(os.environ, CM_BEAM_SELECT="0")
    subprocess.run([sys.executable, "-c", _CHILD.format(here=HERE, path=path)], env=env, check=True, timeout=300,
                   cwd=os.path.dirname(HERE))
    got = torch.load(path)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert torch.equal(a, b.cpu())


def _reference(seed):
    """-> per utterance (ranked, gaps, steps) of R.beam_search in fp64, the fp32 restatement's largest distance from fp64 over the
    CTC deltas met on the way, and the case"""
    cfg, model, wavs, lens = _tiny_model(seed)
    assert (cfg.blank_index, cfg.bos_index, cfg.eos_index) == (0, 1, 2)
    with torch.no_grad():
        enc = model.encode(wavs, lens)
        ctc_logp = torch.log_softmax(model.ctc_lin(enc).float(), dim=-1).cpu()
    T, V = enc.shape[1], ctc_logp.shape[2]
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
            s64, s32 = state(tuple(prefix[1:]))
            d64, d32 = r64.score(s64)[0], r32.score(s32)[0].double()
            fin = torch.isfinite(d64)
            assert torch.equal(fin, torch.isfinite(d32))
            err32[0] = max(err32[0], float((d64[fin] - d32[fin]).abs().max()))
            return att + W * d64

        out.append(R.beam_search(logp, V, BEAM, cfg.bos_index, cfg.eos_index, floors[b], cap, True, BEAM, np.float64))
    return out, err32[0], (cfg, model, wavs, lens)


def _margins(ref):
    """-> (smallest candidate gap over all steps, smallest gap between consecutive final scores of the best hypotheses)"""
    gap = min(g for ranked, gaps, _ in ref for g in gaps)
    final = min(float(a[1] - b[1]) for ranked, _, _ in ref for a, b in zip(ranked, ranked[1:]))
    return gap, final


def test_beam_three_joint_decoding_matches_the_slow_fp64_reference():
    """Tolerance per increment: 4 x the fp32 restatement's own distance from fp64 on these posteriors (the rule of the joint-decoding
    test of tests/test_ctc_prefix_gpu.py); a summed score gets that times the number of steps.  Required: the same BEAM token
    lists in the same order, and the scores within tolerance."""
    ref, err32, (cfg, model, wavs, lens) = _reference(E2E_SEED)
    hyps, lengths, scores, log_probs = model.transcribe_s2s(wavs, lens, ctc_weight=W, beam_size=BEAM, topk=BEAM)
    tol = 4.0 * err32
    gap, final = _margins(ref)
    steps = log_probs.shape[1]
    print(f"seed {E2E_SEED}: fp32 restatement error {err32:.3e}, tolerance {tol:.3e}, smallest candidate gap {gap:.3e}, "
          f"smallest final-score gap {final:.3e}, steps {steps}")
    assert err32 > 0 and all(len(ranked) == BEAM for ranked, _, _ in ref)
    assert gap >= 100.0 * tol and final >= 100.0 * tol, "the case must keep every reference choice clear of the tolerance"
    assert steps == max(s for _, _, s in ref)
    assert scores.shape == (3, BEAM) and lengths.shape == (3, BEAM)
    for u, (ranked, _, ref_steps) in enumerate(ref):
        print(f"utterance {u}: {hyps[u]} / reference {[h[0] for h in ranked]}")
        assert hyps[u] == [h[0] for h in ranked]
        assert lengths[u].tolist() == [len(h[0]) for h in ranked]
        sdiff = max(abs(float(scores[u, i]) - float(h[1])) for i, h in enumerate(ranked))
        incs = torch.tensor([float(x) for x in ranked[0][3]], dtype=torch.float64)
        idiff = float((log_probs[u, :len(incs)].double().cpu() - incs).abs().max())
        print(f"  max|score - reference| {sdiff:.3e} (allowed {tol * steps:.3e}), max|increment - reference| {idiff:.3e} (allowed {tol:.3e})")
        assert sdiff <= tol * steps and idiff <= tol
        assert bool((log_probs[u, len(incs):] == 0).all())
