"""The Transformer decoder of the conmamba_{small,large} S2S recipes on the GPU (modules/Transformer.py):
  * the stepped decoder on the native kernels (cm_xattn_step, and cm_attn_step where the head dimension is 32 / 64) under scripted
    reorders against the fp64 full decode() of every row's prefix, at d_model 128 / 4 heads and at the small recipe's 144 / 4
  * transcribe_s2s(beam_size=3, ctc_weight=0.4) on a reduced conmamba_large_s2s against tests/s2s_beam_ref.beam_search on an fp64
    copy of the decoder and heads on the host
  * TransformerASR.forward against the reference's (golden g_tdec_forward)
"""
import copy
import importlib.util
import math
import os
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ctc_prefix_ref as C  # noqa: E402
import s2s_beam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}

_spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(HERE, "golden", "synth.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


def close(a, b, rtol=2e-3, atol=2e-4):
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol * scale)


def _host64(module):
    """An fp64 copy on the host whose stepped route, if it has one, is the torch one."""
    from mamba_asr_amd import ops
    m = copy.deepcopy(module).cpu().double().eval()
    for sub in m.modules():
        if hasattr(sub, "xattn_fn"):
            sub.xattn_fn, sub.attn_fn = ops.xattn_step_torch, ops.attn_step_torch
    return m


# ------------------------------------------------------------------------------------------------------------ stepped decoder
V_STEP, T_MEM, ENC_LENS = 50, 70, [70, 41]
WIDEN = [0, 0, 0, 1, 1, 1]
ROWS = [[0, 0, 1, 3, 4, 5], [0, 1, 2, 3, 4, 5], [2, 1, 0, 5, 5, 3], [1, 1, 1, 4, 3, 3], [0, 2, 1, 4, 5, 3], [2, 2, 0, 3, 3, 5],
        [0, 1, 2, 3, 4, 5], [1, 0, 2, 5, 4, 3], [0, 0, 0, 4, 4, 4], [2, 1, 0, 3, 5, 4], [1, 2, 2, 3, 3, 4], [0, 1, 2, 3, 4, 5]]
_STEP = {}


def _step_model(d_model):
    """-> (TransformerASR on the GPU in fp32, its fp64 host copy, memory (2, T_MEM, d_model) fp32 on the host)"""
    if d_model not in _STEP:
        from mamba_asr_amd.modules.TransformerASR import TransformerASR
        torch.manual_seed(d_model)
        m = TransformerASR(tgt_vocab=V_STEP, input_size=8, d_model=d_model, nhead=4, num_encoder_layers=1, num_decoder_layers=2,
                           d_ffn=256, dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="transformer",
                           attention_type="RelPosMHAXL", normalize_before=True, causal=False, mamba_config=dict(CFG))
        with torch.no_grad():
            for p in m.decoder.parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn_like(p))
        m.decoder.initial_capacity = 4
        m = m.eval()
        _STEP[d_model] = (copy.deepcopy(m).to(DEV), _host64(m), torch.randn(2, T_MEM, d_model))
    return _STEP[d_model]


def _stepped(m, memory, xattn_fn, attn_fn, autocast):
    """12 steps of 6 rows (2 utterances x 3) with the scripted reorders -> per step the outputs (6, d_model) fp64 on the host, each
    row's prefix and utterance"""
    dec = m.decoder
    keep = dec.xattn_fn, dec.attn_fn
    dec.xattn_fn, dec.attn_fn = xattn_fn, attn_fn
    gen = torch.Generator().manual_seed(11)
    poisoned = memory.clone()
    poisoned[1, ENC_LENS[1]:] = float("nan")
    out, prefixes, utt, hist = [], [[] for _ in WIDEN], list(WIDEN), []
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        state = m.init_decode_state(poisoned.to(DEV), torch.tensor(ENC_LENS)).reorder(torch.tensor(WIDEN, device=DEV))
        for rows in ROWS:
            tokens = torch.randint(1, V_STEP, (6,), generator=gen)
            out.append(m.decode_step(tokens.to(DEV), state)[:, 0].double().cpu())
            prefixes = [p + [int(c)] for p, c in zip(prefixes, tokens)]
            hist.append(([list(p) for p in prefixes], list(utt)))
            state = state.reorder(torch.tensor(rows, device=DEV))
            prefixes, utt = [list(prefixes[i]) for i in rows], [utt[i] for i in rows]
    dec.xattn_fn, dec.attn_fn = keep
    assert state.cache.capacity == 16 and state.ck[0].dtype == (torch.bfloat16 if autocast else torch.float32)
    assert state.ck[0].shape == (2, T_MEM, memory.shape[2])          # per utterance: never widened to the 6 rows
    return out, hist


@pytest.mark.parametrize("mode", ["fp32", "autocast_bf16"])
@pytest.mark.parametrize("d_model", [128, 144])
def test_stepped_decoder_matches_the_fp64_full_decode(d_model, mode):
    """Tolerance: 4 x the distance of the torch routes' outputs (ops.xattn_step_torch / ops.attn_step_torch in the same steps)
    from fp64, and not less than one fp32 ulp at max|reference|."""
    from mamba_asr_amd import ops
    m, m64, memory = _step_model(d_model)
    assert m.decoder.xattn_fn is ops.xattn_step                      # the default route is the native kernel
    assert m.decoder.attn_fn is (ops.attn_step if d_model == 128 else ops.attn_step_torch)   # dh 36: cm_attn_step has 32 / 64
    native, hist = _stepped(m, memory, m.decoder.xattn_fn, m.decoder.attn_fn, mode != "fp32")
    base, hist2 = _stepped(m, memory, ops.xattn_step_torch, ops.attn_step_torch, mode != "fp32")
    assert hist == hist2
    key = ("ref", d_model)
    if key not in _STEP:
        mem64, lens = memory.double(), torch.tensor(ENC_LENS)
        with torch.no_grad():
            _STEP[key] = [torch.stack([m64.decode(torch.tensor([p]), mem64[u:u + 1], lens[u:u + 1])[0][0, -1]
                                       for p, u in zip(*step)]) for step in hist]
    ref = _STEP[key]
    top = max(float(r.abs().max()) for r in ref)
    d_torch = max(float((b - r).abs().max()) for b, r in zip(base, ref))
    d_native = max(float((n - r).abs().max()) for n, r in zip(native, ref))
    tol = max(4.0 * d_torch, 2.0 ** (math.floor(math.log2(top)) - 23))
    print(f"d_model {d_model} {mode}: |native - fp64| {d_native:.3e}, |torch routes - fp64| {d_torch:.3e}, tolerance {tol:.3e}, "
          f"max|reference| {top:.3f}")
    assert not any(bool(torch.isnan(n).any()) for n in native)
    assert d_native <= tol


# --------------------------------------------------------------------------------------------------------------- end to end
W_CTC, BEAM = 0.4, 3
# The first seed from 0 upward at which the fp64 reference's own choices are clear: at every step of every utterance its BEAM-th and
# (BEAM + 1)-th candidates, and the consecutive final scores of its best 3 hypotheses, lie at least 100 x the tolerance apart
# (asserted in the test, no step skipped).  Chosen on the host with the encoder restated by the oracle: seeds 1 and 2 miss it, seed 0
# holds it with less than 2 x to spare on the final scores, seed 3 with more than 3 x on both.
E2E_SEED = 3
_E2E = {}


def _reduced_large(seed):
    """conmamba_large_s2s cut to 2 + 2 layers, d_model 128 with 2 heads (the large recipe's head dimension 64), 60 tokens; three
    utterances of 30 / 21 / 12 encoder frames; <eos> biased up so that hypotheses close near their min_decode_ratio floor."""
    if seed not in _E2E:
        from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
        cfg = replace(CONFIGS["conmamba_large_s2s"], d_model=128, d_ffn=256, num_encoder_layers=2, num_decoder_layers=2, nhead=2,
                      output_neurons=60, seed=seed, min_decode_ratio=0.3, max_decode_ratio=0.25)
        assert cfg.decoder_module == "transformer"
        model = ConMambaASR(cfg).to(DEV).eval()
        with torch.no_grad():
            model.seq_lin.w.weight.mul_(4.0)                          # sharper token distributions: clearer choices
            model.seq_lin.w.bias[cfg.eos_index] += 10.0
            model.seq_lin.w.bias[cfg.bos_index] -= 10.0
        wavs, _ = synthetic_wavs(3, samples_for_frames(120), 5, DEV)
        lens = torch.tensor([1.0, 0.7, 0.4], device=DEV)
        for i, r in enumerate(lens.tolist()):
            wavs[i, int(round(r * wavs.shape[1])):] = 0.0
        with torch.no_grad():
            model.calibrate(wavs, lens)
        _E2E[seed] = (cfg, model, wavs, lens)
    return _E2E[seed]


def _reference(seed):
    """-> per utterance (ranked, gaps, steps) of R.beam_search in fp64 on an fp64 host copy of the decoder and the two heads (the
    encoder output is the GPU's, widened), the largest distance of the same increments restated in fp32 on the host, the case"""
    cfg, model, wavs, lens = _reduced_large(seed)
    assert (cfg.blank_index, cfg.bos_index, cfg.eos_index) == (0, 1, 2)
    with torch.no_grad():
        enc = model.encode(wavs, lens).float().cpu()
    tr64, seq64, ctc64 = _host64(model.Transformer), _host64(model.seq_lin), _host64(model.ctc_lin)
    tr32, seq32, ctc32 = copy.deepcopy(tr64).float(), copy.deepcopy(seq64).float(), copy.deepcopy(ctc64).float()
    T, V = enc.shape[1], cfg.output_neurons
    enc_lens = [round(T * r) for r in lens.tolist()]
    cap = int(cfg.max_decode_ratio * max(enc_lens))
    floors = [int(cfg.min_decode_ratio * e) for e in enc_lens]
    with torch.no_grad():
        lp64 = torch.log_softmax(ctc64(enc.double()), dim=-1)
        lp32 = torch.log_softmax(ctc32(enc), dim=-1)
    r64, r32 = C.RefCTCPrefixScorer(0, cfg.eos_index, np.float64), C.RefCTCPrefixScorer(0, cfg.eos_index, np.float32)
    err32, out = [0.0], []
    for b in range(len(enc_lens)):
        states = {(): (r64.init(lp64[b:b + 1], [enc_lens[b]]), r32.init(lp32[b:b + 1], [enc_lens[b]]))}
        n = torch.tensor([enc_lens[b]])

        def state(g):
            if g not in states:
                s64, s32 = state(g[:-1])
                states[g] = (r64.advance(s64, torch.tensor([g[-1]])), r32.advance(s32, torch.tensor([g[-1]])))
            return states[g]

        def logp(prefix):
            with torch.no_grad():
                a64 = torch.log_softmax(seq64(tr64.decode(torch.tensor([prefix]), enc[b:b + 1].double(), n)[0])[0, -1], dim=-1)
                a32 = torch.log_softmax(seq32(tr32.decode(torch.tensor([prefix]), enc[b:b + 1], n)[0])[0, -1], dim=-1)
            s64, s32 = state(tuple(prefix[1:]))
            d64, d32 = r64.score(s64)[0], r32.score(s32)[0]
            fin = torch.isfinite(d64)
            assert torch.equal(fin, torch.isfinite(d32))
            inc64 = a64 + W_CTC * d64
            inc32 = (a32 + np.float32(W_CTC) * d32.float()).double()
            err32[0] = max(err32[0], float((inc64[fin] - inc32[fin]).abs().max()))
            return inc64

        out.append(R.beam_search(logp, V, BEAM, cfg.bos_index, cfg.eos_index, floors[b], cap, True, BEAM, np.float64))
    return out, err32[0], (cfg, model, wavs, lens)


def _margins(ref):
    gap = min(g for ranked, gaps, _ in ref for g in gaps)
    final = min(float(a[1] - b[1]) for ranked, _, _ in ref for a, b in zip(ranked, ranked[1:]))
    return gap, final


def test_beam_three_joint_decoding_matches_the_fp64_host_reference():
    """Tolerance per increment: 4 x the distance from fp64 of the same increments restated in fp32 on the host (the decoder on the
    torch routes, the CTC term by tests/ctc_prefix_ref.py in fp32); a summed score gets that times the number of steps.  Required:
    the same BEAM token lists in the same order, and the scores within tolerance."""
    from mamba_asr_amd import ops
    ref, err32, (cfg, model, wavs, lens) = _reference(E2E_SEED)
    assert model.Transformer.decoder.xattn_fn is ops.xattn_step and model.Transformer.decoder.attn_fn is ops.attn_step
    hyps, lengths, scores, log_probs = model.transcribe_s2s(wavs, lens, ctc_weight=W_CTC, beam_size=BEAM, topk=BEAM)
    tol = 4.0 * err32
    gap, final = _margins(ref)
    steps = log_probs.shape[1]
    print(f"seed {E2E_SEED}: fp32 restatement error {err32:.3e}, tolerance {tol:.3e}, smallest candidate gap {gap:.3e}, "
          f"smallest final-score gap {final:.3e}, steps {steps}")
    assert err32 > 0 and all(len(ranked) == BEAM for ranked, _, _ in ref)
    assert gap >= 100.0 * tol and final >= 100.0 * tol, "the case must keep every reference choice clear of the tolerance"
    assert steps == max(s for _, _, s in ref)
    assert scores.shape == (3, BEAM) and lengths.shape == (3, BEAM) and any(len(h) for h in hyps[0])
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
    # every other option of transcribe_s2s runs on this decoder too: greedy, and beam 1 without normalisation is greedy bit for bit
    want = model.transcribe_s2s(wavs, lens, ctc_weight=W_CTC)
    got = model.transcribe_s2s(wavs, lens, ctc_weight=W_CTC, beam_size=1, length_normalization=False)
    assert got[0] == want[0] and torch.equal(got[2], want[2])


# --------------------------------------------------------------------------------------------------------------- against the reference
def test_forward_matches_the_reference(golden):
    """Golden g_tdec_forward = outputs of the REFERENCE's TransformerASR.forward with its Transformer decoder; the tolerances of
    tests/test_hip_parity_r3.py for g_s2s_forward."""
    from mamba_asr_amd.modules.TransformerASR import TransformerASR
    g = golden("g_tdec_forward")
    m = TransformerASR(tgt_vocab=53, input_size=640, d_model=128, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=256,
                       dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="transformer",
                       attention_type="RelPosMHAXL", normalize_before=True, causal=False, mamba_config=dict(CFG))
    sd = {k: v for k, v in S.synth_like(m, 1290).items() if not k.endswith(".pe")}
    miss = m.load_state_dict(sd, strict=False)
    assert not miss.unexpected_keys and all(k.endswith(".pe") for k in miss.missing_keys)
    m = m.to(DEV).eval()
    src = S.synth_input("g_tdec.src", (3, 41, 20, 32), 1290).to(DEV)
    tgt, wav_len = g["tgt"].long().to(DEV), g["wav_len"].to(DEV)
    for mode in ("fused-nograd", "module-grad"):
        with torch.set_grad_enabled(mode == "module-grad"):       # no_grad + eval: the fused inference kernels where supported
            enc, dec = m(src, tgt, wav_len)
        close(enc, g["encoder_out"])
        close(dec, g["decoder_out"])
    pred, attn = m.decode(tgt, enc.detach(), g["enc_len"].to(DEV))
    close(pred, g["decode_prediction"])
    close(attn, g["decode_attn"])
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        enc_bf, dec_bf = m(src, tgt, wav_len)
    print(f"bf16 autocast: max|encoder_out - golden| {float((enc_bf.float().cpu() - g['encoder_out']).abs().max()):.3e}, "
          f"max|decoder_out - golden| {float((dec_bf.float().cpu() - g['decoder_out']).abs().max()):.3e}")
    torch.testing.assert_close(enc_bf.float().cpu(), g["encoder_out"], rtol=3e-2, atol=5e-2)
    torch.testing.assert_close(dec_bf.float().cpu(), g["decoder_out"], rtol=3e-2, atol=6e-2)
