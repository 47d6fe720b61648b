"""The stateful Mamba decoder and the greedy S2S searcher on top of it.

  * init_decode_state + decode_step, token by token, against the REFERENCE's own TransformerASR.decode over the whole
    prefix (golden g_s2s_forward, `decode_prediction`), fp32 and bf16 autocast, fused and five-launch mixer step   [GPU]
  * DecoderState.reorder, bit for bit                                                                            [GPU]
  * transcribe_s2s end to end against the full-prefix decode of the sequences it produced                        [GPU]
  * the searcher's host logic on scripted log-probability tables                                                 [CPU]

Bounds: fp32 rtol 2e-3, atol 2e-4 x max(1, max|ref|) and bf16 rtol 3e-2, atol 6e-2: what tests/test_hip_parity_r3.py gives
`decode_prediction` and the bf16 decoder output.
"""
import importlib.util
import os

import pytest
import torch
import torch.nn as nn

DEV = "cuda"
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}

_spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(os.path.dirname(__file__), "golden", "synth.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)


def close(a, b, rtol=2e-3, atol=2e-4):
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol * scale)


_MODEL = {}


def _s2s_model():
    """The construction of tests/test_hip_parity_r3.py `_s2s_model` (D 128, E 256, dt_rank 8, 2 + 2 layers), in eval mode."""
    if "m" not in _MODEL:
        from mamba_asr_amd.modules.TransformerASR import TransformerASR
        m = TransformerASR(tgt_vocab=53, input_size=640, d_model=128, nhead=4, num_encoder_layers=2, num_decoder_layers=2, d_ffn=256,
                           dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="mamba",
                           attention_type="RelPosMHAXL", normalize_before=True, causal=False, mamba_config=dict(CFG))
        sd = {k: v for k, v in S.synth_like(m, 1280).items() if not k.endswith(".pe")}
        miss = m.load_state_dict(sd, strict=False)
        assert not miss.unexpected_keys and all(k.endswith(".pe") for k in miss.missing_keys)
        _MODEL["m"] = m.to(DEV).eval()
    return _MODEL["m"]


def _fused(monkeypatch, on):
    """CM_FUSED_STEP is read once, at import: the switch it sets is flipped here."""
    from mamba_asr_amd.modules.mamba import bimamba
    monkeypatch.setattr(bimamba, "FUSED_STEP", bool(on))


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [1, 0], ids=["CM_FUSED_STEP=1", "CM_FUSED_STEP=0"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stepping_vs_reference_decode(golden, monkeypatch, precision, fused):
    """batch 3, memory T = 41, an 11-token tgt with padding: decode_step on tgt[:, i], i = 0..10, from
    init_decode_state(encoder_out) stacks up to the reference's decode(tgt, encoder_out)."""
    _fused(monkeypatch, fused)
    g = golden("g_s2s_forward")
    m = _s2s_model()
    enc, tgt = g["encoder_out"].to(DEV), g["tgt"].long().to(DEV)
    assert enc.shape == (3, 41, 128) and tgt.shape == (3, 11)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=precision == "bf16"):
        state = m.init_decode_state(enc)
        outs = [m.decode_step(tgt[:, i], state) for i in range(tgt.shape[1])]
    assert state.position == 11 and all(o.shape == (3, 1, 128) for o in outs)
    pred = torch.cat(outs, dim=1).float()
    ref = g["decode_prediction"]
    print(f"{precision} fused={fused}: max|stepped - reference decode| {(pred.cpu() - ref).abs().max().item():.3e} (max|ref| {ref.abs().max().item():.3e})")
    if precision == "fp32":
        close(pred, ref)
    else:
        torch.testing.assert_close(pred.cpu(), ref, rtol=3e-2, atol=6e-2)


@pytest.mark.gpu
def test_reorder_is_bit_exact(golden):
    """3 steps on batch 2, reorder([1, 1, 0]), one more step == the rows of stepping the batch [1, 1, 0] from the start."""
    g = golden("g_s2s_forward")
    m = _s2s_model()
    enc, tgt = g["encoder_out"].to(DEV), g["tgt"].long().to(DEV)
    idx = [1, 1, 0]
    with torch.no_grad():
        state = m.init_decode_state(enc[:2])
        for i in range(3):
            m.decode_step(tgt[:2, i], state)
        moved = state.reorder(idx)
        assert moved is not state and moved.position == 3 and moved.batch == 3 and state.batch == 2
        got = m.decode_step(tgt[idx, 3], moved)
        want_state = m.init_decode_state(enc[idx])
        for i in range(4):
            want = m.decode_step(tgt[idx, i], want_state)
    assert moved.position == 4 and state.position == 3
    assert torch.equal(got, want)
    for a, b in zip(moved.tensors(), want_state.tensors()):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_transcribe_s2s_matches_full_prefix_decode():
    """D 128, 3 synthetic utterances of different lengths.  No token-for-token comparison with an independent argmax loop
    (near-ties may flip): the sequences the searcher produced are fed, <bos> first, through the full-prefix
    TransformerASR.decode + seq_lin + log-softmax, and the searcher's per-token log-probabilities must match those, each
    chosen token within 1e-3 of the full-prefix maximum over the tokens allowed at its position.

    The random-init model is made to stop: seq_lin's <eos> bias is raised by 10 (logits are O(1)), so every row emits
    <eos> at its min_decode_ratio floor (enc_len 30 / 21 / 12 -> steps 9 / 6 / 3), <bos> is biased out, and
    max_decode_ratio caps the loop at 7 steps: two rows finish early at different steps and keep stepping with frozen
    scores, one row is cut by the cap."""
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = ASRConfig("s2s_tiny", d_model=128, d_ffn=256, num_encoder_layers=2, num_decoder_layers=2, output_neurons=50, n_fft=400,
                    seed=21, min_decode_ratio=0.3, max_decode_ratio=0.25)
    assert (cfg.bos_index, cfg.eos_index) == (1, 2)
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
        hyps, lengths, scores, log_probs = model.transcribe_s2s(wavs, lens)
        enc = model.encode(wavs, lens)
    T = enc.shape[1]
    enc_lens = [round(T * r) for r in lens.tolist()]
    cap = int(cfg.max_decode_ratio * max(enc_lens))
    floors = [int(cfg.min_decode_ratio * e) for e in enc_lens]
    print(f"enc T {T}, enc_lens {enc_lens}, floors {floors}, cap {cap}, lengths {lengths.tolist()}, hyps {hyps}")
    steps = log_probs.shape[1]
    assert len(hyps) == 3 and lengths.shape == (3,) and scores.shape == (3,) and log_probs.shape[0] == 3 and steps <= cap
    assert lengths.tolist() == [len(h) for h in hyps] and max(lengths.tolist()) <= cap
    assert all(t not in (cfg.bos_index, cfg.eos_index) for h in hyps for t in h)
    finished_early = 0
    for b, h in enumerate(hyps):
        n = len(h)
        done = n < steps                                                       # the row emitted <eos> at step n
        seq = torch.tensor([[cfg.bos_index] + h], device=DEV)
        with torch.no_grad():
            pred, _ = model.Transformer.decode(seq, enc[b:b + 1])
            full = torch.log_softmax(model.seq_lin(pred)[0].float(), dim=-1)    # (n + 1, vocab): position i predicts token i
        upto = n + 1 if done else n
        chosen = h + [cfg.eos_index] if done else h
        want = torch.stack([full[i, chosen[i]] for i in range(upto)])
        print(f"row {b}: {n} tokens, done {done}, max|lp - full-prefix lp| {(log_probs[b, :upto] - want).abs().max().item():.3e}")
        close(log_probs[b, :upto], want)
        for i in range(upto):
            allowed = full[i].clone()
            if i < floors[b]:
                allowed[cfg.eos_index] = float("-inf")                          # masked below the min_decode_ratio floor
            assert float(want[i]) >= float(allowed.max()) - 1e-3, (b, i)
        if done:
            assert n >= floors[b]
            finished_early += n + 1 < steps
            # frozen: nothing is added behind the <eos>, and the score is the sum up to and including it
            assert bool((log_probs[b, upto:] == 0).all())
        torch.testing.assert_close(scores[b], log_probs[b, :upto].sum(), rtol=1e-5, atol=1e-5)
    assert finished_early >= 1, "the case is built so that a row finishes before the loop ends"


# ----------------------------------------------------------------------------------------------------------
# host logic, no GPU: a scripted per-token function
# ----------------------------------------------------------------------------------------------------------
BOS, EOS, V = 1, 2, 6


def _table(rows):
    """rows[t][b] = the token that wins at step t for row b, as a (steps, batch, V) log-probability table: the winner gets
    log 0.5, <eos> log 0.2 (the runner-up unless it is the winner), the rest share what is left."""
    steps, batch = len(rows), len(rows[0])
    p = torch.full((steps, batch, V), 0.3 / (V - 2))
    for t in range(steps):
        for b in range(batch):
            p[t, b, EOS] = 0.2
            if rows[t][b] == EOS:
                p[t, b] = 0.5 / (V - 1)
            p[t, b, rows[t][b]] = 0.5
    return torch.log(p)


def _searcher(table, seen=None, **kw):
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher

    def init_fn(enc):
        return {"t": 0}

    def step_fn(tokens, state):
        if seen is not None:
            seen.append(tokens.tolist())
        lp = table[state["t"]]
        state["t"] += 1
        return lp, state

    return S2SGreedySearcher(bos_index=BOS, eos_index=EOS, step_fn=step_fn, init_fn=init_fn, **kw)


def test_searcher_stops_rows_at_their_first_eos_and_freezes_scores():
    rows = [[3, 4, 5], [EOS, 4, 3], [3, 5, 4], [4, EOS, 4], [5, 3, EOS], [3, 3, 3]]
    seen = []
    s = _searcher(_table(rows), seen, min_decode_ratio=0.0, max_decode_ratio=1.0)
    hyps, lengths, scores, log_probs = s(torch.zeros(3, 10, 4), torch.ones(3))
    assert hyps == [[3], [4, 4, 5], [5, 3, 4, 4]]
    assert lengths.tolist() == [1, 3, 4] and lengths.dtype == torch.long
    assert log_probs.shape == (3, 5) and scores.shape == (3,)                   # the loop ended when the last row finished
    import math
    lp = math.log(0.5)
    torch.testing.assert_close(scores, torch.tensor([2 * lp, 4 * lp, 5 * lp]))
    assert bool((log_probs[0, 2:] == 0).all()) and bool((log_probs[1, 4:] == 0).all())
    torch.testing.assert_close(log_probs.sum(1), scores)
    # the first call gets <bos>; finished rows are fed <eos>, the batch keeps its shape
    assert seen[0] == [BOS] * 3 and seen[2] == [EOS, 4, 3] and seen[4] == [EOS, EOS, 4] and len(seen) == 5


def test_searcher_min_decode_ratio_floor_is_per_row():
    """enc_len 10 and 5 at ratio 0.3 -> <eos> may be chosen from step 3 / step 1 on; before, the runner-up is taken."""
    rows = [[EOS, EOS]] * 6
    s = _searcher(_table(rows), min_decode_ratio=0.3, max_decode_ratio=1.0)
    hyps, lengths, scores, log_probs = s(torch.zeros(2, 10, 4), torch.tensor([1.0, 0.5]))
    assert lengths.tolist() == [3, 1] and all(t not in (BOS, EOS) for h in hyps for t in h)
    assert log_probs.shape == (2, 4)
    import math
    other, eos = math.log(0.5 / (V - 1)), math.log(0.5)
    torch.testing.assert_close(scores, torch.tensor([3 * other + eos, other + eos]))


def test_searcher_max_decode_ratio_cap():
    rows = [[3, 4]] * 20
    s = _searcher(_table(rows), min_decode_ratio=0.0, max_decode_ratio=0.5)
    hyps, lengths, scores, log_probs = s(torch.zeros(2, 12, 4), torch.tensor([0.5, 1.0]))     # cap = 0.5 * max enc_len = 6
    assert hyps == [[3] * 6, [4] * 6] and lengths.tolist() == [6, 6] and log_probs.shape == (2, 6)


def test_searcher_all_eos_at_step_zero_gives_empty_hypotheses():
    rows = [[EOS, EOS, EOS]] * 4
    s = _searcher(_table(rows))
    hyps, lengths, scores, log_probs = s(torch.zeros(3, 8, 4), torch.ones(3))
    assert hyps == [[], [], []] and lengths.tolist() == [0, 0, 0] and log_probs.shape == (3, 1) and scores.shape == (3,)
    import math
    torch.testing.assert_close(scores, torch.full((3,), math.log(0.5)))
    # a cap of zero steps: the 4-tuple keeps its shapes
    s = _searcher(_table(rows), max_decode_ratio=0.0)
    hyps, lengths, scores, log_probs = s(torch.zeros(3, 8, 4), torch.ones(3))
    assert hyps == [[], [], []] and log_probs.shape == (3, 0) and scores.tolist() == [0.0, 0.0, 0.0]


def test_searcher_needs_modules_or_callables():
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher
    with pytest.raises(ValueError):
        S2SGreedySearcher(modules=None)
