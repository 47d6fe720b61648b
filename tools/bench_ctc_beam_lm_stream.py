"""The streamed LM-fused CTC beam search next to the three searches it is made of, on the inputs of
tests/test_ctc_beam_search_gpu.py::test_benchmark_shape (64 x 1000 x 31: even utterances competing, odd peaky) at the recipe's
settings with the generated order-3 model of tools/bench_ctc_beam_lm.py, in 16-frame steps (62 of 16 frames, then one of 8).
Device events after a warm-up utterance; in each of five rounds the four kernels run one after the other:
    the 1000 frames chunked through cm_ctc_beam_lm_stream   against   one cm_ctc_beam_lm_search launch      (R_lm)
    the 1000 frames chunked through cm_ctc_beam_stream      against   one cm_ctc_beam_search launch         (R_free)
Reported: the medians over the rounds, ms per 64 x 16 step of both streamed searches, R_lm and R_free as ratios of the medians,
each ratio's spread over the rounds (max - min of the per-round ratios) and the bar of DESIGN.md §4q,
    R_lm - 1 <= 1.5 x (R_free - 1) + the larger spread.
Prints one text line per round and a final JSON line."""
import json
import os
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_data as D  # noqa: E402
import ctc_lm_data as LD  # noqa: E402
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.ctc_decode import (HASH_BASE, HASH_SEP, StreamingCTCBeamLMSearcher,  # noqa: E402
                                      StreamingCTCBeamSearcher)

B, FRAMES, V, CHUNK, ROUNDS = 64, 1000, 31, 16, 5
FULL = FRAMES // CHUNK                 # 62 steps of 16 frames; the utterance's last step holds the other 8


def event():
    return torch.cuda.Event(enable_timing=True)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        path, _ = LD.make_arpa(os.path.join(d, "m.arpa"), seed=4, n_words=(18, 300, 300), n_bigrams=400, n_trigrams=300)
        fused = StreamingCTCBeamLMSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path, max_frames=FRAMES)
    free = StreamingCTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, max_frames=FRAMES)
    lm = fused.lm
    lp = torch.stack([(D.competing if b % 2 == 0 else D.peaky)(FRAMES, V, 900 + b) for b in range(B)]).to(dev)
    chunks = [lp[:, t0:t0 + CHUNK] for t0 in range(0, FULL * CHUNK, CHUNK)]
    tail = lp[:, FULL * CHUNK:]
    n = torch.full((B,), FRAMES, dtype=torch.int32, device=dev)
    tc, th, tp = fused._tables(dev)
    tl, tables = fused._tok_len(dev), lm.tables(dev)
    common = dict(blank=0, beam_size=100, topk=1, beam_prune_logp=-12.0, token_prune_min_logp=-1.2)
    states = {"lm": fused.make_state(B, dev), "free": free.make_state(B, dev)}

    def chunked(s, state):
        """-> (ms of the 62 full steps, ms of the whole utterance)"""
        state.reset()
        e0, e1, e2 = event(), event(), event()
        e0.record()
        for c in chunks:
            s.step(c, state)
        e1.record()
        s.step(tail, state)
        e2.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), e0.elapsed_time(e2)

    def whole(fn):
        e0, e1 = event(), event()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def whole_lm():
        return ops.ctc_beam_search_lm(lp, n, tc, th, tp, tl, HASH_BASE, HASH_SEP, tables, order=lm.order, n_words=len(lm.words),
                                      lm_bos=lm.bos, lm_eos=lm.eos, lm_unk=lm.unk, alpha=fused.alpha, beta=fused.beta,
                                      unk_score_offset=fused.unk_score_offset, **common)

    def whole_free():
        return ops.ctc_beam_search(lp, n, tc, th, tp, HASH_BASE, HASH_SEP, **common)

    # warm-up: code objects, cached device constants, one utterance through each kernel
    chunked(fused, states["lm"]), whole(whole_lm), chunked(free, states["free"]), whole(whole_free)
    print(f"{ROUNDS} rounds; {B} x {FRAMES} x {V}, recipe thresholds, beam 100, topk 1, order-{lm.order} model of {lm.n_entries} n-grams; "
          f"{FULL} steps of {CHUNK} frames + one of {FRAMES - FULL * CHUNK}", flush=True)
    rows = []
    for r in range(ROUNDS):
        steps_lm, utt_lm = chunked(fused, states["lm"])
        one_lm, out_lm = whole(whole_lm)
        steps_free, utt_free = chunked(free, states["free"])
        one_free, out_free = whole(whole_free)
        rows.append(dict(lm_step_ms=steps_lm / FULL, lm_chunked_ms=utt_lm, lm_whole_ms=one_lm, free_step_ms=steps_free / FULL,
                         free_chunked_ms=utt_free, free_whole_ms=one_free, r_lm=utt_lm / one_lm, r_free=utt_free / one_free))
        x = rows[-1]
        print(f"round {r}: LM stream {x['lm_chunked_ms']:.2f} ms ({x['lm_step_ms']:.3f} per step), one LM launch {x['lm_whole_ms']:.2f} ms, "
              f"R_lm {x['r_lm']:.4f}; LM-free stream {x['free_chunked_ms']:.2f} ms ({x['free_step_ms']:.3f} per step), one LM-free launch "
              f"{x['free_whole_ms']:.2f} ms, R_free {x['r_free']:.4f}", flush=True)

    # what was timed is the search: the streamed hypotheses are the whole-utterance ones, bit for bit
    tokens, tlen, scores, lms, nh, _ = [t.cpu() for t in out_lm]
    hyps = fused.hypotheses(states["lm"])
    same_lm = all(len(hyps[b]) == int(nh[b]) and all(h.score == float(scores[b, i]) and h.lm_score == float(lms[b, i]) and
                                                     h.text == fused.compose(tokens[b, i, :tlen[b, i]].tolist())
                                                     for i, h in enumerate(hyps[b])) for b in range(B))
    tokens, tlen, scores, nh, _ = [t.cpu() for t in out_free]
    hyps = free.hypotheses(states["free"])
    same_free = all(len(hyps[b]) == int(nh[b]) and all(h.score == float(scores[b, i]) and
                                                       h.text == free.compose(tokens[b, i, :tlen[b, i]].tolist())
                                                       for i, h in enumerate(hyps[b])) for b in range(B))

    med = {k: statistics.median(x[k] for x in rows) for k in rows[0] if not k.startswith("r_")}
    r_lm, r_free = med["lm_chunked_ms"] / med["lm_whole_ms"], med["free_chunked_ms"] / med["free_whole_ms"]
    spread_lm = max(x["r_lm"] for x in rows) - min(x["r_lm"] for x in rows)
    spread_free = max(x["r_free"] for x in rows) - min(x["r_free"] for x in rows)
    bar = 1.5 * (r_free - 1.0) + max(spread_lm, spread_free)
    out = {"batch": B, "frames": FRAMES, "vocab": V, "chunk": CHUNK, "rounds": ROUNDS, "state_bytes_lm": states["lm"].slab.shape[1],
           "state_bytes_free": states["free"].slab.shape[1], **{k: round(v, 4) for k, v in med.items()},
           "step_ratio_lm_over_free": round(med["lm_step_ms"] / med["free_step_ms"], 4),
           "whole_ratio_lm_over_free": round(med["lm_whole_ms"] / med["free_whole_ms"], 4),
           "R_lm": round(r_lm, 4), "R_free": round(r_free, 4), "R_lm_spread": round(spread_lm, 4), "R_free_spread": round(spread_free, 4),
           "bar_R_lm_minus_1": round(bar, 4), "R_lm_minus_1": round(r_lm - 1.0, 4), "within_bar": bool(r_lm - 1.0 <= bar),
           "lm_chunked_equals_whole": bool(same_lm), "free_chunked_equals_whole": bool(same_free), "rounds_detail": rows}
    print(f"medians: 64 x 16 step {med['lm_step_ms']:.3f} ms with the LM, {med['free_step_ms']:.3f} ms LM-free; R_lm {r_lm:.4f} (spread "
          f"{spread_lm:.4f}), R_free {r_free:.4f} (spread {spread_free:.4f}); R_lm - 1 = {r_lm - 1:.4f} against the bar {bar:.4f}: "
          f"{'within' if out['within_bar'] else 'MISSED'}; chunked == whole: LM {same_lm}, LM-free {same_free}", flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
