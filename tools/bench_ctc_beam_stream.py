"""The streamed CTC beam search at the recipe's settings (beam 100, beam_prune_logp -12, token_prune_min_logp -1.2): ms per
StreamingCTCBeamSearcher.step call of 16 frames, and a 1000-frame utterance fed in 16-frame chunks against the one launch of
cm_ctc_beam_search on the same log-probs.  Device events after a warm-up utterance, median of 5 windows of UTTS utterances each
(62 steps of 16 frames, then one of 8); the same 62 steps replayed from one hipGraph give the device time without the host's
enqueue cost.  Prints one text line per case and a final JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_data as D  # noqa: E402
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP, StreamingCTCBeamSearcher  # noqa: E402

FRAMES, CHUNK, WINDOWS, UTTS = 1000, 16, 5, 4
FULL = FRAMES // CHUNK                 # 62 steps of 16 frames; the utterance's last step holds the other 8


def vocabulary(v):
    """The tests' 31 SentencePiece characters, or a synthetic SentencePiece vocabulary of v pieces (every third a word start)."""
    if v == len(D.SPM_VOCAB):
        return D.SPM_VOCAB
    return D.SPM_VOCAB[:4] + [("▁" if i % 3 == 0 else "") + f"p{i}" for i in range(v - 4)]


def elapsed(pairs):
    return sum(a.elapsed_time(b) for a, b in pairs)


def event():
    return torch.cuda.Event(enable_timing=True)


def case(dev, streams, v, name, gen):
    s = StreamingCTCBeamSearcher(**D.RECIPE, vocab_list=vocabulary(v), max_frames=FRAMES)
    uniq = min(streams, 4)
    lp = torch.stack([gen(FRAMES, v, 500 + b) for b in range(uniq)]).to(dev)[torch.arange(streams) % uniq].contiguous()
    chunks = [lp[:, t0:t0 + CHUNK] for t0 in range(0, FULL * CHUNK, CHUNK)]
    tail = lp[:, FULL * CHUNK:]
    state = s.make_state(streams, dev)

    def utterance(timed):
        state.reset()
        e0, e1, e2 = event(), event(), event()
        e0.record()
        for c in chunks:
            s.step(c, state)
        e1.record()
        s.step(tail, state)
        e2.record()
        timed.append((e0, e1, e2))

    utterance([])                                                  # warm-up: code objects, cached device constants
    torch.cuda.synchronize()
    steps_ms, utt_ms = [], []
    for _ in range(WINDOWS):
        timed = []
        for _ in range(UTTS):
            utterance(timed)
        torch.cuda.synchronize()
        steps_ms.append(elapsed((a, b) for a, b, _ in timed) / (UTTS * FULL))
        utt_ms.append(elapsed((a, c) for a, _, c in timed) / UTTS)

    # the one launch of the whole-utterance kernel on the same log-probs
    tc, th, tp = s._tables(dev)
    n = torch.full((streams,), FRAMES, dtype=torch.int32, device=dev)

    def whole():
        return ops.ctc_beam_search(lp, n, tc, th, tp, HASH_BASE, HASH_SEP, blank=0, beam_size=s.beam_size, topk=s.topk,
                                   prune_history=s.prune_history, beam_prune_logp=s.beam_prune_logp,
                                   token_prune_min_logp=s.token_prune_min_logp)
    whole()
    torch.cuda.synchronize()
    whole_ms = []
    for _ in range(WINDOWS):
        e0, e1 = event(), event()
        e0.record()
        for _ in range(UTTS):
            out = whole()
        e1.record()
        torch.cuda.synchronize()
        whole_ms.append(e0.elapsed_time(e1) / UTTS)
    tokens, tlen, scores, nh, _ = [x.cpu() for x in out]
    hyps = s.hypotheses(state)
    same = all(len(hyps[b]) == int(nh[b]) and all(h.score == float(scores[b, i]) and
                                                  h.text == s.compose(tokens[b, i, :tlen[b, i]].tolist()) for i, h in enumerate(hyps[b]))
               for b in range(streams))

    # the 62 full steps as one hipGraph: the device's time per step without the host's enqueue cost
    gstate = s.make_state(streams, dev)
    gstate.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for c in chunks:
            s.step(c, gstate)
    graph_ms = []
    for _ in range(WINDOWS):
        timed = []
        for _ in range(UTTS):
            gstate.reset()
            e0, e1 = event(), event()
            e0.record()
            graph.replay()
            e1.record()
            timed.append((e0, e1))
        torch.cuda.synchronize()
        graph_ms.append(elapsed(timed) / (UTTS * FULL))
    s.step(tail, gstate, reset=None)
    torch.cuda.synchronize()
    replay_same = torch.equal(gstate.slab, state.slab)

    med = statistics.median
    r = {"streams": streams, "vocab": v, "data": name, "step_ms": med(steps_ms), "step_ms_min": min(steps_ms), "step_ms_max": max(steps_ms),
         "graph_step_ms": med(graph_ms), "graph_step_ms_min": min(graph_ms), "graph_step_ms_max": max(graph_ms),
         "chunked_utt_ms": med(utt_ms), "chunked_utt_ms_min": min(utt_ms), "chunked_utt_ms_max": max(utt_ms),
         "whole_utt_ms": med(whole_ms), "whole_utt_ms_min": min(whole_ms), "whole_utt_ms_max": max(whole_ms),
         "chunked_equals_whole": bool(same), "replay_equals_eager": bool(replay_same)}
    print(f"streams {streams:3d} x {CHUNK} frames, V {v:4d}, {name:9s}: step {r['step_ms']:.3f} ms eager (min {r['step_ms_min']:.3f}, max "
          f"{r['step_ms_max']:.3f}), {r['graph_step_ms']:.3f} ms in a hipGraph of {FULL} steps (min {r['graph_step_ms_min']:.3f}, max "
          f"{r['graph_step_ms_max']:.3f}); {FRAMES} frames chunked {r['chunked_utt_ms']:.2f} ms (min {r['chunked_utt_ms_min']:.2f}, max "
          f"{r['chunked_utt_ms_max']:.2f}), one launch {r['whole_utt_ms']:.2f} ms (min {r['whole_utt_ms_min']:.2f}, max "
          f"{r['whole_utt_ms_max']:.2f}); chunked == whole: {same}; replay == eager: {replay_same}", flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=[64, 1])
    ap.add_argument("--vocab", type=int, nargs="+", default=[31, 4096], help="5000 pieces are clipped to the kernel's 4096")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    print(f"{WINDOWS} windows of {UTTS} utterances of {FRAMES} frames in {FULL} steps of {CHUNK} frames + one of {FRAMES - FULL * CHUNK}; "
          "recipe thresholds, beam 100, topk 1", flush=True)
    out = []
    for v in args.vocab:
        for streams in args.streams:
            for name, gen in (("peaky", D.peaky), ("competing", D.competing)):
                out.append(case(dev, streams, min(v, 4096), name, gen))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
