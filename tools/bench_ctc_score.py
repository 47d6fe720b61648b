"""Scoring beside what it replaces, on the GPU; every figure is the median of `--repeats` (at least 5) timed runs
after warm-up, and one JSON line is printed per part.

greedy   64 x 1000 x 5000 bf16 log-probabilities -> token lists.  CTCGreedyDecoder.tokens (cm_ctc_greedy + one read-back) against
         dataio.ctc_greedy_decode (torch.argmax, .cpu(), a Python loop over every frame): host clock around the whole call, which
         ends with the lists on the host.  Beside it the two kernels of cm_ctc_greedy alone (device events) and the bytes the
         arg-max phase has to read over that time -- a lower bound of the phase's read rate, the compaction kernel being inside.
edit     64 x 66 pairs of about 550 characters (an N-best list per utterance through ref_index) -> counts.  ops.edit_distance
         (device events around the launch) against metrics.edit_ops_host, which is timed on `--host-pairs` of the pairs and scaled
         to all of them (pure Python: minutes for the whole set)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mamba_asr_amd import dataio, metrics, ops  # noqa: E402
from mamba_asr_amd.ctc_decode import CTCGreedyDecoder  # noqa: E402


def _host_ms(run, repeats, warmup=2):
    for _ in range(warmup):
        run()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def _device_ms(run, repeats, warmup=3):
    for _ in range(warmup):
        run()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def greedy(dev, repeats, B=64, T=1000, V=5000):
    g = torch.Generator().manual_seed(1)
    lp = torch.cat([torch.log_softmax(torch.randn(8, T, V, generator=g) * 2.0, dim=-1).to(torch.bfloat16) for _ in range(B // 8)]).to(dev)
    wav_lens = torch.linspace(0.6, 1.0, B).to(dev)
    dec = CTCGreedyDecoder(0)
    # the comparison on the host: torch's device argmax leaves ties open, and bf16 has them
    native, old = dec.tokens(lp, wav_lens), dataio.ctc_greedy_decode(lp.float().cpu(), wav_lens.cpu(), 0)
    counts = torch.tensor([int(round(r * T)) for r in wav_lens.tolist()], dtype=torch.int32, device=dev)
    frames = int(counts.sum())
    n_ms = _host_ms(lambda: dec.tokens(lp, wav_lens), repeats)
    d_ms = _host_ms(lambda: dataio.ctc_greedy_decode(lp, wav_lens, 0), repeats)
    k_ms = _device_ms(lambda: ops.ctc_greedy(lp, counts), repeats)
    nbytes = frames * V * 2
    print(json.dumps({"part": "greedy", "batch": B, "frames": T, "vocab": V, "dtype": "bf16", "repeats": repeats, "decoded_frames": frames,
                      "same_tokens_as_dataio": native == old, "native_tokens_ms": round(n_ms[0], 3), "native_tokens_ms_min_max": [round(x, 3) for x in n_ms[1:]],
                      "dataio_ms": round(d_ms[0], 3), "dataio_ms_min_max": [round(x, 3) for x in d_ms[1:]],
                      "speedup": round(d_ms[0] / n_ms[0], 2), "cm_ctc_greedy_kernels_ms": round(k_ms[0], 4),
                      "cm_ctc_greedy_kernels_ms_min_max": [round(x, 4) for x in k_ms[1:]], "argmax_bytes": nbytes,
                      "argmax_read_rate_lower_bound_GBps": round(nbytes / (k_ms[0] * 1e-3) / 1e9, 1)}), flush=True)


def edit(dev, repeats, host_pairs, U=64, NB=66, L=550, alphabet=30):
    rng = random.Random(2)
    refs, hyps, ri = [], [], []
    for u in range(U):
        ref = [rng.randrange(alphabet) for _ in range(rng.randint(L - 50, L + 50))]
        refs.append(ref)
        for _ in range(NB):
            hyp = []
            for tok in ref:
                r = rng.random()
                if r < 0.04:
                    continue
                hyp.append(rng.randrange(alphabet) if r < 0.08 else tok)
                if r > 0.96:
                    hyp.append(rng.randrange(alphabet))
            hyps.append(hyp)
            ri.append(u)
    pad = lambda rows: torch.tensor([r + [0] * (max(map(len, rows)) - len(r)) for r in rows], dtype=torch.int32).to(dev)
    rt, ht = pad(refs), pad(hyps)
    rl, hl = torch.tensor([len(r) for r in refs], dtype=torch.int32).to(dev), torch.tensor([len(h) for h in hyps], dtype=torch.int32).to(dev)
    rit = torch.tensor(ri, dtype=torch.int32).to(dev)
    counts = ops.edit_distance(rt, rl, ht, hl, rit)[0].cpu().tolist()
    picks = list(range(0, len(hyps), len(hyps) // host_pairs))[:host_pairs]
    same = all(metrics.edit_ops_host(refs[ri[p]], hyps[p])[0] == counts[p] for p in picks)
    k_ms = _device_ms(lambda: ops.edit_distance(rt, rl, ht, hl, rit), repeats)
    k_ops_ms = _device_ms(lambda: ops.edit_distance(rt, rl, ht, hl, rit, want_ops=True), repeats)
    h = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for p in picks:
            metrics.edit_ops_host(refs[ri[p]], hyps[p])
        h.append((time.perf_counter() - t0) * 1e3 / len(picks))
    h_ms = statistics.median(h)
    print(json.dumps({"part": "edit", "pairs": len(hyps), "utterances": U, "nbest": NB, "mean_ref_len": round(sum(map(len, refs)) / U, 1),
                      "mean_hyp_len": round(sum(map(len, hyps)) / len(hyps), 1), "repeats": repeats, "same_counts_as_host": same,
                      "native_ms": round(k_ms[0], 3), "native_ms_min_max": [round(x, 3) for x in k_ms[1:]],
                      "native_with_ops_ms": round(k_ops_ms[0], 3), "host_pairs_timed": len(picks), "host_ms_per_pair": round(h_ms, 2),
                      "host_ms_all_pairs_scaled": round(h_ms * len(hyps), 1), "speedup_scaled": round(h_ms * len(hyps) / k_ms[0], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-pairs", type=int, default=8)
    ap.add_argument("--part", choices=["greedy", "edit", "both"], default="both")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    assert a.repeats >= 5, "the median of at least 5"
    dev = torch.device("cuda:0")
    if a.part in ("greedy", "both"):
        greedy(dev, a.repeats)
    if a.part in ("edit", "both"):
        edit(dev, a.repeats, a.host_pairs)


if __name__ == "__main__":
    main()
