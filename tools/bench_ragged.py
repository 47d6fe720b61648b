#!/usr/bin/env python3
"""What exact per-utterance encoding costs on a ragged batch: 64 utterances with lengths uniform in 10 - 40 s (drawn
once), conmamba_large_ctc (18 layers, d_model 256) in bf16, waveform to encoder rows, ms per call for three routes that alternate in
one process:

    padded   ConMambaASR.encode(wavs, wav_lens)               the batch as it is padded; wav_lens ignored (the reference's semantics)
    ragged   ConMambaASR.encode(wavs, wav_lens, ragged=True)  every utterance as if alone, one batch (the kernels with lengths)
    solo     64 x ConMambaASR.encode(wavs[b:b+1, :n[b]])      the only exact route without them

Eager launches from Python, host clock around a device synchronise, median of --repeats calls.  Also printed: the largest difference
between the ragged rows and the solo rows, and between the padded rows and the solo rows (what padding does to the answer).

    python tools/bench_ragged.py [--batch 64] [--min-s 10] [--max-s 40] [--layers 18] [--repeats 5] [--out profiles/ragged/bench_ragged.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--min-s", type=float, default=10.0)
ap.add_argument("--max-s", type=float, default=40.0)
ap.add_argument("--layers", type=int, default=18)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU timing says nothing about it"
dev = "cuda"
SR = 16000
g = torch.Generator().manual_seed(11)
n = torch.randint(int(args.min_s * SR), int(args.max_s * SR) + 1, (args.batch,), generator=g).tolist()
n[0] = int(args.max_s * SR)                                      # the batch is as wide as its longest utterance can be
model = ConMambaASR(ASRConfig("conmamba_large_ctc", num_encoder_layers=args.layers)).to(dev).eval()
wavs, ones = synthetic_wavs(args.batch, max(n), 5, dev)
for b, x in enumerate(n):
    wavs[b, x:] = 0.0                                             # silence behind every utterance: the kindest padding
counts = torch.tensor(n, device=dev)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def padded():
    return model.encode(wavs, ones)


def ragged():
    return model.encode(wavs, counts, ragged=True)[0]


def solo():
    return [model.encode(wavs[b:b + 1, :x], ones[:1]) for b, x in enumerate(n)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
    model.calibrate(wavs, ones)
    p, (r, row_lens), s = padded(), model.encode(wavs, counts, ragged=True), solo()
    torch.cuda.synchronize()
    d_ragged = max(float((r[b, :k] - s[b][0]).abs().max()) for b, k in enumerate(row_lens))
    d_padded = max(float((p[b, :k] - s[b][0]).abs().max()) for b, k in enumerate(row_lens) if k < p.shape[1])
    routes = {"padded": padded, "ragged": ragged, "solo": solo}
    for fn in routes.values():
        timed(fn)
    ms = {k: [] for k in routes}
    for _ in range(args.repeats):                                 # alternate the routes
        for k, fn in routes.items():
            ms[k].append(timed(fn))
rows, total = sum(row_lens), args.batch * r.shape[1]
say(f"{args.batch} utterances, {args.min_s:g} - {args.max_s:g} s (mean {sum(n) / len(n) / SR:.1f} s), {args.layers} layers, bf16; "
    f"{rows} valid encoder rows of {total} in the padded batch ({rows / total:.3f})")
base = statistics.median(ms["padded"])
for k in routes:
    med = statistics.median(ms[k])
    say(f"{k:7s}: {med:9.3f} ms per call (min {min(ms[k]):.3f}, max {max(ms[k]):.3f} over {args.repeats} calls), {med / base:.3f} of padded")
say(f"largest |difference| to the solo rows: ragged {d_ragged:.3e}, padded {d_padded:.3e}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
