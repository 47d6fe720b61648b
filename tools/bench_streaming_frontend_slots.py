#!/usr/bin/env python3
"""Time per call of the per-slot streamed front end (fused.frontend_streaming_slots) and of
ConMambaASR.encode_wav_slots against their lock-step forms, CTC-large settings with a causal encoder, bf16, native route, at
(streams, rows per call) = (1, 16), (64, 16), (64, 64): a call hands over at most rows * 640 samples per stream.  Columns,
alternating in one process: lock step, lock step again (the spread the lock-step route shows against itself), every slot full
(n_valid = n), and a ragged mix of sample counts uniform in [0, n] (drawn once).  tools/bench_streaming.py's protocol: eager
launches from Python, host clock around a device synchronise at the window's end, every shape warmed up first, median of --repeats
windows of --calls calls.

    python tools/bench_streaming_frontend_slots.py [--layers 18] [--calls 200] [--repeats 5]
"""
import argparse
import dataclasses
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mamba_asr_amd import fused
from mamba_asr_amd.asr import CONFIGS, ConMambaASR, synthetic_wavs

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=18)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU timing says nothing about it"
dev, BF16 = "cuda", torch.bfloat16
model = ConMambaASR(dataclasses.replace(CONFIGS["conmamba_large_ctc"], name="bench", num_encoder_layers=args.layers, causal=True)).to(dev).eval()
model.calibrate(*synthetic_wavs(4, 16000, 1, dev))
ROW_SAMPLES = 640
COLUMNS = ("lock step", "lock step (again)", "slots full", "slots ragged")


def timed(step, items):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        for x in items:
            step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(items)


for streams, rows in ((1, 16), (64, 16), (64, 64)):
    n = rows * ROW_SAMPLES
    wav, _ = synthetic_wavs(streams, n * 8, 2, dev)
    chunks = [wav[:, (i % 8) * n:(i % 8 + 1) * n] for i in range(args.calls)]
    g = torch.Generator().manual_seed(7)
    counts = {"slots full": [[n] * streams] * args.calls,
              "slots ragged": [torch.randint(0, n + 1, (streams,), generator=g).tolist() for _ in range(args.calls)]}
    for what in ("front end", "front end + encoder"):
        ctxs = {k: model.make_streaming_context(streams, BF16, per_slot=k.startswith("slots")) for k in COLUMNS}

        def step_of(k):
            ctx = ctxs[k]
            if not k.startswith("slots"):
                if what == "front end":
                    return lambda ic: fused.frontend_streaming(model, ic[1], ctx.frontend)
                return lambda ic: model.encode_wav_streaming(ic[1], ctx)
            if what == "front end":
                return lambda ic: fused.frontend_streaming_slots(model, ic[1], counts[k][ic[0]], ctx.frontend)
            return lambda ic: model.encode_wav_slots(ic[1], counts[k][ic[0]], ctx)
        items = list(enumerate(chunks))
        steps = {k: step_of(k) for k in COLUMNS}
        for k in COLUMNS:
            timed(steps[k], items[:20])
        ms = {k: [] for k in COLUMNS}
        for _ in range(args.repeats):
            for k in COLUMNS:
                ms[k].append(timed(steps[k], items))
        base = statistics.median(ms["lock step"])
        for k in COLUMNS:
            med = statistics.median(ms[k])
            print(f"streams {streams:3d} rows {rows:3d} {what:20s} {k:18s}: {med:7.3f} ms per call (min {min(ms[k]):.3f}, max {max(ms[k]):.3f} over "
                  f"{args.repeats} windows of {args.calls} calls), {med / base:.3f} of lock step", flush=True)
