#!/usr/bin/env python3
"""Time per call of the streamed front end (fused.frontend_streaming) and of ConMambaASR.encode_wav_streaming, CTC-large settings
with a causal encoder, bf16, at (streams, rows per call) = (1, 16), (64, 16), (64, 64): a call hands over rows * 640 samples per
stream (16 rows = 10240 samples = 640 ms).
  * the front-end call alone, native route against the generic torch route (CM_STREAM_FRONT_NATIVE=0), alternating in one process;
  * encode_wav_streaming (front end + src Linear + encoder) against encode_streaming fed precomputed rows (the path without this
    stage), alternating.
tools/bench_streaming.py's protocol: eager launches from Python, host clock around a device synchronise at the window's end, every
shape warmed up first, median of --repeats windows of --calls calls.

    python tools/bench_streaming_frontend.py [--layers 18] [--calls 200] [--repeats 5]
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
ROW_SAMPLES, ROW_MS = 640, 40.0


def timed(step, items):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        for x in items:
            step(x)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(items)


def report(label, streams, rows, ms):
    med, audio = statistics.median(ms), rows * ROW_MS
    print(f"streams {streams:3d} rows {rows:3d} {label:34s}: {med:7.3f} ms per call (min {min(ms):.3f}, max {max(ms):.3f} over {args.repeats} "
          f"windows of {args.calls} calls) = {audio / med:7.1f} x real time per stream", flush=True)
    return med


for streams, rows in ((1, 16), (64, 16), (64, 64)):
    n = rows * ROW_SAMPLES
    wav, _ = synthetic_wavs(streams, n * 8, 2, dev)
    chunks = [wav[:, (i % 8) * n:(i % 8 + 1) * n] for i in range(args.calls)]
    pre = [torch.randn(streams, rows, 640, device=dev).to(BF16) for _ in range(8)]
    pre = [pre[i % 8] for i in range(args.calls)]
    front = {nat: fused.FrontEndStreamingContext(streams, dev, BF16) for nat in (True, False)}
    full = model.make_streaming_context(streams, dtype=BF16)
    enc_only = model.make_streaming_context(streams, dtype=BF16)

    def front_step(nat):
        def step(x):
            fused.USE_STREAM_FRONT_NATIVE = nat
            return fused.frontend_streaming(model, x, front[nat])
        return step

    def wav_step(x):
        fused.USE_STREAM_FRONT_NATIVE = True
        return model.encode_wav_streaming(x, full)

    steps = {"front end, native": (front_step(True), chunks), "front end, generic": (front_step(False), chunks),
             "encode_wav_streaming": (wav_step, chunks), "encode_streaming (rows given)": (lambda x: model.encode_streaming(x, enc_only.encoder), pre)}
    for step, items in steps.values():                              # warm up every route at this shape
        timed(step, items[:20])
    # the two front-end routes compute the same thing: fresh contexts, two calls, compared before anything is timed
    a, b = fused.FrontEndStreamingContext(streams, dev, BF16), fused.FrontEndStreamingContext(streams, dev, BF16)
    with torch.no_grad():
        fused.USE_STREAM_FRONT_NATIVE = True
        ya = torch.cat([fused.frontend_streaming(model, c, a) for c in chunks[:2]], dim=1).float()
        fused.USE_STREAM_FRONT_NATIVE = False
        yb = torch.cat([fused.frontend_streaming(model, c, b) for c in chunks[:2]], dim=1).float()
    diff = (ya - yb).abs()
    ms = {k: [] for k in steps}
    for _ in range(args.repeats):                                   # alternate
        for k, (step, items) in steps.items():
            ms[k].append(timed(step, items))
    med = {k: report(k, streams, rows, v) for k, v in ms.items()}
    print(f"    front end native / generic time {med['front end, native'] / med['front end, generic']:.3f}; rows of the two routes over two calls: "
          f"max|diff| {diff.max():.3e} mean {diff.mean():.3e}", flush=True)
    print(f"    encode_wav_streaming - encode_streaming = {1e3 * (med['encode_wav_streaming'] - med['encode_streaming (rows given)']):.0f} us per call "
          f"(the front end's three launches and the rows' allocation)", flush=True)
fused.USE_STREAM_FRONT_NATIVE = True
