#!/usr/bin/env python3
"""Time per ConmambaEncoder.forward_streaming call of the 18-layer, d_model 256 causal encoder in bf16 (the CTC-large width):
the native route against the generic prepend-history route (CM_STREAM_NATIVE=0), alternating in one process, at
(streams, frames per chunk) = (1, 16), (64, 16), (64, 64).  Eager launches from Python, host clock around a device synchronise;
one encoder frame is 40 ms of audio, so a chunk of t frames is t * 40 ms of real time per stream.

    python tools/bench_streaming.py [--layers 18] [--calls 200] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

from mamba_asr_amd import fused
from mamba_asr_amd.modules.Conmamba import ConmambaEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=18)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU timing says nothing about it"
dev = "cuda"
torch.manual_seed(1)
enc = ConmambaEncoder(num_layers=args.layers, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True, dropout=0.0,
                      causal=True, mamba_config={"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True})
for p in enc.parameters():
    if p.dim() > 1:
        nn.init.xavier_normal_(p)
enc = enc.to(dev).eval()
FRAME_MS = 40.0


def window(ctx, chunks, native):
    """ms per call over one window of len(chunks) calls."""
    fused.USE_STREAM_NATIVE = native
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for c in chunks:
            enc.forward_streaming(c, ctx)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(chunks)


for streams, frames in ((1, 16), (64, 16), (64, 64)):
    chunks = [torch.randn(streams, frames, 256, device=dev) for _ in range(args.calls)]
    ctxs = {n: enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16) for n in (True, False)}
    for n in (True, False):                                        # warm up both routes at this shape
        window(ctxs[n], chunks[:20], n)
    # the two routes compute the same thing: one chunk from fresh contexts, compared before anything is timed
    a, b = (enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16) for _ in range(2))
    with torch.no_grad():
        fused.USE_STREAM_NATIVE = True
        ya = enc.forward_streaming(chunks[0], a)[0]
        fused.USE_STREAM_NATIVE = False
        yb = enc.forward_streaming(chunks[0], b)[0]
    diff = (ya - yb).abs()
    ms = {True: [], False: []}
    for _ in range(args.repeats):                                  # alternate the routes
        for n in (True, False):
            ms[n].append(window(ctxs[n], chunks, n))
    audio = frames * FRAME_MS
    for n in (True, False):
        med, lo, hi = statistics.median(ms[n]), min(ms[n]), max(ms[n])
        print(f"streams {streams:3d} frames {frames:3d} {'native ' if n else 'generic'}: {med:7.3f} ms per call (min {lo:.3f}, max {hi:.3f} over "
              f"{args.repeats} windows of {args.calls} calls) = {audio / med:7.1f} x real time per stream, {streams * audio / med:9.1f} x in all",
              flush=True)
    print(f"    native / generic time {statistics.median(ms[True]) / statistics.median(ms[False]):.3f}; outputs of the two routes on one chunk: "
          f"max|diff| {diff.max():.3e} mean {diff.mean():.3e}", flush=True)
    # the native route as a serving loop would replay it: the row histories alternate between two buffers, so TWO consecutive
    # steps make one hipGraph (after them the context's buffers are where they were); device-bound time per call
    fused.USE_STREAM_NATIVE = True
    ctx = enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16)
    static = [chunks[0].clone(), chunks[1].clone()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        for c in static:
            enc.forward_streaming(c, ctx)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        outs = [enc.forward_streaming(c, ctx)[0] for c in static]
    ctx.reset()
    graph.replay()
    fresh = enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16)
    with torch.no_grad():
        same = all(torch.equal(enc.forward_streaming(c, fresh)[0], o) for c, o in zip(static, outs))
    reps = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls // 2):
            graph.replay()
        torch.cuda.synchronize()
        reps.append((time.perf_counter() - t0) * 1e3 / (args.calls // 2 * 2))
    med = statistics.median(reps)
    print(f"    native, two steps per hipGraph replay: {med:7.3f} ms per call (min {min(reps):.3f}, max {max(reps):.3f}) = {audio / med:7.1f} x real "
          f"time per stream, {streams * audio / med:9.1f} x in all; replay == eager: {same}", flush=True)
