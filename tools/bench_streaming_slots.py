#!/usr/bin/env python3
"""Time per ConmambaEncoder.forward_streaming call with per-slot lengths against the lock-step call, 18-layer,
d_model 256 causal encoder in bf16, native route, at (streams, frames per call) = (1, 16), (64, 16), (64, 64).  Four columns
alternate in one process: lock step, lock step again (the spread the lock-step route shows against itself), lens = t for every
slot, and a ragged mix of lengths uniform in [0, t] (fixed per call, drawn once).  Eager launches from Python, host clock around a
device synchronise, median of --repeats windows of --calls calls, as tools/bench_streaming.py.

    python tools/bench_streaming_slots.py [--layers 18] [--calls 200] [--repeats 5]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn

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
COLUMNS = ("lock step", "lock step (again)", "lens full", "lens ragged")


def window(ctx, chunks, lens):
    """ms per call over one window; lens: None, or one (B,) int32 device tensor per call."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for i, c in enumerate(chunks):
            enc.forward_streaming(c, ctx, lens=None if lens is None else lens[i])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(chunks)


for streams, frames in ((1, 16), (64, 16), (64, 64)):
    chunks = [torch.randn(streams, frames, 256, device=dev) for _ in range(args.calls)]
    g = torch.Generator().manual_seed(7)
    full = [torch.full((streams,), frames, dtype=torch.int32, device=dev)] * args.calls
    ragged = [torch.randint(0, frames + 1, (streams,), generator=g).to(torch.int32).to(dev) for _ in range(args.calls)]
    lens = {"lock step": None, "lock step (again)": None, "lens full": full, "lens ragged": ragged}
    ctxs = {k: enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16) for k in COLUMNS}
    # lens = t is the lock-step call: one chunk from fresh contexts, compared before anything is timed
    a, b = (enc.make_streaming_context(None, batch_size=streams, dtype=torch.bfloat16) for _ in range(2))
    with torch.no_grad():
        same = torch.equal(enc.forward_streaming(chunks[0], a)[0], enc.forward_streaming(chunks[0], b, lens=full[0])[0])
    for k in COLUMNS:
        window(ctxs[k], chunks[:20], None if lens[k] is None else lens[k][:20])
    ms = {k: [] for k in COLUMNS}
    for _ in range(args.repeats):                                  # alternate the columns
        for k in COLUMNS:
            ms[k].append(window(ctxs[k], chunks, lens[k]))
    base = statistics.median(ms["lock step"])
    for k in COLUMNS:
        med = statistics.median(ms[k])
        print(f"streams {streams:3d} frames {frames:3d} {k:18s}: {med:7.3f} ms per call (min {min(ms[k]):.3f}, max {max(ms[k]):.3f} over "
              f"{args.repeats} windows of {args.calls} calls), {med / base:.3f} of lock step", flush=True)
    print(f"    lens = t equals the lock-step call bit for bit on one chunk: {same}; mean ragged length "
          f"{float(torch.stack(ragged).float().mean()):.1f} of {frames}", flush=True)
