#!/usr/bin/env python3
"""cm_ln_pw_glu vs cm_add_layernorm + library pointwise GEMM (rows = B x 1000, d_model 256), hipGraph-timed."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mamba_asr_amd import ops
from bench_ffn import timeit

dev = "cuda"
for b in (32, 64):
    rows, D = b * 1000, 256
    x = torch.randn(rows, D, device=dev)
    y = (torch.randn(rows, D, device=dev) * 0.5).bfloat16()
    ln = (torch.ones(D, device=dev), torch.zeros(D, device=dev), 1e-5)
    w = (torch.randn(2 * D, D, device=dev) / 16).bfloat16()
    bias = torch.randn(2 * D, device=dev) * 0.1
    wp = ops.PackedWeight(w)
    bb = bias.bfloat16()
    t1 = timeit(lambda: ops.ln_pw_glu(x, y, 0.0, ln, wp, bias))

    def lib():
        _, h = ops.add_layernorm(x, y, 0.0, x_out=x, norm2=ln, out_dtype=torch.bfloat16)
        return torch.addmm(bb, h, w.t())
    t2 = timeit(lib)
    mb = rows * (D * 4 * 2 + D * 2 * 2) / 1e6
    print(f"B={b}: ln_pw_glu {t1:6.1f} us ({mb / t1:5.2f} TB/s on {mb:.0f} MB)   add_ln + GEMM {t2:6.1f} us", flush=True)

# ---- the mixer's tail: library out_proj GEMM + cm_ln_pw_glu against cm_ln_pw_glu with the projection in front (cm_ln_pw_glu_mix),
# cycling through buffer sets whose total exceeds the 256 MB memory-side cache (in the encoder ycat was written by the scan and x by
# an FFN kernel, with ~1 GB of traffic in between)
K = 1024
for b in (32, 64):
    rows, D = b * 1000, 256
    ln = (torch.ones(D, device=dev), torch.zeros(D, device=dev), 1e-5)
    w = (torch.randn(2 * D, D, device=dev) / 16).bfloat16()
    bias = torch.randn(2 * D, device=dev) * 0.1
    wo = (torch.randn(D, K, device=dev) * 0.05).bfloat16()
    wp, wop = ops.PackedWeight(w), ops.PackedWeight(wo)
    nset = max(2, int(1.2e9 / (rows * (K * 2 + D * 4 + D * 2 + D * 2))))
    sets = [(torch.randn(rows, D, device=dev), torch.randn(rows, K, device=dev).bfloat16(), torch.empty(rows, D, device=dev, dtype=torch.bfloat16))
            for _ in range(nset)]
    state = {"i": 0}

    def pair():
        xs, yc, ys = sets[state["i"] % nset]
        state["i"] += 1
        torch.mm(yc, wo.t(), out=ys)
        ops.ln_pw_glu(xs, ys, 0.0, ln, wp, bias)

    def mix():
        xs, yc, _ = sets[state["i"] % nset]
        state["i"] += 1
        ops.ln_pw_glu(xs, None, 0.0, ln, wp, bias, ycat=yc, out_w=wop)
    res = [timeit(f, iters=2 * nset) for f in (pair, mix, pair, mix)]
    mb = rows * (K * 2 + D * 4 * 2 + D * 2) / 1e6
    print(f"B={b}: cold buffers ({nset} sets): GEMM + ln_pw_glu {res[0]:6.1f} / {res[2]:6.1f} us   projection inside {res[1]:6.1f} / {res[3]:6.1f} us "
          f"({mb / res[3]:5.2f} TB/s on {mb:.0f} MB)", flush=True)
    del sets
