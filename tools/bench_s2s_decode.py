"""Per-token cost of S2S decoding at the S2S-large dims (hparams/S2S/conmambamamba_large.yaml: D 512, E 1024, dt_rank 32, 6 decoder
layers), batch 4, 4000 memory frames (160 s), bf16 autocast, on the GPU:

  (a) the full-prefix way of producing token i: TransformerASR.decode on the length-i prefix, at i = 32
  (b) TransformerASR.decode_step with the five-launch mixer step (CM_FUSED_STEP=0)
  (c) decode_step with cm_mamba_step
  and init_decode_state (the prefill over the memory), plus the native launches per token of (b) and (c) as ops.LAUNCH_LOG counts
  them (vendor GEMM / elementwise launches are not in that count; the kernel trace has them).

Timing: a host clock around `iters` calls that end in a device synchronise, after warm-up, (b) and (c) alternating, three rounds.
Prints one JSON line."""
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.modules.mamba import bimamba  # noqa: E402
from mamba_asr_amd.modules.TransformerASR import TransformerASR  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, D, prefix, layers = 4, 4000, 512, 32, 6
    torch.manual_seed(0)
    m = TransformerASR(tgt_vocab=5000, input_size=640, d_model=D, nhead=4, num_encoder_layers=1, num_decoder_layers=layers, d_ffn=2048,
                       dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="mamba", attention_type="RelPosMHAXL",
                       normalize_before=True, causal=False,
                       mamba_config={"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}).to(dev).eval()
    enc = torch.randn(B, T, D, device=dev)
    tgt = torch.randint(3, 5000, (B, prefix), device=dev)
    out = {"batch": B, "memory_frames": T, "d_model": D, "decoder_layers": layers, "prefix": prefix, "dtype": "bf16"}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for _ in range(3):
            m.decode(tgt, enc)
        out["a_full_prefix_decode_ms"] = [round(timed(lambda: m.decode(tgt, enc), 10), 3) for _ in range(3)]
        for _ in range(2):
            m.init_decode_state(enc)
        out["init_decode_state_ms"] = [round(timed(lambda: m.init_decode_state(enc), 5), 3) for _ in range(3)]
        state = m.init_decode_state(enc)
        tok = tgt[:, 0]

        def step():
            state.position = 0                                     # the cost of a step does not depend on the position
            m.decode_step(tok, state)

        res = {0: [], 1: []}
        for fused in (0, 1):
            bimamba.FUSED_STEP = bool(fused)
            for _ in range(20):
                step()
        for _ in range(3):
            for fused in (0, 1):
                bimamba.FUSED_STEP = bool(fused)
                res[fused].append(round(timed(step, 200), 4))
        out["b_decode_step_five_launch_ms"], out["c_decode_step_fused_ms"] = res[0], res[1]
        for fused in (0, 1):
            bimamba.FUSED_STEP = bool(fused)
            ops.LAUNCH_LOG = []
            step()
            torch.cuda.synchronize()
            names = [e[0] for e in ops.LAUNCH_LOG]
            ops.LAUNCH_LOG = None
            out["native_launches_per_token_" + ("fused" if fused else "five_launch")] = {n: names.count(n) for n in sorted(set(names))}
        # all device kernels per token, vendor GEMMs and elementwise kernels included, from the profiler's kernel records
        for fused in (0, 1):
            bimamba.FUSED_STEP = bool(fused)
            key = "kernels_per_token_" + ("fused" if fused else "five_launch")
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    for _ in range(10):
                        step()
                    torch.cuda.synchronize()
                kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
                out[key] = len(kernels) / 10
            except Exception as exc:                                # no tracer on this box: say so instead of guessing
                out[key] = f"not measured ({type(exc).__name__})"
        bimamba.FUSED_STEP = True
    print(json.dumps(out))


if __name__ == "__main__":
    main()
