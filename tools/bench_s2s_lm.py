"""Cost of TransformerLM fusion in the S2S beam search (modules/TransformerLM.py on cm_attn_step) on the GPU:

  (a) ops.attn_step alone against ops.attn_step_torch (gather by the ancestry, matmul, softmax, matmul) on the same inputs at the
      recipes' LM dims (D 768, 12 heads), R 40 and 264 rows (beams 10 and 66 of 4 utterances), t 16 / 48 / 128 cached positions,
      bf16: device events around 100 calls after warm-up, the two alternating over three rounds; all rounds and the spread reported;
  (b) TransformerLM.step at 12 layers, d_ffn 3072, 5000 tokens, bf16 autocast: ms per token over positions 16 .. 47 for both
      attention routes (three alternating rounds), and device kernels per token from the profiler's kernel records;
  (c) the searcher's ms per token (the slope between a 16- and a 48-token search, <eos> barred) at tools/bench_s2s_beam.py's
      configuration, beams 10 and 66, joint CTC 0.4, without an LM and with lm_weight 0.6 on both attention routes.

The torch route measured in the same run is the comparison point.  Prints one JSON line (profiles/s2s_decode/)."""
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.modules.TransformerLM import TransformerLM  # noqa: E402
from mamba_asr_amd.s2s_decode import S2SBeamSearcher, TransformerLMScorer  # noqa: E402

BLANK, EOS = 0, 2
BEAMS = (10, 66)
ROUTES = {"native": ops.attn_step, "torch": ops.attn_step_torch}
DEV = torch.device("cuda:0")


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def summarise(res):
    for name in ROUTES:
        ms = res[name + "_ms"]
        res[name + "_spread"] = round((max(ms) - min(ms)) / min(ms), 3)
    res["speedup_min_over_min"] = round(min(res["torch_ms"]) / min(res["native_ms"]), 2)
    # the native route stays the default only where its minimum is below the torch route's by more than both spreads
    res["native_faster_beyond_spreads"] = bool(min(res["native_ms"]) * (1 + res["native_spread"] + res["torch_spread"]) < min(res["torch_ms"]))


def kernel(out):
    D, H = 768, 12
    gen = torch.Generator().manual_seed(0)
    for R in (40, 264):
        for t in (16, 48, 128):
            qkv = torch.randn(R, 3 * D, generator=gen).to(DEV, torch.bfloat16)
            kc, vc = (torch.randn(t + 1, R, D, generator=gen).to(DEV, torch.bfloat16) for _ in range(2))
            anc = torch.randint(0, R, (t + 1, R), generator=gen).int().to(DEV)
            fns = {name: (lambda fn=fn: fn(qkv, kc, vc, anc, t, H)) for name, fn in ROUTES.items()}
            a, b = fns["native"]().float(), fns["torch"]().float()
            res = {"max_abs_diff": round(float((a - b).abs().max()), 5), "native_ms": [], "torch_ms": []}
            for fn in fns.values():
                for _ in range(10):
                    fn()
            for _ in range(3):
                for name, fn in fns.items():
                    res[name + "_ms"].append(round(events_ms(fn, 100), 4))
            summarise(res)
            res["bytes_read"] = 2 * R * D * t * 2
            res["native_GBps"] = round(res["bytes_read"] / min(res["native_ms"]) / 1e6, 1)
            out[f"attn_step_R{R}_t{t}"] = res


def lm_step(out, lm):
    from torch.profiler import ProfilerActivity, profile
    for R in (40, 264):
        tokens = torch.randint(3, 5000, (R,), device=DEV)
        rows = torch.randint(0, R, (R,), device=DEV)

        def run(route, steps, timed_from=None):
            lm.attn_fn = ROUTES[route]
            state = lm.init_state(R, steps)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for t in range(steps):
                if t == timed_from:
                    e0.record()
                lm.step(tokens, state)
                state.reorder(rows)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / (steps - timed_from) if timed_from is not None else None

        res = {"native_ms": [], "torch_ms": []}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            for route in ROUTES:
                run(route, 8)
            for _ in range(3):
                for route in ROUTES:
                    res[route + "_ms"].append(round(run(route, 48, 16), 4))
            for route in ROUTES:
                counts = []
                for steps in (4, 14):
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        run(route, steps)
                    counts.append(len([e for e in prof.events() if str(e.device_type).endswith("CUDA")
                                       and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]))
                res[route + "_kernels_per_token"] = (counts[1] - counts[0]) / 10
        summarise(res)
        out[f"lm_step_R{R}"] = res
    lm.attn_fn = ops.attn_step


def searcher(out, lm):
    from mamba_asr_amd.modules.TransformerASR import TransformerASR
    U, T, D, layers, V = 4, 4000, 512, 6, 5000
    torch.manual_seed(0)
    m = TransformerASR(tgt_vocab=V, input_size=640, d_model=D, nhead=4, num_encoder_layers=1, num_decoder_layers=layers, d_ffn=2048,
                       dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="mamba", attention_type="RelPosMHAXL",
                       normalize_before=True, causal=False,
                       mamba_config={"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}).to(DEV).eval()
    seq_lin, ctc_lin = nn.Linear(D, V).to(DEV), nn.Linear(D, V).to(DEV)
    enc, lens = torch.randn(U, T, D, device=DEV), torch.ones(U, device=DEV)
    scorer = TransformerLMScorer(lm, temperature=1.15)

    def run(tokens, beam, route):
        extra = {}
        if route != "no_lm":
            lm.attn_fn = ROUTES[route]
            extra = dict(lm_scorer=scorer, lm_weight=0.6)
        s = S2SBeamSearcher(modules=[m, seq_lin, ctc_lin], beam_size=beam, bos_index=1, eos_index=EOS, min_decode_ratio=1.0,
                            max_decode_ratio=(tokens + 0.5) / T, ctc_weight=0.4, blank_index=BLANK, temperature=1.15, **extra)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log_probs = s(enc, lens)[3]
        torch.cuda.synchronize()
        assert log_probs.shape[1] == tokens
        return (time.perf_counter() - t0) * 1e3

    res = {"utterances": U, "memory_frames": T, "d_model": D, "decoder_layers": layers, "vocab": V, "dtype": "bf16", "lm_layers": 12}
    routes = ("no_lm", "native", "torch")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for beam in BEAMS:
            for route in routes:
                run(4, beam, route)
            slopes = {route: [] for route in routes}
            for _ in range(3):
                for route in routes:
                    t16, t48 = run(16, beam, route), run(48, beam, route)
                    slopes[route].append(round((t48 - t16) / 32, 4))
            for route in routes:
                res[f"beam_{beam}_joint_ctc_0.4_{route}_ms_per_token"] = slopes[route]
    lm.attn_fn = ops.attn_step
    out["searcher"] = res


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    out = {}
    torch.manual_seed(0)
    lm = TransformerLM(5000, d_model=768, nhead=12, num_encoder_layers=12, d_ffn=3072).to(DEV).eval()
    with torch.no_grad():
        kernel(out)
        lm_step(out, lm)
    searcher(out, lm)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
