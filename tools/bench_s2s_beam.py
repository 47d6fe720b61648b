"""Cost of the S2S beam search (s2s_decode.S2SBeamSearcher on cm_beam_select) on the GPU, at the configuration of
tools/bench_s2s_decode.py (S2S-large dims D 512, 6 decoder layers, 4 utterances, 4000 memory frames, 5000 tokens, bf16 autocast) and
at the recipes' beams 10 and 66:

  (a) ops.beam_select alone against the torch selection (s2s_decode.select_torch: mask, scale-add, broadcast add, topk, div / mod,
      gather) on the same inputs, with the CTC term: device events around `iters` calls after warm-up, the two alternating over three
      rounds; all rounds and the spread are reported;
  (b) the searcher's ms per token (the slope between a 16- and a 48-token search, <eos> barred) with the native selection and with
      the torch one, with and without ctc_weight 0.4, alternating over three rounds;
  (c) device kernels per token of both routes, from the profiler's kernel records.

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
from mamba_asr_amd.s2s_decode import S2SBeamSearcher, select_torch  # noqa: E402

BLANK, EOS = 0, 2
BEAMS = (10, 66)


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def selection(out):
    dev = torch.device("cuda:0")
    U, V = 4, 5000
    gen = torch.Generator().manual_seed(0)
    for B in BEAMS:
        att = torch.log_softmax(torch.randn(U * B, V, generator=gen) * 3.0, dim=-1).to(dev)
        delta = (-torch.rand(U * B, V, generator=gen) * 30.0).to(dev)
        alive = (-torch.rand(U * B, generator=gen) * 20.0).to(dev)
        blocked = torch.zeros(U, dtype=torch.int32, device=dev)
        routes = {"native": lambda: ops.beam_select(att, alive, B, EOS, delta=delta, weight=0.4, eos_blocked=blocked),
                  "torch": lambda: select_torch(att, alive, B, EOS, delta=delta, weight=0.4, eos_blocked=blocked)}
        a, b = routes["native"](), routes["torch"]()
        res = {"same_tokens": bool(torch.equal(a[3], b[3]) and torch.equal(a[2], b[2]) and torch.equal(a[0], b[0])),
               "native_ms": [], "torch_ms": []}
        for fn in routes.values():
            for _ in range(10):
                fn()
        for _ in range(3):
            for name, fn in routes.items():
                res[name + "_ms"].append(round(events_ms(fn, 100), 4))
        for name in routes:
            ms = res[name + "_ms"]
            res[name + "_spread"] = round((max(ms) - min(ms)) / min(ms), 3)
        res["speedup_min_over_min"] = round(min(res["torch_ms"]) / min(res["native_ms"]), 2)
        res["bytes_read"] = 2 * U * B * V * 4
        res["native_GBps"] = round(res["bytes_read"] / min(res["native_ms"]) / 1e6, 1)
        out[f"select_beam_{B}"] = res


def searcher(out):
    from mamba_asr_amd.modules.TransformerASR import TransformerASR
    dev = torch.device("cuda:0")
    U, T, D, layers, V = 4, 4000, 512, 6, 5000
    torch.manual_seed(0)
    m = TransformerASR(tgt_vocab=V, input_size=640, d_model=D, nhead=4, num_encoder_layers=1, num_decoder_layers=layers, d_ffn=2048,
                       dropout=0.1, activation=nn.GELU, encoder_module="conmamba", decoder_module="mamba", attention_type="RelPosMHAXL",
                       normalize_before=True, causal=False,
                       mamba_config={"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}).to(dev).eval()
    seq_lin, ctc_lin = nn.Linear(D, V).to(dev), nn.Linear(D, V).to(dev)
    enc, lens = torch.randn(U, T, D, device=dev), torch.ones(U, device=dev)
    routes = {"native": ops.beam_select, "torch": select_torch}

    def make(tokens, weight, beam, route):
        # <eos> is barred (min_decode_ratio 1), so every search runs exactly `tokens` steps
        return S2SBeamSearcher(modules=[m, seq_lin, ctc_lin], beam_size=beam, bos_index=1, eos_index=EOS, min_decode_ratio=1.0,
                               max_decode_ratio=(tokens + 0.5) / T, ctc_weight=weight, blank_index=BLANK, select_fn=routes[route])

    def run(tokens, weight, beam, route):
        s = make(tokens, weight, beam, route)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        log_probs = s(enc, lens)[3]
        torch.cuda.synchronize()
        assert log_probs.shape[1] == tokens
        return (time.perf_counter() - t0) * 1e3

    res = {"utterances": U, "memory_frames": T, "d_model": D, "decoder_layers": layers, "vocab": V, "dtype": "bf16"}
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for beam in BEAMS:
            for name, w in (("attention_only", 0.0), ("joint_ctc_0.4", 0.4)):
                for route in routes:
                    run(4, w, beam, route)
                slopes = {route: [] for route in routes}
                for _ in range(3):
                    for route in routes:
                        t16, t48 = run(16, w, beam, route), run(48, w, beam, route)
                        slopes[route].append(round((t48 - t16) / 32, 4))
                for route in routes:
                    res[f"beam_{beam}_{name}_{route}_ms_per_token"] = slopes[route]
            from torch.profiler import ProfilerActivity, profile
            for route in routes:
                counts = []
                for tokens in (4, 14):
                    s = make(tokens, 0.4, beam, route)
                    with profile(activities=[ProfilerActivity.CUDA]) as prof:
                        s(enc, lens)
                        torch.cuda.synchronize()
                    counts.append(len([e for e in prof.events() if str(e.device_type).endswith("CUDA")
                                       and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]))
                res[f"beam_{beam}_joint_{route}_kernels_per_token"] = (counts[1] - counts[0]) / 10
    out["searcher"] = res


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    out = {}
    with torch.no_grad():
        selection(out)
    searcher(out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
