"""Cost of the stepped Transformer decoder's cross-attention (modules/Transformer.py on cm_xattn_step) on the GPU, at
the large recipe's dims (hparams/S2S/conmamba_large.yaml: 6 decoder layers, d_model 512, 8 heads, d_ffn 2048) and its two decoding
shapes, bf16:
    test   U = 1 utterance, beam 66, T = 875 memory frames (batch 1, test_beam_size 66, a 35 s utterance)
    valid  U = 8 utterances, beam 10, T = 300 frames

  (a) ops.xattn_step alone against ops.xattn_step_torch in its grouped form (one (B, dh) x (dh, T) product per utterance and
      head, a length mask, softmax, the product with V: no gather, no host read) on the same inputs: device events around 200
      calls after warm-up, the two alternating over five rounds; all rounds and their spread reported, with the bytes of K and V a
      call has to read and the rate that makes;
  (b) TransformerDecoder.step (6 layers, bf16 autocast): ms per token over positions 8 .. 39, with a reorder per token, on
      CM_XATTN_STEP=1 (cm_xattn_step) against =0 (the torch route; the self-attention stays on cm_attn_step for both), five
      alternating rounds.

Prints one JSON line."""
import json
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.modules.Transformer import TransformerDecoder  # noqa: E402

DEV = torch.device("cuda:0")
D, H, LAYERS, FFN = 512, 8, 6, 2048
SHAPES = {"test_U1_B66_T875": (1, 66, 875), "valid_U8_B10_T300": (8, 10, 300)}
ROUTES = {"native": ops.xattn_step, "torch": lambda *a: ops.xattn_step_torch(*a, grouped=True)}
ROUNDS = 5


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
    # the native route is the default only where its minimum is below the torch route's by more than both spreads
    res["native_faster_beyond_spreads"] = bool(min(res["native_ms"]) * (1 + res["native_spread"] + res["torch_spread"]) < min(res["torch_ms"]))


def kernel(out):
    gen = torch.Generator().manual_seed(0)
    for tag, (U, B, T) in SHAPES.items():
        R = U * B
        q = torch.randn(R, D, generator=gen).to(DEV, torch.bfloat16)
        kv = torch.randn(U, T, 2 * D, generator=gen).to(DEV, torch.bfloat16)
        k, v = kv[..., :D], kv[..., D:]
        row_utt = torch.arange(U, dtype=torch.int32, device=DEV).repeat_interleave(B)
        enc_len = torch.full((U,), T, dtype=torch.int32, device=DEV)
        fns = {name: (lambda fn=fn: fn(q, k, v, row_utt, enc_len, H)) for name, fn in ROUTES.items()}
        a, b = fns["native"]().float(), fns["torch"]().float()
        res = {"max_abs_diff": round(float((a - b).abs().max()), 5), "native_ms": [], "torch_ms": []}
        for fn in fns.values():
            for _ in range(20):
                fn()
        for _ in range(ROUNDS):
            for name, fn in fns.items():
                res[name + "_ms"].append(round(events_ms(fn, 200), 4))
        summarise(res)
        res["kv_bytes"] = 2 * U * T * D * 2                          # what a call must read at least once (L2-resident: 1.8 MB / 4.9 MB)
        res["native_kv_GBps_if_read_once"] = round(res["kv_bytes"] / min(res["native_ms"]) / 1e6, 1)
        res["native_kv_GBps_as_issued"] = round(res["kv_bytes"] * B / min(res["native_ms"]) / 1e6, 1)   # every row reads its utterance's K and V
        out["xattn_step_" + tag] = res


def decoder_step(out):
    torch.manual_seed(0)
    dec = TransformerDecoder(num_layers=LAYERS, nhead=H, d_ffn=FFN, d_model=D, activation=nn.GELU, normalize_before=True,
                             causal=True).to(DEV).eval()
    assert dec.attn_fn is ops.attn_step
    routes = {"native": ops.xattn_step, "torch": ops.xattn_step_torch}       # as CM_XATTN_STEP=1 / =0 select them
    for tag, (U, B, T) in SHAPES.items():
        R = U * B
        memory = torch.randn(U, T, D, device=DEV)
        x = torch.randn(R, 1, D, device=DEV)
        widen = torch.arange(U, device=DEV).repeat_interleave(B)
        rows = (torch.arange(U, device=DEV) * B).repeat_interleave(B) + torch.randint(0, B, (R,), device=DEV)   # parents inside the utterance

        def run(route, steps, timed_from):
            dec.xattn_fn = routes[route]
            state = dec.init_state(memory).reorder(widen)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for t in range(steps):
                if t == timed_from:
                    e0.record()
                dec.step(x, state)
                state.reorder(rows)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / (steps - timed_from)

        res = {"native_ms": [], "torch_ms": [], "layers": LAYERS, "rows": R}
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            for route in routes:
                run(route, 8, 0)
            for _ in range(ROUNDS):
                for route in routes:
                    res[route + "_ms"].append(round(run(route, 40, 8), 4))
        summarise(res)
        out["decoder_step_" + tag] = res
    dec.xattn_fn = ops.xattn_step


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    out = {}
    with torch.no_grad():
        kernel(out)
    decoder_step(out)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
