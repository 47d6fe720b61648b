"""CTC forced alignment beside the CTC loss: ms per launch of cm_ctc_align and of cm_ctc_loss at the same shape on
the same build (device events around `iters` launches after warm-up), their ratio, and the share of cm_ctc_align spent behind the
forward pass -- backtrace, spans, label_logp -- measured as the difference to the same launch with the last frame at -inf: the
forward pass does not depend on the data, and an utterance without an alignment (status 1) skips everything behind it.
cm_ctc_loss takes at most 511 labels: at S = 1023 its column is null and both are also timed at S = 511.  Prints one JSON line per
shape."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mamba_asr_amd import ops  # noqa: E402

SHAPES = [(32, 1000, 31, 500), (64, 1000, 5000, 100), (1, 4000, 31, 1023), (1, 4000, 31, 511)]


def _ms(run, iters):
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    for B, T, V, S in SHAPES:
        g = torch.Generator().manual_seed(B * 7 + S)
        lp = torch.log_softmax(torch.randn(B, T, V, generator=g), dim=-1).to(dev)
        targets = torch.randint(1, V, (B, S), generator=g).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), S, dtype=torch.int32, device=dev)
        dead = lp.clone()
        dead[:, T - 1] = -float("inf")
        iters = 20 if B * T * V < 1e8 else 8
        status = ops.ctc_align(lp, targets, il, tl)[1]
        assert status.cpu().tolist() == [0] * B and ops.ctc_align(dead, targets, il, tl)[1].cpu().tolist() == [1] * B
        align = _ms(lambda: ops.ctc_align(lp, targets, il, tl), iters)
        forward = _ms(lambda: ops.ctc_align(dead, targets, il, tl), iters)
        align2 = _ms(lambda: ops.ctc_align(lp, targets, il, tl), iters)          # the spread of the same launch
        loss = _ms(lambda: ops.ctc_loss_grad(lp, targets, il, tl), iters) if S <= 511 else None
        print(json.dumps({"batch": B, "frames": T, "vocab": V, "labels": S, "iters": iters, "align_ms": round(align, 4),
                          "align_ms_again": round(align2, 4), "align_forward_only_ms": round(forward, 4),
                          "behind_forward_share": round(1 - forward / align, 3), "loss_ms": None if loss is None else round(loss, 4),
                          "align_over_loss": None if loss is None else round(align / loss, 3)}), flush=True)


if __name__ == "__main__":
    main()
