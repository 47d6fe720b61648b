"""CTC beam search at the recipe's settings (hparams/CTC/conmamba_large.yaml:168-172): ms per 64 x 1000 x 31 batch on the GPU
(cm_ctc_beam_search alone, device events after warm-up) for peaky and competing posteriors, and ms per 1000-frame utterance for
the tests' float64 host restatement.  Prints one JSON line."""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_data as D  # noqa: E402
import ctc_beam_ref as R  # noqa: E402
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP, CTCBeamSearcher  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, V, iters = 64, 1000, 31, 10
    s = CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB)
    tc, th, tp = s._tables(dev)
    n = torch.full((B,), T, dtype=torch.int32, device=dev)
    out = {"batch": B, "frames": T, "vocab": V, "beam_size": 100}
    for name, gen in (("peaky", D.peaky), ("competing", D.competing)):
        lp = torch.stack([gen(T, V, 500 + b) for b in range(B)]).to(dev)

        def run():
            return ops.ctc_beam_search(lp, n, tc, th, tp, HASH_BASE, HASH_SEP, blank=0, beam_size=100, topk=1,
                                       beam_prune_logp=-12.0, token_prune_min_logp=-1.2)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        out[f"gpu_ms_per_batch_{name}"] = round(e0.elapsed_time(e1) / iters, 3)
        lp0 = lp[0].double().cpu().tolist()
        t0 = time.perf_counter()
        R.beam_search(lp0, T, D.SPM_VOCAB, blank=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2)
        out[f"host_ms_per_utt_{name}"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
