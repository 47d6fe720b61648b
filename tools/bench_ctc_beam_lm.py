"""LM-fused CTC beam search next to the LM-free one on the same inputs: ms per 64 x 1000 x 31 batch at the recipe's settings
(the shape of tests/test_ctc_beam_search_gpu.py::test_benchmark_shape: even utterances competing, odd peaky), kernels alone, device
events after warm-up, the two searches alternating inside the timed loop.  Also the host time to parse and pack the test
generator's largest ARPA file.  Prints one JSON line."""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ctc_beam_data as D  # noqa: E402
import ctc_lm_data as LD  # noqa: E402
from mamba_asr_amd import ops  # noqa: E402
from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP, CTCBeamSearcher  # noqa: E402
from mamba_asr_amd.ngram_lm import NgramLM  # noqa: E402


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    B, T, V, iters = 64, 1000, 31, 10
    out = {"batch": B, "frames": T, "vocab": V, "beam_size": 100}
    with tempfile.TemporaryDirectory() as d:
        big, _ = LD.make_arpa(os.path.join(d, "big.arpa"), seed=1, **LD.LARGEST)
        t0 = time.perf_counter()
        lm_big = NgramLM.from_arpa(big)
        out["arpa_pack_ms_largest"] = round((time.perf_counter() - t0) * 1e3, 1)
        out["arpa_ngrams_largest"] = lm_big.n_entries
        path, _ = LD.make_arpa(os.path.join(d, "m.arpa"), seed=4, n_words=(18, 300, 300), n_bigrams=400, n_trigrams=300)
        s = CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path)
    lm = s.lm
    tc, th, tp = s._tables(dev)
    tl, tables = s._tok_len(dev), lm.tables(dev)
    n = torch.full((B,), T, dtype=torch.int32, device=dev)
    lp = torch.stack([(D.competing if b % 2 == 0 else D.peaky)(T, V, 900 + b) for b in range(B)]).to(dev)
    common = dict(blank=0, beam_size=100, topk=1, beam_prune_logp=-12.0, token_prune_min_logp=-1.2)

    def free():
        return ops.ctc_beam_search(lp, n, tc, th, tp, HASH_BASE, HASH_SEP, **common)

    def fused():
        return ops.ctc_beam_search_lm(lp, n, tc, th, tp, tl, HASH_BASE, HASH_SEP, tables, order=lm.order, n_words=len(lm.words),
                                      lm_bos=lm.bos, lm_eos=lm.eos, lm_unk=lm.unk, alpha=s.alpha, beta=s.beta,
                                      unk_score_offset=s.unk_score_offset, **common)
    for _ in range(2):
        free()
        fused()
    torch.cuda.synchronize()
    ms = {"free": 0.0, "fused": 0.0}
    for _ in range(iters):
        for name, fn in (("free", free), ("fused", fused)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name] += e0.elapsed_time(e1)
    out["gpu_ms_per_batch_lm_free"] = round(ms["free"] / iters, 3)
    out["gpu_ms_per_batch_lm_fused"] = round(ms["fused"] / iters, 3)
    out["ratio"] = round(ms["fused"] / ms["free"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
