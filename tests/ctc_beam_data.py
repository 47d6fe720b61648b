"""Synthetic CTC posteriors for the beam-search tests and benchmark (seeded, host-generated)."""
import torch

# a 31-piece SentencePiece character vocabulary shaped like the CTC recipe's (blank / bos / eos control pieces, the word
# boundary piece and 27 characters)
SPM_VOCAB = ["<unk>", "<s>", "</s>", "▁"] + [chr(ord("A") + i) for i in range(26)] + ["'"]
RECIPE = dict(blank_index=0, beam_size=100, beam_prune_logp=-12.0, token_prune_min_logp=-1.2, prune_history=False)


def peaky(T, V, seed):
    """A random label path through blanks, plus noise: one token dominates most frames."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, V, generator=g) * 0.7
    lab = torch.randint(1, V, (T,), generator=g)
    blank = torch.rand(T, generator=g) < 0.6
    lab = torch.where(blank, torch.zeros_like(lab), lab)
    logits[torch.arange(T), lab] += 7.0
    return torch.log_softmax(logits, dim=-1)


def competing(T, V, seed):
    """2-3 tokens above log 0.3 in most frames, so that a beam of 100 really fills."""
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(T, V, generator=g) * 0.3
    for t in range(T):
        k = 2 + int(torch.randint(0, 2, (1,), generator=g))
        idx = torch.randperm(V, generator=g)[:k]
        logits[t, idx] += (5.2 if k == 3 else 4.5) + torch.randn(k, generator=g) * 0.15
    return torch.log_softmax(logits, dim=-1)
