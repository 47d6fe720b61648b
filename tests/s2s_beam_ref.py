"""The S2S beam search contracts restated the slow way: helpers for the tests, no tests here.

  select       the per-token selection (ops.beam_select's contract) in torch, on any device: the same three fp32 operations, then
               a stable descending sort, which is the order (score descending, flat index ascending)
  beam_search  S2SBeamSearcher's loop and final ranking for ONE utterance on Python lists, one hypothesis at a time, each
               hypothesis scored by a ``logp(prefix)`` callback; the accumulation dtype is a parameter
"""
import math

import numpy as np
import torch

NEG = -math.inf


def select(att, alive, B, eos, delta=None, weight=0.0, eos_blocked=None):
    """att (U * B, V) fp32, alive (U * B) fp32, delta (U * B, V) fp32 or None, eos_blocked (U) or None
    -> (score, inc, parent, token), each (U, B); parent / token int32."""
    rows, V = att.shape
    U = rows // B
    a = att.clone()
    if eos_blocked is not None and 0 <= eos < V:
        blocked = eos_blocked.to(torch.bool).repeat_interleave(B)
        a[blocked, eos] = NEG
    inc = a
    if delta is not None:
        prod = weight * delta                                  # rounded to fp32
        inc = a + prod                                         # rounded again
    s = alive.unsqueeze(1) + inc
    s = torch.where(torch.isnan(s), torch.full_like(s, NEG), s)
    s = s.reshape(U, B * V)
    order = torch.sort(s, dim=1, descending=True, stable=True).indices[:, :B]     # equal scores keep their index order; +0 == -0
    score = s.gather(1, order)
    parent = torch.div(order, V, rounding_mode="floor")
    token = order - parent * V
    return score, inc.reshape(U, B * V).gather(1, order), parent.to(torch.int32), token.to(torch.int32)


def beam_search(logp, V, beam_size, bos, eos, min_steps, max_steps, length_normalization=True, topk=1, dtype=np.float64):
    """One utterance.  ``logp(prefix)`` -> the (V,) increments of extending ``prefix`` (a list that starts with <bos>), the
    weighted CTC term included when decoding jointly.  -> (ranked, gaps, steps):
      ranked  up to topk tuples (tokens, final score, raw score, increments along the path), best first
      gaps    per step the distance between the beam_size-th and the (beam_size + 1)-th candidate (inf when the latter is -inf)
      steps   how many steps the loop ran"""
    B = beam_size
    slots = [None] * B                                         # (prefix, raw score, increments) or None: dead
    slots[0] = ([bos], dtype(0), [])
    finished, gaps, steps, n_fin = [], [], 0, 0
    for t in range(max_steps):
        cands = []
        for k, slot in enumerate(slots):
            if slot is None:
                continue
            row = np.array(torch.as_tensor(logp(slot[0])).detach().cpu().numpy(), dtype=dtype)
            assert row.shape == (V,)
            if min_steps > t:
                row[eos] = NEG
            for c in range(V):
                s = slot[1] + row[c]
                if np.isnan(s):
                    s = dtype(NEG)
                cands.append((s, k * V + c, row[c]))
        cands.sort(key=lambda x: (-x[0], x[1]))
        at = lambda i: cands[i][0] if i < len(cands) else NEG
        gaps.append(math.inf if at(B) == NEG else float(at(B - 1) - at(B)))
        new = [None] * B
        for j, (s, flat, inc) in enumerate(cands[:B]):
            if s == NEG:
                break
            prefix, _, incs = slots[flat // V]
            c = flat % V
            if c == eos:
                finished.append((prefix[1:], s, t + 1, t, j, incs + [inc]))
                n_fin += 1
            else:
                new[j] = (prefix + [c], s, incs + [inc])
        slots = new
        steps = t + 1
        if n_fin >= B or all(s is None for s in slots):
            break
    for j, slot in enumerate(slots):
        if slot is not None and steps > 0:
            finished.append((slot[0][1:], slot[1], steps, steps, j, slot[2]))
    if max_steps == 0:
        finished.append(([], dtype(0), 0, 0, 0, []))
    final = lambda h: h[1] / dtype(max(h[2], 1)) if length_normalization else h[1]
    finished.sort(key=lambda h: (-final(h), h[3], h[4]))
    return [(h[0], final(h), h[1], h[5]) for h in finished[:topk]], gaps, steps
