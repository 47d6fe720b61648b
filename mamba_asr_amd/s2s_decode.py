"""Greedy S2S search on the stepped Mamba decoder: what a recipe's ``valid_search`` / ``test_search`` slot takes
(reference train_S2S.py:388-394 unpacks ``hyps, _, _, _ = searcher(enc_out, wav_lens)``; the reference fills the slot with
speechbrain's S2STransformerBeamSearcher, which re-runs ``TransformerASR.decode`` over the whole prefix for every token).

Here each token costs one ``TransformerASR.decode_step``: the decoder's state (modules/Conmamba.py DecoderState) has a
constant size, and the scan over the encoder frames is done once, by ``init_decode_state``.  Beam search, CTC / LM
scoring and temperature are not provided.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch


class S2SGreedySearcher:
    """``searcher(enc_states, wav_lens) -> (hyps, lengths, scores, log_probs)``

    enc_states (batch, T, d_model), wav_lens (batch,) relative lengths in (0, 1].  With enc_len = round(T * wav_lens):
      * a row stops at its first <eos> at or after step floor(min_decode_ratio * enc_len) (counting from 0); before
        that step <eos> cannot be chosen (its log-probability is masked to -inf);
      * every row stops after floor(max_decode_ratio * max(enc_len)) steps;
      * a finished row keeps stepping on <eos> with its score frozen, so the batch shape never changes.
    hyps: per utterance the list of chosen tokens, without <bos> / <eos>; lengths (batch,) long: their counts;
    scores (batch,) fp32: the sum of the chosen tokens' log-probabilities, the closing <eos> included;
    log_probs (batch, steps) fp32: each chosen token's log-probability, 0 behind a row's <eos>.

    ``modules`` = [transformer (TransformerASR), seq_lin]: the default per-token function is
    log_softmax(seq_lin(transformer.decode_step(tokens, state))) on the state of transformer.init_decode_state.  Both are
    injectable -- ``init_fn(enc_states) -> state`` and ``step_fn(tokens (batch,) long, state) -> (log_probs (batch, vocab),
    state)`` -- which is also how the host logic is tested without a GPU.

    The loop reads one flag per token from the device (have all rows finished?); everything else stays on the device.
    """

    def __init__(self, modules=None, bos_index: int = 1, eos_index: int = 2, min_decode_ratio: float = 0.0,
                 max_decode_ratio: float = 1.0, step_fn: Optional[Callable] = None, init_fn: Optional[Callable] = None):
        if step_fn is None or init_fn is None:
            if modules is None or len(modules) != 2:
                raise ValueError("S2SGreedySearcher needs modules=[transformer, seq_lin] (or step_fn and init_fn)")
            transformer, seq_lin = modules

            def default_init(enc_states):
                return transformer.init_decode_state(enc_states)

            def default_step(tokens, state):
                out = transformer.decode_step(tokens, state)                      # (batch, 1, d_model)
                return torch.log_softmax(seq_lin(out)[:, 0].float(), dim=-1), state

            init_fn, step_fn = init_fn or default_init, step_fn or default_step
        self.init_fn, self.step_fn = init_fn, step_fn
        self.bos_index, self.eos_index = int(bos_index), int(eos_index)
        self.min_decode_ratio, self.max_decode_ratio = float(min_decode_ratio), float(max_decode_ratio)

    @torch.no_grad()
    def __call__(self, enc_states, wav_lens) -> Tuple[List[List[int]], torch.Tensor, torch.Tensor, torch.Tensor]:
        batch, T = enc_states.shape[0], enc_states.shape[1]
        dev = enc_states.device
        enc_lens = torch.round(T * wav_lens.to(device=dev, dtype=torch.float32))
        # the truncations, in fp64: in fp32 the product 0.3 * 10 falls just below 3
        min_steps = torch.floor(self.min_decode_ratio * enc_lens.double()).long()   # per row
        max_steps = int(torch.floor(self.max_decode_ratio * enc_lens.double().max()))   # the loop bound: read once, before the loop
        state = self.init_fn(enc_states)
        tokens = torch.full((batch,), self.bos_index, dtype=torch.long, device=dev)
        finished = torch.zeros(batch, dtype=torch.bool, device=dev)
        scores = torch.zeros(batch, dtype=torch.float32, device=dev)
        lengths = torch.zeros(batch, dtype=torch.long, device=dev)
        eos = torch.full((batch,), self.eos_index, dtype=torch.long, device=dev)
        zero = torch.zeros(batch, dtype=torch.float32, device=dev)
        chosen, chosen_lp = [], []
        for t in range(max_steps):
            lp, state = self.step_fn(tokens, state)
            lp = lp.float()
            too_early = min_steps > t
            lp = lp.clone()
            lp[:, self.eos_index] = torch.where(too_early, torch.full_like(zero, float("-inf")), lp[:, self.eos_index])
            best_lp, best = lp.max(dim=-1)
            best = torch.where(finished, eos, best)
            best_lp = torch.where(finished, zero, best_lp)                        # a finished row's score is frozen
            scores = scores + best_lp
            is_eos = best == self.eos_index
            lengths = lengths + (~is_eos).long()                                  # finished rows sit on <eos>: not counted
            finished = finished | is_eos
            chosen.append(best)
            chosen_lp.append(best_lp)
            tokens = best
            if bool(finished.all()):                                              # the one host read per token
                break
        if chosen:
            tok = torch.stack(chosen, dim=1)
            log_probs = torch.stack(chosen_lp, dim=1)
        else:
            tok = torch.zeros((batch, 0), dtype=torch.long, device=dev)
            log_probs = torch.zeros((batch, 0), dtype=torch.float32, device=dev)
        tok_host, len_host = tok.cpu().tolist(), lengths.cpu().tolist()
        hyps = [row[:n] for row, n in zip(tok_host, len_host)]                    # a row's tokens before its <eos>
        return hyps, lengths, scores, log_probs
