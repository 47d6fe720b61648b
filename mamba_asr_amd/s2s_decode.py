"""Greedy S2S search on the stepped Mamba decoder: what a recipe's ``valid_search`` / ``test_search`` slot takes
(reference train_S2S.py:388-394 unpacks ``hyps, _, _, _ = searcher(enc_out, wav_lens)``; the reference fills the slot with
speechbrain's S2STransformerBeamSearcher, which re-runs ``TransformerASR.decode`` over the whole prefix for every token).

Here each token costs one ``TransformerASR.decode_step``: the decoder's state (modules/Conmamba.py DecoderState) has a
constant size, and the scan over the encoder frames is done once, by ``init_decode_state``.

Joint CTC/attention decoding (the recipes' ``ctc_weight_decode``): ``CTCPrefixScorer`` gives, for every hypothesis row, the
CTC prefix score of each possible next token from the encoder's CTC head (native kernels cm_ctc_prefix_score /
cm_ctc_prefix_advance), and the searcher adds it, weighted, to the decoder's log-probabilities.  Beam
search, LM scoring, temperature and length normalisation are not provided.
"""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, List, Optional, Tuple

import torch


@dataclass
class CTCPrefixState:
    """logp (U, T, V) fp32 and n_u (U) int32 are per utterance and shared by every state derived from one ``init``; the
    rest is per hypothesis row: row_utt (rows) int32, last (rows) int32 (-1: empty prefix), r_n / r_b (rows, T) fp32 and
    psi_g (rows) fp32 as include/conmamba_hip.h cm_ctc_prefix_args describes them."""
    logp: torch.Tensor
    n_u: torch.Tensor
    row_utt: torch.Tensor
    last: torch.Tensor
    r_n: torch.Tensor
    r_b: torch.Tensor
    psi_g: torch.Tensor


class CTCPrefixScorer:
    """CTC prefix scores on the GPU (what speechbrain's CTCScorer contributes to a search; reference hparams/S2S/*.yaml).

      state = init(logp (U, T, V) log-posteriors, enc_lens (U) frames per utterance, row_utt=None)   rows -> utterances,
                                                                                       default one row per utterance
      score(state, candidates=None) -> (rows, V) or (rows, K) fp32   log p_ctc(prefix + c, ...) - log p_ctc(prefix, ...);
                                       column <eos>: the prefix's own CTC log-likelihood over all frames; -inf: impossible
      advance(state, tokens (rows)) -> state of every row's prefix + its token (a row given <eos> keeps its state)
      reorder(state, index) -> state whose row i is the old row index[i] (row_utt included)

    No state is kept per (row, token): score recomputes the log-sum-exp over time that a stored (rows, V, T, 2) table would be
    gathered from.  States are never modified in place."""

    def __init__(self, blank_index: int, eos_index: int):
        self.blank_index, self.eos_index = int(blank_index), int(eos_index)

    def init(self, logp, enc_lens, row_utt=None) -> CTCPrefixState:
        logp = logp.detach().float().contiguous()
        U, T, _ = logp.shape
        dev = logp.device
        n_u = torch.as_tensor(enc_lens).to(device=dev, dtype=torch.float32).round().clamp(1, T).to(torch.int32).contiguous()
        if row_utt is None:
            row_utt = torch.arange(U, dtype=torch.int32, device=dev)
        row_utt = row_utt.to(device=dev, dtype=torch.int32).contiguous()
        if row_utt.numel() and bool(((row_utt < 0) | (row_utt >= U)).any()):          # the one check of the range: reorder keeps it
            raise ValueError(f"row_utt holds an utterance index outside [0, {U})")
        rows = row_utt.shape[0]
        r_b = torch.cumsum(logp[:, :, self.blank_index], dim=1)                       # once per batch
        return CTCPrefixState(logp, n_u, row_utt, torch.full((rows,), -1, dtype=torch.int32, device=dev),
                              torch.full((rows, T), float("-inf"), dtype=torch.float32, device=dev),
                              r_b.index_select(0, row_utt.long()).contiguous(), torch.zeros(rows, dtype=torch.float32, device=dev))

    def score(self, state: CTCPrefixState, candidates=None):
        from . import ops
        if candidates is not None:
            candidates = candidates.to(torch.int32).contiguous()
        return ops.ctc_prefix_score(state.logp, state.n_u, state.row_utt, state.last, state.r_n, state.r_b, state.psi_g,
                                    self.blank_index, self.eos_index, candidates=candidates, validated=True)

    def advance(self, state: CTCPrefixState, tokens) -> CTCPrefixState:
        from . import ops
        r_n, r_b, psi_g, last = ops.ctc_prefix_advance(state.logp, state.n_u, state.row_utt, state.last, state.r_n, state.r_b,
                                                       state.psi_g, tokens.to(torch.int32).contiguous(), self.blank_index,
                                                       self.eos_index, validated=True)
        return replace(state, last=last, r_n=r_n, r_b=r_b, psi_g=psi_g)

    def reorder(self, state: CTCPrefixState, index) -> CTCPrefixState:
        idx = torch.as_tensor(index, dtype=torch.long, device=state.row_utt.device)
        return replace(state, row_utt=state.row_utt[idx], last=state.last[idx], r_n=state.r_n[idx], r_b=state.r_b[idx],
                       psi_g=state.psi_g[idx])


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

    Joint CTC/attention decoding: with ``ctc_weight`` > 0 the token of a step is argmax(lp + ctc_weight * delta), lp the
    decoder's log-probabilities after the <eos> floor mask and delta the CTC prefix score of ``ctc_scorer`` (default
    CTCPrefixScorer(blank_index, eos_index); any object with its init / score / advance / reorder works) on
    ``ctc_fn(enc_states)`` -> (batch, T, vocab) CTC log-posteriors, enc_len frames per row.  The attention term has weight 1
    and the scorer is added with its weight, speechbrain's ScorerBuilder rule.  ``modules`` = [transformer, seq_lin, ctc_lin]
    gives the default ctc_fn log_softmax(ctc_lin(enc_states)).  scores and log_probs then hold the joint values.  With
    ctc_weight == 0 (the default) none of this runs.

    The loop reads one flag per token from the device (have all rows finished?); everything else stays on the device.
    """

    def __init__(self, modules=None, bos_index: int = 1, eos_index: int = 2, min_decode_ratio: float = 0.0,
                 max_decode_ratio: float = 1.0, step_fn: Optional[Callable] = None, init_fn: Optional[Callable] = None,
                 ctc_weight: float = 0.0, ctc_scorer=None, ctc_fn: Optional[Callable] = None, blank_index: int = 0):
        self.ctc_weight = float(ctc_weight)
        if not self.ctc_weight >= 0.0:
            raise ValueError(f"ctc_weight must be >= 0, got {ctc_weight}")
        if ctc_fn is None and modules is not None and len(modules) == 3:
            ctc_lin = modules[2]

            def ctc_fn(enc_states):
                return torch.log_softmax(ctc_lin(enc_states).float(), dim=-1)
        if modules is not None and len(modules) == 3:
            modules = list(modules)[:2]
        if self.ctc_weight > 0.0:
            if ctc_fn is None:
                raise ValueError("ctc_weight > 0 needs modules=[transformer, seq_lin, ctc_lin] or ctc_fn")
            if ctc_scorer is None:
                ctc_scorer = CTCPrefixScorer(blank_index, eos_index)
        self.ctc_scorer, self.ctc_fn = ctc_scorer, ctc_fn
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
        joint = self.ctc_weight > 0.0
        if joint:
            ctc_state = self.ctc_scorer.init(self.ctc_fn(enc_states), enc_lens)
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
            if joint:
                lp = lp + self.ctc_weight * self.ctc_scorer.score(ctc_state).to(lp.dtype)
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
            if joint:
                ctc_state = self.ctc_scorer.advance(ctc_state, best)              # finished rows sit on <eos>: their state stays
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
