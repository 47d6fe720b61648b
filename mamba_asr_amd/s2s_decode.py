"""Greedy and beam S2S search on the stepped decoder (Mamba or Transformer): what a recipe's ``valid_search`` / ``test_search`` slot takes
(reference train_S2S.py:388-394 unpacks ``hyps, _, _, _ = searcher(enc_out, wav_lens)``; the reference fills the slot with
speechbrain's S2STransformerBeamSearcher, which re-runs ``TransformerASR.decode`` over the whole prefix for every token).

Here each token costs one ``TransformerASR.decode_step``.  Mamba decoder: the state (modules/Conmamba.py DecoderState) has a
constant size, and the scan over the encoder frames is done once, by ``init_decode_state``.  Transformer decoder
(modules/Transformer.py TransformerDecoderState): the encoder frames are projected to keys and values once per
utterance by ``init_decode_state``, which also takes the utterances' lengths; per token cm_xattn_step attends to them and
cm_attn_step to the prefix's own cache, and a reorder moves no key or value.

Joint CTC/attention decoding (the recipes' ``ctc_weight_decode``): ``CTCPrefixScorer`` gives, for every hypothesis row, the
CTC prefix score of each possible next token from the encoder's CTC head (native kernels cm_ctc_prefix_score /
cm_ctc_prefix_advance), and the searcher adds it, weighted, to the decoder's log-probabilities.

``S2SBeamSearcher`` is the recipes' beam search (beam size, length normalisation, temperature, joint CTC scoring) on the same
stepped decoder: per token one native selection (cm_beam_select) keeps every utterance's best beam_size of
its beam_size x vocabulary candidates, and the decoder and CTC states are reordered by the chosen parents.
``TransformerLMScorer`` adds the recipes' language model (modules/TransformerLM.py on cm_attn_step) as a second
full scorer.  ScorerBuilder objects, the eos threshold and the coverage penalty are not provided.
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


class TransformerLMScorer:
    """The recipes' LM scorer (speechbrain's TransformerLMScorer; reference hparams/S2S/*.yaml: lm_weight 0.60, temperature
    1.15) on the stepped language model of modules/TransformerLM.py.

      state = init(R, device, max_steps)      the LM's caches for R hypothesis rows
      score(tokens (R,), state) -> (log_softmax(logits / temperature) (R, V) fp32, state)   consumes one token per row
      reorder(state, rows) -> state whose row i continues the old row rows[i] (no K or V is moved)"""

    def __init__(self, language_model, temperature: float = 1.0):
        self.lm, self.temperature = language_model, float(temperature)
        if not self.temperature > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")

    def init(self, R, device, max_steps):
        have, want = next(self.lm.parameters()).device, torch.device(device)
        if want.type == "cuda" and want.index is None:              # "cuda" names the current card
            want = torch.device("cuda", torch.cuda.current_device())
        if have != want:
            raise ValueError(f"TransformerLMScorer: the language model is on {have}, not on {want}")
        return self.lm.init_state(int(R), int(max_steps))

    def score(self, tokens, state):
        logits = self.lm.step(tokens, state).float()
        if self.temperature != 1.0:
            logits = logits / self.temperature
        return torch.log_softmax(logits, dim=-1), state

    def reorder(self, state, rows):
        return state.reorder(rows)


def _default_step(transformer, seq_lin, temperature=1.0):
    """The searchers' default per-token function: log_softmax(seq_lin(transformer.decode_step(tokens, state)) / temperature)."""
    def step(tokens, state):
        logits = seq_lin(transformer.decode_step(tokens, state))[:, 0].float()    # decode_step: (batch, 1, d_model)
        if temperature != 1.0:
            logits = logits / temperature
        return torch.log_softmax(logits, dim=-1), state
    return step


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
    log_softmax(seq_lin(transformer.decode_step(tokens, state))) on the state of transformer.init_decode_state (called with
    enc_len as well where the transformer's decoder is the Transformer one, which masks the frames beyond it).  Both are
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

    temperature = 1.0                                                            # of the default step; S2SBeamSearcher sets its own

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
                raise ValueError(f"{type(self).__name__} needs modules=[transformer, seq_lin] (or step_fn and init_fn)")
            transformer, seq_lin = modules

            if init_fn is None and getattr(transformer, "decoder_module", "mamba") == "transformer":
                self._init_takes_lens = True                                      # the memory frames beyond enc_len are masked

            def default_init(enc_states, enc_lens=None):
                if enc_lens is None:
                    return transformer.init_decode_state(enc_states)
                return transformer.init_decode_state(enc_states, enc_lens)

            default_step = _default_step(transformer, seq_lin, self.temperature)

            init_fn, step_fn = init_fn or default_init, step_fn or default_step
        self.init_fn, self.step_fn = init_fn, step_fn
        self._init_takes_lens = getattr(self, "_init_takes_lens", False)
        self.bos_index, self.eos_index = int(bos_index), int(eos_index)
        self.min_decode_ratio, self.max_decode_ratio = float(min_decode_ratio), float(max_decode_ratio)

    def _init_state(self, enc_states, enc_lens):
        """A user's ``init_fn(enc_states)`` keeps its one-argument call; the default one of a Transformer decoder gets enc_lens."""
        return self.init_fn(enc_states, enc_lens) if self._init_takes_lens else self.init_fn(enc_states)

    @torch.no_grad()
    def __call__(self, enc_states, wav_lens) -> Tuple[List[List[int]], torch.Tensor, torch.Tensor, torch.Tensor]:
        batch, T = enc_states.shape[0], enc_states.shape[1]
        dev = enc_states.device
        enc_lens = torch.round(T * wav_lens.to(device=dev, dtype=torch.float32))
        # the truncations, in fp64: in fp32 the product 0.3 * 10 falls just below 3
        min_steps = torch.floor(self.min_decode_ratio * enc_lens.double()).long()   # per row
        max_steps = int(torch.floor(self.max_decode_ratio * enc_lens.double().max()))   # the loop bound: read once, before the loop
        state = self._init_state(enc_states, enc_lens)
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


def select_torch(att, alive, B, eos, delta=None, weight=0.0, eos_blocked=None):
    """ops.beam_select restated in torch (the CM_BEAM_SELECT=0 route; any device): the same three fp32 operations, then
    torch.topk over each utterance's B * V joint scores.  Among EQUAL scores topk's order is not the native kernel's (lowest
    flat index first); for a searcher that only matters among the -inf candidates that fill dead slots."""
    rows, V = att.shape
    U = rows // B
    a = att
    if eos_blocked is not None and 0 <= eos < V:
        a = att.clone()
        blocked = eos_blocked.bool().repeat_interleave(B)
        a[:, eos] = torch.where(blocked, torch.full_like(alive, float("-inf")), a[:, eos])
    inc = a if delta is None else a + weight * delta
    s = alive.unsqueeze(1) + inc
    s = torch.where(torch.isnan(s), torch.full_like(s, float("-inf")), s)
    score, flat = torch.topk(s.view(U, B * V), B, dim=1)
    parent = torch.div(flat, V, rounding_mode="floor")
    token = flat - parent * V
    inc_sel = inc.reshape(U, B * V).gather(1, flat)
    return score, inc_sel, parent.to(torch.int32), token.to(torch.int32)


class S2SBeamSearcher(S2SGreedySearcher):
    """Beam search in the call shape of S2SGreedySearcher: ``searcher(enc_states, wav_lens) -> (hyps, lengths, scores,
    log_probs)``, the slot the reference recipes fill with speechbrain's S2STransformerBeamSearcher (hparams/S2S/*.yaml:
    valid_beam_size 10, test_beam_size 66, length_normalization True, temperature 1.15, ctc_weight_decode 0.40).

    modules / step_fn / init_fn / ctc_weight / ctc_scorer / ctc_fn / blank_index / bos_index / eos_index / min_decode_ratio /
    max_decode_ratio are the greedy searcher's.  The state ``init_fn`` returns and the CTC scorer's state must have
    ``reorder`` (DecoderState and CTCPrefixScorer do).  Added:
      beam_size             1 .. 128 hypotheses per utterance; hypothesis rows are u * beam_size + slot
      length_normalization  rank finished hypotheses by score / (number of summed increments) instead of the raw sum
      temperature           the default step is log_softmax(seq_lin(out) / temperature)
      topk                  hypotheses returned per utterance
      select_fn             the per-token selection, ``ops.beam_select``'s signature and contract; default ops.beam_select
                            (cm_beam_select), or ``select_torch`` with CM_BEAM_SELECT=0 in the environment
      lm_scorer, lm_weight  a language model as a second full scorer: any object with TransformerLMScorer's init / score /
                            reorder; lm_weight > 0 is required with it.  Per token ``lm_scorer.score(tokens, state)`` is called
                            once with the tokens just chosen, and lm_weight * its log-probabilities joins the increment: as the
                            selection's delta (LM alone), or as ctc_weight * delta_ctc + lm_weight * lm_lp formed in torch
                            (fp32, two separately rounded products) and passed with weight 1.0
    No ScorerBuilder object, eos threshold or coverage penalty: asking for one raises NotImplementedError, as does an lm_weight
    without an lm_scorer.

    Per token: step every row, add the weighted CTC prefix scores, and keep per utterance the beam_size best of its
    beam_size x vocab candidates (<eos> masked below the utterance's min_decode_ratio floor; <eos> candidates compete for
    the slots like any other).  A slot that took <eos> is a finished hypothesis; it and the slots filled with -inf candidates
    are dead from then on (they step on <eos>, as the greedy searcher's finished rows do).  An utterance's search is over once
    it has beam_size finished hypotheses or no live slot, whatever the rest of the batch does; the loop ends when that holds
    for all, or after floor(max_decode_ratio * max(enc_len)) steps.  That cap is the batch's (as in the greedy searcher), so an
    utterance decoded alone equals the same utterance in a batch only where its search ends below its own cap.  Slots still alive when their utterance's search ends are
    closed as they are (no <eos> term).  Per utterance the hypotheses are ranked by final score,
    then earlier completion, then lower slot.  One flag is read from the device per token; the records of all steps come to
    the host at the end (one fp32 and one int32 copy).

    topk == 1: hyps / lengths (U,) / scores (U,) / log_probs (U, steps) as the greedy searcher's, scores the final (raw or
    normalised) scores, log_probs the increments along the best path and 0 behind it.  topk > 1: hyps[u] is a list of up to
    topk token lists, lengths / scores are (U, topk) padded with 0 / -inf; log_probs belongs to the best hypothesis."""

    def __init__(self, modules=None, beam_size: int = 10, length_normalization: bool = True, temperature: float = 1.0,
                 topk: int = 1, select_fn: Optional[Callable] = None, using_eos_threshold: bool = False, scorer=None,
                 lm_weight: float = 0.0, lm_modules=None, lm_scorer=None, **greedy_args):
        if using_eos_threshold:
            raise NotImplementedError("S2SBeamSearcher: the eos threshold (using_eos_threshold) is not provided")
        if scorer is not None:
            raise NotImplementedError("S2SBeamSearcher: a scorer= object (ScorerBuilder) is not provided; joint CTC decoding "
                                      "is ctc_weight=")
        if lm_modules is not None or (lm_scorer is None and lm_weight):
            raise NotImplementedError("S2SBeamSearcher: LM scoring without an lm_scorer (lm_weight alone / lm_modules) is not "
                                      "provided; give lm_scorer=TransformerLMScorer(language_model) and lm_weight")
        self.lm_scorer, self.lm_weight = lm_scorer, float(lm_weight or 0.0)
        if lm_scorer is not None and not self.lm_weight > 0.0:
            raise ValueError(f"lm_scorer needs lm_weight > 0, got {lm_weight}")
        self.beam_size, self.topk = int(beam_size), int(topk)
        if not 1 <= self.beam_size <= 128:
            raise ValueError(f"beam_size must be in [1, 128], got {beam_size}")
        if self.topk < 1:
            raise ValueError(f"topk must be >= 1, got {topk}")
        self.temperature = float(temperature)
        if not self.temperature > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature}")
        self.length_normalization = bool(length_normalization)
        super().__init__(modules=modules, **greedy_args)
        if select_fn is None:
            import os
            if os.environ.get("CM_BEAM_SELECT", "1") == "0":
                select_fn = select_torch
            else:
                from . import ops
                select_fn = ops.beam_select
        self.select_fn = select_fn

    @torch.no_grad()
    def __call__(self, enc_states, wav_lens):
        U, T = enc_states.shape[0], enc_states.shape[1]
        B, eos_index = self.beam_size, self.eos_index
        dev = enc_states.device
        enc_lens = torch.round(T * wav_lens.to(device=dev, dtype=torch.float32))
        min_steps = torch.floor(self.min_decode_ratio * enc_lens.double()).long()
        max_steps = int(torch.floor(self.max_decode_ratio * enc_lens.double().max()))
        idx = torch.arange(U, device=dev).repeat_interleave(B)
        state = self._init_state(enc_states, enc_lens).reorder(idx)                          # the prefill runs once per utterance
        joint = self.ctc_weight > 0.0
        if joint:
            ctc_state = self.ctc_scorer.init(self.ctc_fn(enc_states), enc_lens, row_utt=idx)
        lm = self.lm_scorer is not None
        if lm:
            lm_state = self.lm_scorer.init(U * B, dev, max_steps)
        neg_inf = torch.full((U, B), float("-inf"), dtype=torch.float32, device=dev)
        alive = neg_inf.clone()
        alive[:, 0] = 0.0
        tokens = torch.full((U * B,), self.bos_index, dtype=torch.long, device=dev)
        eos = torch.full((U, B), eos_index, dtype=torch.long, device=dev)
        row0 = (torch.arange(U, device=dev) * B).unsqueeze(1)
        n_fin = torch.zeros(U, dtype=torch.long, device=dev)
        records, choices = [], []                                                # per step (score, inc) fp32 and (parent, token) int32
        for t in range(max_steps):
            lp, state = self.step_fn(tokens, state)
            lp = lp.float().contiguous()
            delta = self.ctc_scorer.score(ctc_state).float().contiguous() if joint else None
            weight = self.ctc_weight if joint else 0.0
            if lm:
                lm_lp, lm_state = self.lm_scorer.score(tokens, lm_state)
                lm_lp = lm_lp.float().contiguous()
                if joint:                                                        # two separately rounded products, then one add;
                    delta, weight = self.ctc_weight * delta + self.lm_weight * lm_lp, 1.0   # the selection's multiply by 1.0 is exact
                else:
                    delta, weight = lm_lp, self.lm_weight
            score, inc, parent, token = self.select_fn(lp, alive.reshape(-1).contiguous(), B, eos_index, delta=delta,
                                                       weight=weight,
                                                       eos_blocked=(min_steps > t).to(torch.int32))
            parent, token = parent.int(), token.int()
            finite = torch.isfinite(score)
            is_eos = token == eos_index
            n_fin = n_fin + (is_eos & finite).sum(dim=1)
            alive = torch.where(is_eos | ~finite, neg_inf, score)
            tokens = torch.where(finite, token.long(), eos).reshape(-1)          # a dead slot steps on <eos>, never on blank
            rows = (row0 + parent.long()).reshape(-1)
            state = state.reorder(rows)
            if joint:
                ctc_state = self.ctc_scorer.advance(self.ctc_scorer.reorder(ctc_state, rows), tokens)
            if lm:
                lm_state = self.lm_scorer.reorder(lm_state, rows)
            records.append(torch.stack([score, inc]))
            choices.append(torch.stack([parent, token]))
            full = n_fin >= B
            if bool((full | ~torch.isfinite(alive).any(dim=1)).all()):           # the one host read per token
                break
            # an utterance with beam_size finished hypotheses is over, whatever the rest of the batch still does: its live slots
            # (recorded above) are closed as they are and extend no further
            alive = torch.where(full.unsqueeze(1), neg_inf, alive)
        return self._finish(records, choices, U, dev)

    def _finish(self, records, choices, U, dev):
        """Ranking and backtrace on the host, from one copy each of the stacked (steps, 2, U, B) fp32 and int32 records."""
        B, steps = self.beam_size, len(records)
        if steps == 0:                                                           # a cap of zero steps: the empty hypothesis, score 0
            hyps = [[] for _ in range(U)] if self.topk == 1 else [[[]] for _ in range(U)]
            shape = (U,) if self.topk == 1 else (U, self.topk)
            lengths = torch.zeros(shape, dtype=torch.long, device=dev)
            scores = torch.zeros(shape, dtype=torch.float32, device=dev)
            if self.topk > 1:
                scores[:, 1:] = float("-inf")
            return hyps, lengths, scores, torch.zeros((U, 0), dtype=torch.float32, device=dev)
        rec, cho = torch.stack(records).cpu(), torch.stack(choices).cpu()
        score, inc, parent, token = rec[:, 0], rec[:, 1], cho[:, 0], cho[:, 1]   # (steps, U, B)
        finite = torch.isfinite(score)
        fin = finite & (token == self.eos_index)                                 # finished at step t: t tokens and the <eos>
        reached = fin.sum(dim=2).cumsum(dim=0) >= B                              # (steps, U): the utterance's search is over
        last = torch.where(reached.any(dim=0), reached.long().argmax(dim=0), torch.full((U,), steps - 1))
        open_ = torch.zeros_like(fin)
        for u in range(U):                                                       # alive when the utterance's search ended: closed as it is
            open_[last[u], u] = finite[last[u], u] & ~fin[last[u], u]
        n_inc = torch.arange(1, steps + 1, dtype=torch.float32).view(-1, 1, 1).expand_as(score)
        final = score / n_inc if self.length_normalization else score            # fp32; open slots: `steps` tokens, no <eos>
        done_step = torch.arange(steps).view(-1, 1, 1).expand_as(score) + open_.long()   # open slots complete after the last step
        score_l, inc_l, parent_l, token_l = score.tolist(), inc.tolist(), parent.tolist(), token.tolist()
        hyps_all, len_all, score_all = [], [], []
        log_probs = torch.zeros((U, steps), dtype=torch.float32)
        for u in range(U):
            cand = (fin[:, u] | open_[:, u]).nonzero().tolist()                  # (step, slot) pairs
            cand.sort(key=lambda ts: (-float(final[ts[0], u, ts[1]]), int(done_step[ts[0], u, ts[1]]), ts[1]))
            hyps_u, scores_u = [], []
            for rank, (t, j) in enumerate(cand[:self.topk]):
                toks, incs, slot = [], [], j
                for s in range(t, -1, -1):
                    toks.append(token_l[s][u][slot])
                    incs.append(inc_l[s][u][slot])
                    slot = parent_l[s][u][slot]
                toks.reverse()
                incs.reverse()
                if bool(fin[t, u, j]):
                    toks.pop()                                                   # the closing <eos>
                hyps_u.append(toks)
                scores_u.append(float(final[t, u, j]))
                if rank == 0:
                    log_probs[u, :len(incs)] = torch.tensor(incs, dtype=torch.float32)
            hyps_all.append(hyps_u)
            score_all.append(scores_u)
            len_all.append([len(h) for h in hyps_u])
        if self.topk == 1:
            hyps = [h[0] if h else [] for h in hyps_all]
            lengths = torch.tensor([n[0] if n else 0 for n in len_all], dtype=torch.long)
            scores = torch.tensor([s[0] if s else float("-inf") for s in score_all], dtype=torch.float32)
        else:
            hyps = hyps_all
            lengths = torch.zeros((U, self.topk), dtype=torch.long)
            scores = torch.full((U, self.topk), float("-inf"), dtype=torch.float32)
            for u in range(U):
                n = len(len_all[u])
                lengths[u, :n] = torch.tensor(len_all[u], dtype=torch.long)
                scores[u, :n] = torch.tensor(score_all[u], dtype=torch.float32)
        return hyps, lengths.to(dev), scores.to(dev), log_probs.to(dev)
