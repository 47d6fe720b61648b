"""CTC beam search on the GPU, LM-free or with a fused n-gram LM: the drop-in for speechbrain.decoders.ctc.CTCBeamSearcher in the CTC recipe's TEST stage
(reference train_CTC.py:1155-1161 builds it from hparams/CTC/conmamba_large.yaml:232-237; compute_forward calls it at :309-310;
compute_objectives reads hyp[0].text at :411-414).  The search itself is the HIP kernel behind ops.ctc_beam_search
(csrc/ctc_beam.hip); this module classifies the vocabulary once, maps relative lengths to frame counts and composes texts.

The contract (speechbrain's searcher without an LM, itself a port of pyctcdecode, as restated here; parity with speechbrain is
not pinned because speechbrain is not installable):

State.  A beam is (text, partial, last, score): completed words joined by single spaces, the word being built, the last token
index (initially none) and a float64 log score (initially 0).  Start with one beam ("", "", none, 0).

Token classes.  blank = blank_index.  If any piece starts with spm_token the vocabulary is SentencePiece and every piece that
starts with it is word-start with clean part piece[1:]; otherwise the piece equal to space_token is word-start with an empty
clean part.  Every other piece is a char whose clean part is the whole piece (any length, e.g. "<unk>").

Per frame t < n_b.  Skip the frame if logp[blank] > log(blank_skip_threshold) (never under the default 1.0).  Otherwise:
  1. select {v : logp[v] > token_prune_min_logp} plus the first argmax, in ascending index order;
  2. for each selected token (outer) and each beam in rank order (inner) make a candidate with score + logp[v] and last = v:
     blank or v == last leave text and partial unchanged; word-start: text = join(text, partial), partial = clean(v);
     char: partial += clean(v);  join(a, b) = a if b == "" else b if a == "" else a + " " + b;
  3. merge candidates with equal (text, partial, last): the survivor sits at the earliest candidate's position and its score
     is a left fold of logaddexp in candidate order, logaddexp(a, b) = max + log1p(exp(-|a - b|)) (-inf when both are -inf);
  4. drop beams below max + beam_prune_logp;  5. rank by score descending, ties by earliest candidate, keep beam_size;
  6. if prune_history, keep only the first beam per (last word of text, partial, last).
Finish: text = join(text, partial), partial = ""; merge by text (same fold); prune by beam_prune_logp; rank; the first topk are
returned as CTCHypothesis(text, None, score, score, None).

Choices recorded where speechbrain could not be checked: n_b = round(wav_lens[b] * T) (dataio.ctc_greedy_decode's rule;
speechbrain may truncate); the exact blank-skip comparison; the loop order over selected tokens (speechbrain iterates a Python
set: only ties and rounding can differ).  n_b = 0 gives the single hypothesis "" with score 0.  NaN in a decoded frame raises
ValueError naming the utterance.

Streaming.  StreamingCTCBeamSearcher carries the same search across chunks (ops.ctc_beam_stream, csrc/ctc_beam_stream.hip): the
beams and the backtracking history live in a device slab per stream, a step is one launch that reads nothing back, and
hypotheses() after n frames is by definition what the search above returns for n_b = n -- the kernels share the frame body, so the
score bits agree as well.

N-gram LM fusion (kenlm_model_path; ops.ctc_beam_search_lm, csrc/ctc_beam_lm.hip, tables by ngram_lm.NgramLM).
kenlm, pyctcdecode and speechbrain cannot be installed here, so parity with them is not pinned: these rules are the contract.

Model.  A backoff n-gram LM in ARPA text format, plain or .gz, of order 1 to 5; log10 probabilities and backoffs are stored as
fp32, a missing backoff column means 0; <s>, </s> and <unk> are optional.  A kenlm binary file or a malformed ARPA file raises
ValueError naming the path and the line.  (Choices: an n-gram whose context is not listed as an (n-1)-gram, a duplicate n-gram,
a count that differs from the header and a non-finite number are malformed.)

Conditional probability.  log10 p(w | c) is plain ARPA backoff over the last order-1 words of c: the longest stored n-gram gives
the probability, every context that had to be dropped contributes its backoff if it is stored.  (Choice: the fp32 values are
summed in float64, probability first, then the backoffs from the shortest dropped context to the longest.)

Word score.  A completed word w after the beam's completed words c (preceded by <s> when score_boundary is set and the LM lists
<s>): lw = log10 p(w|c) when w is in the LM vocabulary (the 1-grams); otherwise lw = log10 p(<unk>|c) + unk_score_offset, the
p(<unk>|c) term being 0 when the LM lists no <unk>, and the context continues with <unk> (no <unk>: the context is emptied, <s>
included).  word_score = alpha * ln(10) * lw + beta.  LM(text) is the float64 sum of word_score over the words of text, in order.

Partial-word score.  partial_score(p) = 0 if p is empty or a prefix of, or equal to, some word of the unigram list (unigrams=
when given, else the ARPA 1-grams minus the three specials); otherwise alpha * ln(10) * unk_score_offset * max(1, len(p) / 6),
len in code points.

Per frame.  Steps 1 to 3 above are unchanged and act on the acoustic score alone (equal keys have equal LM state by
construction, so the merge folds acoustic scores).  Then every merged candidate gets total = acoustic + LM(text) +
partial_score(partial); steps 4 and 5 act on total, ties to the earliest candidate; step 6 is unchanged.

Finish.  Commit the partial as a word, scored as above; merge by text, folding the acoustic score; total = acoustic + LM(text),
plus alpha * ln(10) * log10 p(</s> | text) when score_boundary is set and the LM lists </s> (no beta for it); prune and rank by
total; return CTCHypothesis(text, None, score=acoustic, lm_score=total, None).  n_b = 0 or T = 0 gives one hypothesis with
text "", score 0.0 and lm_score = LM("") by the same rules (the </s> term alone).  Without kenlm_model_path the LM keywords are
inert.  StreamingCTCBeamLMSearcher carries this search across chunks (ops.ctc_beam_lm_stream, csrc/ctc_beam_lm_stream.hip;
DESIGN.md §4q): every beam's LM state lives in the stream's slab beside its identity, and hypotheses() after n frames is what the
search above returns for n_b = n, lm_score bits included.  StreamingCTCBeamSearcher itself stays LM-free and refuses a path.

Forced alignment (CTCAligner, CTCBeamSearcher.search(..., text_frames=True); ops.ctc_align, csrc/ctc_align.hip): the
best path of a KNOWN label sequence through the CTC trellis, pinned bit for bit by tests/ctc_align_ref.py.  Per utterance
n = min(input_lengths[b], T), L = min(target_lengths[b], S); the extended sequence e has E = 2 L + 1 entries, e[2j] = blank,
e[2j+1] = y_j; x_t(s) = (double) lp[row, t, e[s]] (fp32 or bf16 in, the conversion is exact; a label outside [0, V) has x = -inf).
  D_0(s) = x_0(s) for s in {0, 1} with s < E, else -inf.  For t >= 1 the candidates are c0 = D_{t-1}(s); c1 = D_{t-1}(s-1) when
  s >= 1; c2 = D_{t-1}(s-2) when s is odd, s >= 3 and e[s] != e[s-2].  best = c0, move 0; if c1 > best: best = c1, move 1; if
  c2 > best: best = c2, move 2 (strict: ties keep the smaller move).  D_t(s) = best + x_t(s) in float64.
  End: sE = E-1; if E >= 2 and D_{n-1}(E-2) > D_{n-1}(E-1), sE = E-2.  score = D_{n-1}(sE); s_{n-1} = sE and
  s_{t-1} = s_t - move_t(s_t).
Every operation is a float64 add or compare, so the kernel's bits are the reference's by construction, ties included.
status 0: aligned.  1: no alignment (score == -inf, or n == 0 with L > 0; a row index outside log_probs as well).  2: some x_t(s)
with t < n, s < E is NaN (tracked by a flag, not through max; also a NaN score, which +inf inputs can make); NaN anywhere else in
log_probs has no effect.  n == 0 and L == 0: status 0, score 0.0, an empty path.
Outputs: score (B) fp64 (-inf under status 1, NaN under 2); status (B) int32; states (B, T) int32 = s_t for t < n, -1 elsewhere,
all -1 when status != 0; starts / ends (B, S) int32 = label j's first frame and one past its last frame in state 2j+1, -1 for
j >= L or status != 0; label_logp (B, S) fp64 = the left fold, in increasing t, of x_t(2j+1) over the label's frames, 0.0 where
starts is -1.  At most 1023 labels per utterance.
Words.  A word is the tokens between word-starts, by the rules of compose(): its span runs from its first token's start to its
last token's end, its log-probability is the sum of its tokens'; a piece whose clean part is empty (the bare space piece, a bare
spm_token) and blank belong to no word.  CTCBeamSearcher.search(text_frames=True) aligns each returned hypothesis' own tokens in one
extra launch: those are the Viterbi frames of the hypothesis, not the frames at which the beam emitted its tokens.

Greedy decoding (CTCGreedyDecoder; ops.ctc_greedy, csrc/ctc_greedy.hip), pinned bit for bit by
tests/ctc_score_ref.py: per frame the lowest index attaining the maximum (-inf an ordinary value), a frame kept when that index is
not blank and differs from the previous frame's, each kept token with its run's frames and the float64 left fold of its own
log-probabilities; a NaN in a frame below the length gives status 2.  The class docstring has the whole contract.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import torch

from . import ops

P61 = (1 << 61) - 1
HASH_BASE = (0x1D2C3B4A59687F11 % P61, 0x0F1E2D3C4B5A6979 % P61)   # two fixed bases of the polynomial hashes mod 2^61 - 1
HASH_SEP = 0x110001                                                 # word separator: above every code point + 1
BLANK, CHAR, WORD_START = -1, 0, 1


@dataclass
class CTCHypothesis:
    """One decoded hypothesis, with the fields of speechbrain.decoders.ctc.CTCHypothesis."""
    text: str
    last_lm_state: None = None
    score: float = 0.0
    lm_score: float = 0.0
    text_frames: Optional[list] = None
    tokens: Optional[list] = None            # CTCGreedyDecoder fills it; the beam searchers leave it None


def piece_hash(s: str):
    """(H_k(s), base_k^len(s)) mod 2^61 - 1 for both bases, H_k(s) = sum_i (ord(s_i) + 1) base_k^(n-1-i)."""
    out_h, out_p = [], []
    for base in HASH_BASE:
        h, pw = 0, 1
        for ch in s:
            h = (h * base + ord(ch) + 1) % P61
            pw = pw * base % P61
        out_h.append(h)
        out_p.append(pw)
    return out_h, out_p


def _join(a: str, b: str) -> str:
    return a if not b else (b if not a else a + " " + b)


def classify_vocab(vocab: Sequence[str], blank_index: int, space_token: str, spm_token: str):
    """The token classes of the module docstring -> (is_spm, classes, clean parts), one entry per piece."""
    is_spm = any(p.startswith(spm_token) for p in vocab)
    classes, cleans = [], []
    for v, p in enumerate(vocab):
        if v == blank_index:
            cls, clean = BLANK, ""
        elif is_spm and p.startswith(spm_token):
            cls, clean = WORD_START, p[len(spm_token):]
        elif not is_spm and p == space_token:
            cls, clean = WORD_START, ""
        else:
            cls, clean = CHAR, p
        classes.append(cls)
        cleans.append(clean)
    return is_spm, classes, cleans


def group_words(tokens, starts, ends, logp, classes, clean):
    """Aligned tokens -> (words, word_frames [(start, end)], word_logp), all host lists: ``tokens`` the label ids, ``starts`` /
    ``ends`` / ``logp`` their frames and log-probabilities, ``classes`` / ``clean`` the vocabulary's (classify_vocab).  The words
    are those of compose(tokens), in order; a token with an empty clean part and blank belong to no word."""
    words, frames, lps = [], [], []
    cur = None                                   # [text, start, end, logp] of the word being built

    def commit():
        if cur is not None and cur[0]:
            words.append(cur[0])
            frames.append((cur[1], cur[2]))
            lps.append(cur[3])
    for v, a, z, lp in zip(tokens, starts, ends, logp):
        if classes[v] == BLANK:
            continue
        if classes[v] == WORD_START:
            commit()
            cur = None
        if not clean[v]:
            continue
        if cur is None:
            cur = [clean[v], int(a), int(z), float(lp)]
        else:
            cur[0], cur[2], cur[3] = cur[0] + clean[v], int(z), cur[3] + float(lp)
    commit()
    return words, frames, lps


def _frame_counts(steps: int, wav_lens: Optional[torch.Tensor], batch: int) -> List[int]:
    if wav_lens is None:
        return [steps] * batch
    return [min(max(int(round(rel * steps)), 0), steps) for rel in wav_lens.detach().cpu().tolist()]


class CTCBeamSearcher:
    """CTC beam search without a language model, on the GPU (constructor keywords of speechbrain's CTCBeamSearcher).

    __call__(log_probs (batch, T, V) on the GPU, wav_lens (batch) relative lengths or None, lengths=None: absolute frame counts,
    which win when given) -> List[List[CTCHypothesis]]
    with at most topk hypotheses per utterance, best first.  There is no host implementation: CPU tensors raise."""

    def __init__(self, blank_index: int, vocab_list: Sequence[str], space_token: str = " ", spm_token: str = "▁",
                 kenlm_model_path: Optional[str] = None, unigrams: Optional[List[str]] = None, alpha: float = 0.5,
                 beta: float = 1.5, unk_score_offset: float = -10.0, score_boundary: bool = True, beam_size: int = 100,
                 beam_prune_logp: float = -10.0, token_prune_min_logp: float = -5.0, prune_history: bool = True,
                 blank_skip_threshold: float = 1.0, topk: int = 1):
        vocab = list(vocab_list)
        if len(set(vocab)) != len(vocab):
            dup = sorted({p for p in vocab if vocab.count(p) > 1})
            raise ValueError(f"CTCBeamSearcher: duplicate pieces in vocab_list: {dup}")
        if not 0 <= blank_index < len(vocab):
            raise ValueError(f"CTCBeamSearcher: blank_index {blank_index} outside a vocabulary of {len(vocab)}")
        if not 1 <= beam_size <= 256:
            raise ValueError(f"CTCBeamSearcher: beam_size {beam_size} not in [1, 256]")
        if topk < 1:
            raise ValueError(f"CTCBeamSearcher: topk {topk} < 1")
        if not blank_skip_threshold > 0:
            raise ValueError("CTCBeamSearcher: blank_skip_threshold must be > 0")
        self.blank_index, self.vocab_list = int(blank_index), vocab
        self.space_token, self.spm_token = space_token, spm_token
        self.beam_size, self.topk, self.prune_history = int(beam_size), int(topk), bool(prune_history)
        self.beam_prune_logp, self.token_prune_min_logp = float(beam_prune_logp), float(token_prune_min_logp)
        self.blank_skip_threshold = float(blank_skip_threshold)
        self.is_spm, self.classes, self.clean = classify_vocab(vocab, self.blank_index, space_token, spm_token)
        hashes = [piece_hash(c) for c in self.clean]
        self.tok_class = torch.tensor([1 if c == WORD_START else 0 for c in self.classes], dtype=torch.int32)
        self.tok_hash = torch.tensor([h for h, _ in hashes], dtype=torch.int64)
        self.tok_pow = torch.tensor([p for _, p in hashes], dtype=torch.int64)
        self.tok_len = torch.tensor([len(c) for c in self.clean], dtype=torch.int32)
        self._dev_tables = {}
        self.lm = None
        if kenlm_model_path is not None:
            from .ngram_lm import NgramLM
            if WORD_START not in self.classes:
                raise NotImplementedError("CTCBeamSearcher: language-model fusion (kenlm_model_path) needs a vocabulary with a "
                                          "word-start piece (a piece starting with spm_token, or space_token): without one no word "
                                          "ever completes and a word-level n-gram LM has nothing to score")
            for name, x in (("alpha", alpha), ("beta", beta), ("unk_score_offset", unk_score_offset)):
                if not math.isfinite(float(x)):
                    raise ValueError(f"CTCBeamSearcher: {name} must be finite, got {x}")
            self.lm = NgramLM.from_arpa(kenlm_model_path, unigrams=unigrams)
            self.alpha, self.beta, self.unk_score_offset = float(alpha), float(beta), float(unk_score_offset)
            self.score_boundary = bool(score_boundary)

    def compose(self, tokens: Sequence[int]) -> str:
        """Text of a sequence of text-changing tokens, by the class rules."""
        text, partial = "", ""
        for v in tokens:
            if self.classes[v] == WORD_START:
                text, partial = _join(text, partial), self.clean[v]
            elif self.classes[v] == CHAR:
                partial += self.clean[v]
        return _join(text, partial)

    def _tables(self, device):
        key = str(device)
        if key not in self._dev_tables:
            self._dev_tables[key] = tuple(t.to(device) for t in (self.tok_class, self.tok_hash, self.tok_pow))
        return self._dev_tables[key]

    def _tok_len(self, device):
        key = (str(device), "tok_len")
        if key not in self._dev_tables:
            self._dev_tables[key] = self.tok_len.to(device)
        return self._dev_tables[key]

    def frame_counts(self, steps: int, wav_lens: Optional[torch.Tensor], batch: int) -> List[int]:
        return _frame_counts(steps, wav_lens, batch)

    def __call__(self, log_probs: torch.Tensor, wav_lens: Optional[torch.Tensor] = None, lengths=None) -> List[List[CTCHypothesis]]:
        """``lengths``: absolute frame counts per utterance (a host sequence of ints, e.g. the fused.RowLens of
        ConMambaASR.encode(..., ragged=True)); it wins over ``wav_lens``, whose round(rel * T) can miss an utterance's own row count
        by one.  text_frames stays None: search(..., text_frames=True) is the call that fills it."""
        return self.search(log_probs, wav_lens, lengths)

    def search(self, log_probs: torch.Tensor, wav_lens: Optional[torch.Tensor] = None, lengths=None,
               text_frames: bool = False) -> List[List[CTCHypothesis]]:
        """__call__ with one more keyword (speechbrain's call signature is left as it is).  ``text_frames=True``: every returned
        hypothesis gets text_frames = [(start_frame, end_frame), ...], one span per word of its text, from ONE extra cm_ctc_align
        launch over all returned hypotheses' tokens (the topk hypotheses of an utterance share its frames through ``rows``).  These
        are the Viterbi frames of the hypothesis' tokens, not the frames at which the beam emitted them.  A hypothesis of more
        than 1023 tokens raises ValueError.  The default leaves text_frames None.  Whole-utterance searches only: the streaming
        searchers do not take it."""
        if not log_probs.is_cuda:
            raise RuntimeError("CTCBeamSearcher runs on the GPU only (got a CPU tensor): move log_probs to the GPU")
        if log_probs.dim() != 3 or log_probs.shape[2] != len(self.vocab_list):
            raise ValueError(f"CTCBeamSearcher: log_probs must be (batch, T, {len(self.vocab_list)}), got {tuple(log_probs.shape)}")
        b, steps, _ = log_probs.shape
        if lengths is None:
            counts = self.frame_counts(steps, wav_lens, b)
        else:
            counts = [int(x) for x in lengths]
            if len(counts) != b or any(not 0 <= x <= steps for x in counts):
                raise ValueError(f"CTCBeamSearcher: lengths must be {b} frame counts in [0, {steps}], got {counts}")
        if steps == 0:
            empty = 0.0 if self.lm is None else self.lm.lm_of_text("", self.alpha, self.beta, self.unk_score_offset,
                                                                   self.score_boundary, finish=True)
            return [[CTCHypothesis("", None, 0.0, empty, [] if text_frames else None)] for _ in range(b)]
        lengths = torch.tensor(counts, dtype=torch.int32).to(log_probs.device)
        tc, th, tp = self._tables(log_probs.device)
        if self.lm is not None:
            lm, tl = self.lm, self._tok_len(log_probs.device)
            tokens, token_len, scores, lm_scores, num_hyps, bad = ops.ctc_beam_search_lm(
                log_probs, lengths, tc, th, tp, tl, HASH_BASE, HASH_SEP, lm.tables(log_probs.device), order=lm.order,
                n_words=len(lm.words), lm_bos=lm.bos if self.score_boundary else -1, lm_eos=lm.eos if self.score_boundary else -1,
                lm_unk=lm.unk, alpha=self.alpha, beta=self.beta, unk_score_offset=self.unk_score_offset, blank=self.blank_index,
                beam_size=self.beam_size, topk=self.topk, prune_history=self.prune_history, beam_prune_logp=self.beam_prune_logp,
                token_prune_min_logp=self.token_prune_min_logp, blank_skip_threshold=self.blank_skip_threshold)
            out = self._hypotheses(tokens, token_len, scores, num_hyps, bad, range(b), "utterance", lm_scores=lm_scores)
            return self._text_frames(out, log_probs, lengths, tokens, token_len) if text_frames else out
        tokens, token_len, scores, num_hyps, bad = ops.ctc_beam_search(
            log_probs, lengths, tc, th, tp, HASH_BASE, HASH_SEP, blank=self.blank_index, beam_size=self.beam_size,
            topk=self.topk, prune_history=self.prune_history, beam_prune_logp=self.beam_prune_logp,
            token_prune_min_logp=self.token_prune_min_logp, blank_skip_threshold=self.blank_skip_threshold)
        out = self._hypotheses(tokens, token_len, scores, num_hyps, bad, range(b), "utterance")
        return self._text_frames(out, log_probs, lengths, tokens, token_len) if text_frames else out

    def _text_frames(self, hyps, log_probs, lengths, tokens, token_len):
        """Word spans for the hypotheses of a whole-utterance search: one cm_ctc_align launch over the (batch x topk) token
        sequences the kernel returned (rows past num_hyps hold no tokens and align as empty), then the word grouping."""
        b, topk, _ = tokens.shape
        lens = token_len.cpu().tolist()
        lmax = max((lens[u][h] for u in range(b) for h in range(len(hyps[u]))), default=0)
        if lmax > 1023:
            raise ValueError(f"{type(self).__name__}: text_frames aligns at most 1023 tokens per hypothesis, got {lmax}")
        dev = log_probs.device
        tl = token_len.reshape(-1).clamp(max=lmax)
        _, status, _, starts, ends, logp = ops.ctc_align(
            log_probs, tokens.reshape(b * topk, -1)[:, :lmax], lengths.repeat_interleave(topk), tl, blank=self.blank_index,
            rows=torch.arange(b, dtype=torch.int32, device=dev).repeat_interleave(topk))
        status, starts, ends, logp = status.cpu().tolist(), starts.cpu().tolist(), ends.cpu().tolist(), logp.cpu().tolist()
        tok = tokens[:, :, :lmax].cpu().tolist()
        for u in range(b):
            for h, hyp in enumerate(hyps[u]):
                r, k = u * topk + h, lens[u][h]
                if status[r] != 0:
                    raise ValueError(f"{type(self).__name__}: the tokens of hypothesis {h} of utterance {u} have no alignment "
                                     f"(status {status[r]})")
                hyp.text_frames = group_words(tok[u][h][:k], starts[r][:k], ends[r][:k], logp[r][:k], self.classes, self.clean)[1]
        return hyps

    def _hypotheses(self, tokens, token_len, scores, num_hyps, bad, rows, what, lm_scores=None) -> List[List[CTCHypothesis]]:
        """The kernel's outputs of the named rows, read to the host: NaN check, then one list of hypotheses per row."""
        bad, num_hyps = bad.cpu().tolist(), num_hyps.cpu().tolist()
        for u in rows:
            if bad[u] >= 0:
                raise ValueError(f"{type(self).__name__}: log_probs of {what} {u} hold NaN at frame {bad[u]}")
        token_len, scores = token_len.cpu().tolist(), scores.cpu().tolist()
        lm_scores = scores if lm_scores is None else lm_scores.cpu().tolist()
        lmax = max((token_len[u][h] for u in rows for h in range(num_hyps[u])), default=0)
        tok = tokens[:, :, :lmax].cpu().tolist()
        out = []
        for u in rows:
            hyps = []
            for h in range(num_hyps[u]):
                s = scores[u][h]
                hyps.append(CTCHypothesis(self.compose(tok[u][h][:token_len[u][h]]), None, s, lm_scores[u][h], None))
            out.append(hyps)
        return out

    def decode_beams(self, log_probs, wav_lens=None, lm_start_state=None):
        """speechbrain's name for the same call."""
        return self(log_probs, wav_lens)


@dataclass
class CTCAlignment:
    """One utterance's forced alignment.  status 0: aligned; 1: the labels do not fit the frames (the lists are empty, score is
    -inf).  Frames are half-open spans [start, end) of log_probs rows; ConMambaASR.align adds token_times / word_times in seconds."""
    status: int
    score: float
    tokens: List[int]
    token_frames: List[tuple]
    token_logp: List[float]
    words: List[str]
    word_frames: List[tuple]
    word_logp: List[float]
    token_times: Optional[List[tuple]] = None
    word_times: Optional[List[tuple]] = None


class CTCAligner:
    """CTC forced alignment of known label sequences on the GPU (cm_ctc_align; the contract is in the module docstring).

    __call__(log_probs (batch, T, V) on the GPU, targets: a padded (batch, S) integer tensor or a list of id lists, target_lens
    (batch) label counts (None with a list of lists), wav_lens relative lengths or None, lengths=None: absolute frame counts, which
    win when given) -> List[CTCAlignment].  Status 2 (NaN on the lattice) raises ValueError naming the utterance.  There is no host
    implementation: CPU tensors raise."""

    def __init__(self, blank_index: int, vocab_list: Sequence[str], space_token: str = " ", spm_token: str = "▁"):
        vocab = list(vocab_list)
        if not 0 <= blank_index < len(vocab):
            raise ValueError(f"CTCAligner: blank_index {blank_index} outside a vocabulary of {len(vocab)}")
        self.blank_index, self.vocab_list = int(blank_index), vocab
        self.space_token, self.spm_token = space_token, spm_token
        self.is_spm, self.classes, self.clean = classify_vocab(vocab, self.blank_index, space_token, spm_token)

    def words(self, tokens, starts, ends, logp):
        """group_words with this vocabulary's classes."""
        return group_words(tokens, starts, ends, logp, self.classes, self.clean)

    def __call__(self, log_probs: torch.Tensor, targets, target_lens=None, wav_lens: Optional[torch.Tensor] = None,
                 lengths=None) -> List[CTCAlignment]:
        if not log_probs.is_cuda:
            raise RuntimeError("CTCAligner runs on the GPU only (got a CPU tensor): move log_probs to the GPU")
        if log_probs.dim() != 3 or log_probs.shape[2] != len(self.vocab_list):
            raise ValueError(f"CTCAligner: log_probs must be (batch, T, {len(self.vocab_list)}), got {tuple(log_probs.shape)}")
        b, steps, v = log_probs.shape
        dev = log_probs.device
        if isinstance(targets, torch.Tensor):
            if targets.dim() != 2 or targets.shape[0] != b or target_lens is None:
                raise ValueError(f"CTCAligner: a targets tensor must be ({b}, S) and come with target_lens")
            tl = [int(x) for x in (target_lens.detach().cpu().tolist() if isinstance(target_lens, torch.Tensor) else target_lens)]
            ids = targets.detach().cpu().tolist()
        else:
            ids = [[int(x) for x in row] for row in targets]
            tl = [len(row) for row in ids] if target_lens is None else [int(x) for x in target_lens]
        if len(ids) != b or len(tl) != b or any(not 0 <= k <= len(row) for k, row in zip(tl, ids)):
            raise ValueError(f"CTCAligner: need {b} label sequences and {b} target_lens within them, got lengths {tl}")
        ids = [row[:k] for row, k in zip(ids, tl)]
        for u, row in enumerate(ids):
            if any(not 0 <= x < v for x in row):
                raise ValueError(f"CTCAligner: utterance {u} has a label outside the vocabulary of {v}")
        s = max(tl, default=0)
        if s > 1023:
            raise ValueError(f"CTCAligner: at most 1023 labels per utterance, got {s}")
        if lengths is None:
            counts = _frame_counts(steps, wav_lens, b)
        else:
            counts = [int(x) for x in lengths]
            if len(counts) != b or any(not 0 <= x <= steps for x in counts):
                raise ValueError(f"CTCAligner: lengths must be {b} frame counts in [0, {steps}], got {counts}")
        if steps == 0:
            return [CTCAlignment(0 if not row else 1, 0.0 if not row else -math.inf, [], [], [], [], [], []) for row in ids]
        padded = torch.tensor([row + [0] * (s - len(row)) for row in ids], dtype=torch.int64).reshape(b, s).to(dev)
        score, status, _, starts, ends, logp = ops.ctc_align(
            log_probs, padded, torch.tensor(counts, dtype=torch.int32).to(dev), torch.tensor(tl, dtype=torch.int32).to(dev),
            blank=self.blank_index)
        score, status = score.cpu().tolist(), status.cpu().tolist()
        starts, ends, logp = starts.cpu().tolist(), ends.cpu().tolist(), logp.cpu().tolist()
        out = []
        for u, row in enumerate(ids):
            if status[u] == 2:
                raise ValueError(f"CTCAligner: log_probs of utterance {u} hold NaN on its alignment lattice")
            if status[u] != 0:
                out.append(CTCAlignment(status[u], score[u], [], [], [], [], [], []))
                continue
            k = len(row)
            a, z, lp = starts[u][:k], ends[u][:k], logp[u][:k]
            words, frames, wlp = self.words(row, a, z, lp)
            out.append(CTCAlignment(0, score[u], row, list(zip(a, z)), lp, words, frames, wlp))
        return out


def greedy_host(log_probs: torch.Tensor, counts: Sequence[int], blank: int):
    """The greedy contract of the module docstring on the host (CPU tensors; the GPU kernel's bits).
    -> per utterance (status, tokens, starts, ends, token_logp) as host lists."""
    out = []
    for row, n in zip(log_probs.detach().cpu(), counts):
        x = row[:n].double()                                         # exact from fp32 and bf16
        if bool(torch.isnan(x).any()):
            out.append((2, [], [], [], []))
            continue
        if n == 0:
            out.append((0, [], [], [], []))
            continue
        top = x.max(dim=-1, keepdim=True).values                     # the lowest index attaining it, whatever argmax would pick
        idx = torch.where(x == top, torch.arange(x.shape[1])[None, :], x.shape[1]).min(dim=-1).values
        best, vals = idx.tolist(), x.gather(1, idx[:, None])[:, 0].tolist()
        tokens, starts, ends, logp = [], [], [], []
        for t, v in enumerate(best):
            if v != blank and (t == 0 or v != best[t - 1]):
                tokens.append(v), starts.append(t), ends.append(t + 1), logp.append(vals[t])
            elif v != blank:
                ends[-1], logp[-1] = t + 1, logp[-1] + vals[t]
        out.append((0, tokens, starts, ends, logp))
    return out


class CTCGreedyDecoder:
    """Greedy CTC decoding (the VALID stage's decode, reference train_CTC.py:305-310): per frame the arg-max, repeats collapsed,
    blanks removed -- dataio.ctc_greedy_decode's tokens, plus each token's frames and log-probability, from cm_ctc_greedy on the
    GPU (no host loop over frames) and from greedy_host on CPU tensors, with the same bits.

    The contract (ops.ctc_greedy, csrc/ctc_greedy.hip; pinned by tests/ctc_score_ref.py).  n_b frames are decoded.
    best[t] = the LOWEST index attaining frame t's maximum; -inf is an ordinary value (an all -inf frame gives index 0).  Frame t is
    kept when best[t] != blank and (t == 0 or best[t] != best[t-1]): a run broken by blank starts a new token.  A kept token's span
    is [first frame of its run, one past the last), its log-probability the float64 left fold, in increasing t, of
    (double) lp[t][token] over the run.  A NaN in any frame < n_b gives that utterance status 2 (ValueError here, naming the
    utterance); frames at and past n_b are never read.

    __call__(log_probs (batch, T, V), wav_lens (batch) relative lengths or None, lengths=None: absolute frame counts, which win
    when given) -> one CTCHypothesis per utterance: ``tokens`` the kept ids, ``text`` their composition by the class rules when a
    vocabulary was given (else ""), ``text_frames`` the words' spans (group_words; None without a vocabulary), ``score`` the sum of
    the tokens' log-probabilities.  .tokens(log_probs, wav_lens) -> List[List[int]]."""

    def __init__(self, blank_index: int, vocab_list: Optional[Sequence[str]] = None, space_token: str = " ", spm_token: str = "▁"):
        self.blank_index = int(blank_index)
        self.vocab_list = None if vocab_list is None else list(vocab_list)
        self.space_token, self.spm_token = space_token, spm_token
        if self.blank_index < 0 or (self.vocab_list is not None and self.blank_index >= len(self.vocab_list)):
            raise ValueError(f"CTCGreedyDecoder: blank_index {blank_index} outside the vocabulary")
        if self.vocab_list is not None:
            self.is_spm, self.classes, self.clean = classify_vocab(self.vocab_list, self.blank_index, space_token, spm_token)

    def compose(self, tokens: Sequence[int]) -> str:
        return CTCBeamSearcher.compose(self, tokens)

    def _decode(self, log_probs, wav_lens, lengths, spans=True):
        """-> per utterance (tokens, starts, ends, token_logp) as host lists; spans=False reads the tokens back alone (the other
        three are None).  Status 2 raises."""
        if log_probs.dim() != 3 or (self.vocab_list is not None and log_probs.shape[2] != len(self.vocab_list)):
            raise ValueError(f"CTCGreedyDecoder: log_probs must be (batch, T, V) over the vocabulary, got {tuple(log_probs.shape)}")
        b, steps, v = log_probs.shape
        if not self.blank_index < v:
            raise ValueError(f"CTCGreedyDecoder: blank_index {self.blank_index} outside the {v} classes of log_probs")
        if lengths is None:
            counts = _frame_counts(steps, wav_lens, b)
        else:
            counts = [int(x) for x in lengths]
            if len(counts) != b or any(not 0 <= x <= steps for x in counts):
                raise ValueError(f"CTCGreedyDecoder: lengths must be {b} frame counts in [0, {steps}], got {counts}")
        if b == 0 or steps == 0:
            return [([], [], [], []) for _ in range(b)]
        if not log_probs.is_cuda:
            rows = greedy_host(log_probs, counts, self.blank_index)
            status, rows = [r[0] for r in rows], [r[1:] for r in rows]
        else:
            tokens, token_len, starts, ends, logp, status = ops.ctc_greedy(
                log_probs, torch.tensor(counts, dtype=torch.int32).to(log_probs.device), blank=self.blank_index)
            k, status = torch.stack((token_len, status)).cpu().tolist()          # one read-back for both
            kmax = max(k)
            cols = [x[:, :kmax].cpu().tolist() if (spans or x is tokens) else None for x in (tokens, starts, ends, logp)]
            rows = [tuple(None if c is None else c[u][:k[u]] for c in cols) for u in range(b)]
        for u, s in enumerate(status):
            if s == 2:
                raise ValueError(f"CTCGreedyDecoder: log_probs of utterance {u} hold NaN inside its length")
        return rows

    def tokens(self, log_probs: torch.Tensor, wav_lens: Optional[torch.Tensor] = None, lengths=None) -> List[List[int]]:
        return [row[0] for row in self._decode(log_probs, wav_lens, lengths, spans=False)]

    def __call__(self, log_probs: torch.Tensor, wav_lens: Optional[torch.Tensor] = None, lengths=None) -> List[CTCHypothesis]:
        out = []
        for tok, starts, ends, logp in self._decode(log_probs, wav_lens, lengths):
            score = float(sum(logp))
            hyp = CTCHypothesis("", None, score, score, None, tok)
            if self.vocab_list is not None:
                hyp.text = self.compose(tok)
                hyp.text_frames = group_words(tok, starts, ends, logp, self.classes, self.clean)[1]
            out.append(hyp)
        return out


class CTCStreamState:
    """The streams of one StreamingCTCBeamSearcher.make_state call: the device slab (slots, state bytes) uint8 -- plain memory, a
    row copied is a stream copied -- and per slot the host's upper bound of frames fed since the last reset (None: never reset)."""

    def __init__(self, searcher: "StreamingCTCBeamSearcher", slab: torch.Tensor):
        self._searcher, self.slab = searcher, slab
        self.fed: List[Optional[int]] = [None] * slab.shape[0]

    @property
    def batch_size(self) -> int:
        return self.slab.shape[0]

    def reset(self, rows: Optional[Sequence[int]] = None) -> None:
        """Start a new utterance in the named slots (default all), now: one launch that consumes nothing."""
        rows = self._searcher._rows(self, rows)
        self._searcher._launch(self, None, [0] * self.batch_size, reset=rows)
        for u in rows:
            self.fed[u] = 0


class StreamingCTCBeamSearcher(CTCBeamSearcher):
    """CTCBeamSearcher carried across chunks (cm_ctc_beam_stream): the constructor keywords of CTCBeamSearcher plus
    max_frames, the frames one utterance (reset to reset) may hold -- 1500 is a minute of 40-ms encoder frames.  After n frames in
    any chunking, hypotheses() returns what CTCBeamSearcher returns for those n frames, score bits included.  This class is the
    LM-free search and refuses kenlm_model_path; StreamingCTCBeamLMSearcher below streams the LM-fused one.

        state = searcher.make_state(batch_size, device); state.reset()
        searcher.step(log_probs_chunk, state)           # per chunk: one launch, nothing read back
        searcher.hypotheses(state)                      # whenever wanted, in mid-stream too: the beams are left as they are
    """

    def __init__(self, *args, max_frames: int = 1500, **kw):
        if kw.get("kenlm_model_path") is not None or (len(args) > 4 and args[4] is not None):
            raise NotImplementedError("StreamingCTCBeamSearcher is LM-free: streamed language-model fusion (kenlm_model_path) is "
                                      "StreamingCTCBeamLMSearcher's; CTCBeamSearcher fuses an n-gram LM over whole utterances")
        self._init_searcher(args, kw, max_frames)

    def _init_searcher(self, args, kw, max_frames):
        CTCBeamSearcher.__init__(self, *args, **kw)
        if not 1 <= max_frames <= 0x7fff0000 // 256:
            raise ValueError(f"{type(self).__name__}: max_frames {max_frames} not in [1, {0x7fff0000 // 256}]")
        self.max_frames = int(max_frames)
        self._dev_lengths = {}

    def make_state(self, batch_size: int, device) -> CTCStreamState:
        """``batch_size`` slots that were never reset: reset them (state.reset, or step's ``reset``) before their first chunk."""
        return CTCStreamState(self, ops.ctc_beam_stream_state(batch_size, self.beam_size, self.max_frames, device))

    def _rows(self, state, rows) -> List[int]:
        rows = list(range(state.batch_size)) if rows is None else [int(u) for u in rows]
        for u in rows:
            if not 0 <= u < state.batch_size:
                raise ValueError(f"{type(self).__name__}: slot {u} outside a state of {state.batch_size} slots")
        return rows

    def _flags(self, values: Sequence[int], device) -> torch.Tensor:
        return torch.tensor(list(values), dtype=torch.int32).to(device)

    def _constant(self, value: int, n: int, device) -> torch.Tensor:
        """(n) int32 of ``value`` on the device, made once: a step without host lists uploads nothing."""
        key = (str(device), n, value)
        if key not in self._dev_lengths:
            self._dev_lengths[key] = torch.full((n,), value, dtype=torch.int32, device=device)
        return self._dev_lengths[key]

    def _launch(self, state, log_probs, lengths, reset=None, emit=None):
        dev, n = state.slab.device, state.batch_size
        tc, th, tp = self._tables(dev)
        same = len(set(lengths)) == 1
        chunk_len = self._constant(lengths[0], n, dev) if same else self._flags(lengths, dev)

        def mark(rows):
            return self._flags([1 if u in rows else 0 for u in range(n)], dev) if rows else None
        return ops.ctc_beam_stream(
            log_probs, chunk_len, state.slab, self.max_frames, tc, th, tp, HASH_BASE, HASH_SEP, reset=mark(reset), emit=mark(emit),
            blank=self.blank_index, beam_size=self.beam_size, topk=self.topk, prune_history=self.prune_history,
            beam_prune_logp=self.beam_prune_logp, token_prune_min_logp=self.token_prune_min_logp,
            blank_skip_threshold=self.blank_skip_threshold)

    def step(self, log_probs: torch.Tensor, state: CTCStreamState, lengths: Optional[Sequence[int]] = None,
             reset: Optional[Sequence[int]] = None) -> None:
        """Feed the next chunk log_probs (B, t, V): slot b consumes its first lengths[b] rows (host list; default t; 0: idle).
        ``reset``: host list of the slots that start a new utterance with this chunk.  One launch and nothing read from the
        device; with neither list given nothing is uploaded either, so the call can be captured in a hipGraph with the encoder
        step -- after one eager call of the same (B, t) on this searcher, which makes the cached device constants outside the
        graph's memory pool (the host's frame count sees the capture once, not the replays: the device then refuses a chunk past max_frames on
        its own, status -2).  Raises ValueError before launching when a slot was never reset or would pass max_frames."""
        n = state.batch_size
        if log_probs.dim() != 3 or log_probs.shape[0] != n or log_probs.shape[2] != len(self.vocab_list):
            raise ValueError(f"{type(self).__name__}: log_probs must be ({n}, t, {len(self.vocab_list)}), got {tuple(log_probs.shape)}")
        t = log_probs.shape[1]
        lengths = [t] * n if lengths is None else [int(x) for x in lengths]
        if len(lengths) != n or any(not 0 <= x <= t for x in lengths):
            raise ValueError(f"{type(self).__name__}: lengths must be {n} frame counts in [0, {t}], got {lengths}")
        reset = self._rows(state, reset) if reset is not None else []
        fed = list(state.fed)
        for u in reset:
            fed[u] = 0
        for u, x in enumerate(lengths):
            if x and fed[u] is None:
                raise ValueError(f"{type(self).__name__}: slot {u} was never reset: pass reset=[{u}] with its first chunk, or call state.reset([{u}])")
            if x and fed[u] + x > self.max_frames:
                raise ValueError(f"{type(self).__name__}: slot {u} would hold {fed[u] + x} frames, more than max_frames={self.max_frames}: "
                                 "end-point the utterance and reset the slot")
            if x:
                fed[u] += x
        if not log_probs.is_cuda or not state.slab.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (got a CPU tensor): move log_probs and the state to the GPU")
        if t and (reset or any(lengths)):
            self._launch(state, log_probs, lengths, reset=reset)
        elif reset:
            self._launch(state, None, [0] * n, reset=reset)
        state.fed = fed

    def hypotheses(self, state: CTCStreamState, rows: Optional[Sequence[int]] = None) -> List[List[CTCHypothesis]]:
        """The hypotheses of the named slots (default all) after the frames fed so far, one list per named slot in the order given:
        an emit-only launch, then the one host read.  The beams stay as they are: callable any number of times, in mid-stream
        and at the end.  A slot never reset has no hypotheses.  Raises ValueError naming the slot and the frame, counted from its
        reset, when the slot met a NaN."""
        rows = self._rows(state, rows)
        if not state.slab.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (got a CPU state)")
        if not rows:
            return []
        tokens, token_len, scores, num_hyps, status = self._launch(state, None, [0] * state.batch_size, emit=rows)
        return self._hypotheses(tokens, token_len, scores, num_hyps, status, rows, "slot")


class StreamingCTCBeamLMSearcher(StreamingCTCBeamSearcher):
    """StreamingCTCBeamSearcher with the n-gram LM of CTCBeamSearcher(kenlm_model_path=...) fused into the streamed search
    (cm_ctc_beam_lm_stream): the same constructor keywords, ``kenlm_model_path`` required and validated as
    CTCBeamSearcher validates it, plus max_frames.  After n frames in any chunking, hypotheses() returns what
    CTCBeamSearcher(kenlm_model_path=...) returns for those n frames -- CTCHypothesis(text, None, score=acoustic, lm_score=total,
    None), score and lm_score bits included.  make_state, step (lengths=, reset=, hipGraph capture after one eager call),
    state.reset and hypotheses are the base class's; a step uploads nothing, the LM tables being cached on the device.  A state
    belongs to the searcher (the LM tables) that advanced it: its slabs hold entry numbers of those tables."""

    def __init__(self, *args, max_frames: int = 1500, **kw):
        if kw.get("kenlm_model_path") is None and not (len(args) > 4 and args[4] is not None):
            raise ValueError("StreamingCTCBeamLMSearcher: kenlm_model_path is required (StreamingCTCBeamSearcher is the LM-free "
                             "streamed search)")
        self._init_searcher(args, kw, max_frames)

    def make_state(self, batch_size: int, device) -> CTCStreamState:
        """``batch_size`` slots that were never reset, their slabs sized for the LM state as well."""
        return CTCStreamState(self, ops.ctc_beam_lm_stream_state(batch_size, self.beam_size, self.max_frames, device))

    def _launch(self, state, log_probs, lengths, reset=None, emit=None):
        dev, n = state.slab.device, state.batch_size
        tc, th, tp = self._tables(dev)
        lm = self.lm
        same = len(set(lengths)) == 1
        chunk_len = self._constant(lengths[0], n, dev) if same else self._flags(lengths, dev)

        def mark(rows):
            return self._flags([1 if u in rows else 0 for u in range(n)], dev) if rows else None
        return ops.ctc_beam_lm_stream(
            log_probs, chunk_len, state.slab, self.max_frames, tc, th, tp, self._tok_len(dev), HASH_BASE, HASH_SEP, lm.tables(dev),
            order=lm.order, n_words=len(lm.words), lm_bos=lm.bos if self.score_boundary else -1,
            lm_eos=lm.eos if self.score_boundary else -1, lm_unk=lm.unk, alpha=self.alpha, beta=self.beta,
            unk_score_offset=self.unk_score_offset, reset=mark(reset), emit=mark(emit), blank=self.blank_index,
            beam_size=self.beam_size, topk=self.topk, prune_history=self.prune_history, beam_prune_logp=self.beam_prune_logp,
            token_prune_min_logp=self.token_prune_min_logp, blank_skip_threshold=self.blank_skip_threshold)

    def hypotheses(self, state: CTCStreamState, rows: Optional[Sequence[int]] = None) -> List[List[CTCHypothesis]]:
        """As StreamingCTCBeamSearcher.hypotheses; each hypothesis carries score = its acoustic score and lm_score = its total, by
        which the list is ranked."""
        rows = self._rows(state, rows)
        if not state.slab.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only (got a CPU state)")
        if not rows:
            return []
        tokens, token_len, scores, lm_scores, num_hyps, status = self._launch(state, None, [0] * state.batch_size, emit=rows)
        return self._hypotheses(tokens, token_len, scores, num_hyps, status, rows, "slot", lm_scores=lm_scores)
