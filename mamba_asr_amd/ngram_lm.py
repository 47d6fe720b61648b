"""Backoff n-gram language models in ARPA text format, packed into plain tensors the LM-fused CTC beam search probes on the
device (csrc/ctc_beam_lm.hip behind ops.ctc_beam_search_lm; contract and layout: DESIGN.md §4p).

    lm = NgramLM.from_arpa(path, unigrams=None)      # plain or .gz, order 1 .. 5
    lm.score(("THE", "CAT"), "SAT")                  # -> (log10 p, next context), read through the packed tables
    lm.tables(device)                                # the tensors, uploaded once per device

Layout.  Every n-gram of the file is an entry; entries are numbered order by order in file order, so the unigram of word id w
is entry w.  prob / backoff (entries) fp32 hold log10 p and the backoff weight (0 when the file gives none).  Three open-
addressing tables with linear probing, capacities powers of two of at least twice the entry count, empty key = all ones:
  word table    key = the two 61-bit piece_hash values of the word string (the identity the search uses for text) -> word id;
  prefix set    the same kind of key for every non-empty prefix of every unigram-list word (``unigrams`` when given, else the
                1-grams minus <s>, </s>, <unk>);
  n-gram table  key = (entry of the context as an (n-1)-gram << 32) | word id -> entry, for n >= 2.
slot(key) = mix(key) & (cap - 1) for the n-gram table and mix(h0 * 0x9E3779B97F4A7C15 + h1) for the hash pairs, mix being the
splitmix64 finaliser.  A context is therefore the tuple of the entries of its last 1 .. order-1 words (-1: not stored); one word
costs at most ``order`` independent probes and yields the next context.

Choices.  An n-gram whose first n-1 words are not listed as an (n-1)-gram cannot be keyed and is refused as malformed (kenlm's
trie builder refuses such files as well).  Non-finite numbers are refused.  Numbers are rounded to fp32 once, at parse time.
"""
from __future__ import annotations

import gzip
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

MAX_ORDER = 5
SPECIALS = ("<s>", "</s>", "<unk>")
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
_M64 = (1 << 64) - 1
_PAIR_MUL = 0x9E3779B97F4A7C15


def _mix(x: int) -> int:
    x &= _M64
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _M64
    return x ^ (x >> 31)


def _mix_np(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def _capacity(n: int) -> int:
    cap = 2
    while cap < 2 * n:
        cap <<= 1
    return cap


def _place(home: np.ndarray, cap: int) -> np.ndarray:
    """Linear-probing slots for keys with the given home slots, inserted in rounds: -> slot per key (all distinct)."""
    mask = cap - 1
    used = np.zeros(cap, dtype=bool)
    slot = home.astype(np.int64) & mask
    out = np.full(len(home), -1, dtype=np.int64)
    pending = np.arange(len(home))
    while pending.size:
        s = slot[pending]
        free = ~used[s]
        uniq, first = np.unique(s[free], return_index=True)
        winners = pending[free][first]
        out[winners] = uniq
        used[uniq] = True
        pending = pending[out[pending] < 0]
        slot[pending] = (slot[pending] + 1) & mask
    return out


def _open(path: str):
    with open(path, "rb") as f:
        magic = f.read(2)
    return gzip.open(path, "rb") if magic == b"\x1f\x8b" else open(path, "rb")


class NgramLM:
    """A parsed and packed ARPA model.  ``words[w]`` is the string of word id w; ``bos`` / ``eos`` / ``unk`` are the word ids of
    <s>, </s>, <unk> (-1 when the file does not list them); ``counts[n - 1]`` the number of n-grams."""

    def __init__(self, order, words, prob, backoff, ngram_ctx, ngram_word, unigrams=None, path="<memory>"):
        from .ctc_decode import HASH_BASE, P61
        self.path, self.order, self.words = path, int(order), list(words)
        self.word_id: Dict[str, int] = {w: i for i, w in enumerate(self.words)}
        self.bos, self.eos, self.unk = (self.word_id.get(s, -1) for s in SPECIALS)
        self.prob = np.asarray(prob, dtype=np.float32)
        self.backoff = np.asarray(backoff, dtype=np.float32)
        self.n_entries = len(self.prob)
        if self.n_entries >= 1 << 31:
            raise ValueError(f"{path}: {self.n_entries} n-grams, more than 2^31 - 1")
        self.unigram_list = [w for w in self.words if w not in SPECIALS] if unigrams is None else [str(w) for w in unigrams]

        def hashes(strings, prefixes):
            """piece_hash of every string (or of every non-empty prefix of every string), as a set-free (n, 2) uint64 array."""
            out = []
            for s in strings:
                h0 = h1 = 0
                for i, ch in enumerate(s):
                    c = ord(ch) + 1
                    h0 = (h0 * HASH_BASE[0] + c) % P61
                    h1 = (h1 * HASH_BASE[1] + c) % P61
                    if prefixes or i == len(s) - 1:
                        out.append((h0, h1))
                if not s and not prefixes:
                    out.append((0, 0))
            return np.array(out, dtype=np.uint64).reshape(-1, 2)

        def pair_home(h):
            with np.errstate(over="ignore"):
                return _mix_np(h[:, 0] * np.uint64(_PAIR_MUL) + h[:, 1])

        wh = hashes(self.words, False)
        if len(np.unique(wh, axis=0)) != len(self.words):
            raise ValueError(f"{path}: two words of the vocabulary share both 61-bit hashes")
        self.word_cap = _capacity(len(self.words))
        self.word_keys = np.full((self.word_cap, 2), _EMPTY, dtype=np.uint64)
        self.word_ids = np.full(self.word_cap, -1, dtype=np.int32)
        slots = _place(pair_home(wh), self.word_cap)
        self.word_keys[slots] = wh
        self.word_ids[slots] = np.arange(len(self.words), dtype=np.int32)

        ph = hashes(self.unigram_list, True)
        ph = np.unique(ph, axis=0) if len(ph) else ph
        self.prefix_cap = _capacity(len(ph))
        self.prefix_keys = np.full((self.prefix_cap, 2), _EMPTY, dtype=np.uint64)
        if len(ph):
            self.prefix_keys[_place(pair_home(ph), self.prefix_cap)] = ph

        ctx = np.asarray(ngram_ctx, dtype=np.uint64)
        keys = (ctx << np.uint64(32)) | np.asarray(ngram_word, dtype=np.uint64)
        self.ngram_cap = _capacity(len(keys))
        self.ngram_keys = np.full(self.ngram_cap, _EMPTY, dtype=np.uint64)
        self.ngram_vals = np.full(self.ngram_cap, -1, dtype=np.int32)
        if len(keys):
            slots = _place(_mix_np(keys), self.ngram_cap)
            self.ngram_keys[slots] = keys
            self.ngram_vals[slots] = np.arange(len(self.words), len(self.words) + len(keys), dtype=np.int32)
        self._dev = {}

    # ---- parsing ----
    @classmethod
    def from_arpa(cls, path: str, unigrams: Optional[Sequence[str]] = None) -> "NgramLM":
        """Parse an ARPA file (plain or gzip).  Raises ValueError naming the path and the line for a kenlm binary file or a
        malformed ARPA file."""
        path = str(path)

        def bad(no, why):
            return ValueError(f"{path}: line {no}: {why}")

        counts: List[int] = []
        words: List[str] = []
        prob: List[float] = []
        backoff: List[float] = []
        nctx: List[int] = []
        nword: List[int] = []
        index: List[Dict[Tuple[int, int], int]] = []      # per order n >= 2: (context entry, word id) -> entry
        word_id: Dict[str, int] = {}
        section, seen, state, no = 0, 0, "start", 0
        with _open(path) as f:
            for no, raw in enumerate(f, 1):
                if no == 1 and raw.startswith(b"mmap lm "):
                    raise bad(1, "a kenlm binary file, not ARPA text: convert it back to ARPA (it holds no text to parse)")
                try:
                    line = raw.decode("utf-8").strip()
                except UnicodeDecodeError:
                    raise bad(no, "not UTF-8 text (a kenlm binary file?)") from None
                if not line:
                    continue
                if state == "start":
                    if line != "\\data\\":
                        raise bad(no, f"expected \\data\\, got {line[:40]!r}")
                    state = "counts"
                elif state == "counts" and line.startswith("ngram "):
                    try:
                        n, c = line[6:].split("=")
                        n, c = int(n), int(c)
                    except ValueError:
                        raise bad(no, f"malformed count line {line!r}") from None
                    if n != len(counts) + 1 or c < 0:
                        raise bad(no, f"count line out of order or negative: {line!r}")
                    if n > MAX_ORDER:
                        raise bad(no, f"order {n} above the supported {MAX_ORDER}")
                    counts.append(c)
                elif line.startswith("\\") and line.endswith("-grams:") and state in ("counts", "grams"):
                    if state == "grams" and seen != counts[section - 1]:
                        raise bad(no, f"{seen} {section}-grams listed, the header announces {counts[section - 1]}")
                    if not counts or line != f"\\{section + 1}-grams:" or section + 1 > len(counts):
                        raise bad(no, f"unexpected section {line!r}")
                    section, seen, state = section + 1, 0, "grams"
                    if section >= 2:
                        index.append({})
                elif line == "\\end\\" and state == "grams":
                    if seen != counts[section - 1]:
                        raise bad(no, f"{seen} {section}-grams listed, the header announces {counts[section - 1]}")
                    if section != len(counts):
                        raise bad(no, f"\\end\\ after the {section}-grams of an order-{len(counts)} model")
                    state = "end"
                elif state == "grams":
                    parts = line.split()
                    if len(parts) not in (section + 1, section + 2):
                        raise bad(no, f"a {section}-gram line needs {section + 1} or {section + 2} fields, got {len(parts)}")
                    try:
                        p = float(parts[0])
                        bo = float(parts[section + 1]) if len(parts) == section + 2 else 0.0
                    except ValueError:
                        raise bad(no, f"not a number in {line!r}") from None
                    if not (math.isfinite(p) and math.isfinite(bo)):
                        raise bad(no, f"non-finite number in {line!r}")
                    ws = parts[1:section + 1]
                    if section == 1:
                        if ws[0] in word_id:
                            raise bad(no, f"1-gram {ws[0]!r} listed twice")
                        word_id[ws[0]] = len(words)
                        words.append(ws[0])
                    else:
                        if len(words) != counts[0]:
                            raise bad(no, "n-grams before the 1-grams are complete")
                        ctx = -1
                        for k, w in enumerate(ws):
                            wid = word_id.get(w)
                            if wid is None:
                                raise bad(no, f"word {w!r} is not among the 1-grams")
                            if k == section - 1:
                                break
                            ctx = wid if k == 0 else index[k - 1].get((ctx, wid), -1)
                            if ctx < 0:
                                raise bad(no, f"the context {' '.join(ws[:k + 1])!r} is not listed as a {k + 1}-gram")
                        if (ctx, wid) in index[section - 2]:
                            raise bad(no, f"{section}-gram {' '.join(ws)!r} listed twice")
                        index[section - 2][(ctx, wid)] = len(prob)
                        nctx.append(ctx)
                        nword.append(wid)
                    prob.append(p)
                    backoff.append(bo)
                    seen += 1
                else:
                    raise bad(no, f"unexpected line {line[:40]!r}")
        if state != "end":
            raise bad(no + 1, "the file ends before \\end\\" if state != "start" else "no \\data\\ header: not an ARPA file")
        if not words:
            raise bad(no, "the model lists no 1-grams")
        return cls(len(counts), words, prob, backoff, nctx, nword, unigrams=unigrams, path=path)

    # ---- host probes: the kernel's rule, on the packed arrays ----
    def _find_pair(self, keys, cap, h0, h1) -> int:
        mask = cap - 1
        s = _mix(h0 * _PAIR_MUL + h1) & mask
        for _ in range(cap):
            k0 = int(keys[s, 0])
            if k0 == _M64:
                return -1
            if k0 == h0 and int(keys[s, 1]) == h1:
                return s
            s = (s + 1) & mask
        return -1

    def lookup_word(self, word: str) -> int:
        """Word id through the packed word table, -1 for a word outside the vocabulary."""
        from .ctc_decode import piece_hash
        h, _ = piece_hash(word)
        s = self._find_pair(self.word_keys, self.word_cap, h[0], h[1])
        return int(self.word_ids[s]) if s >= 0 else -1

    def is_prefix(self, partial: str) -> bool:
        """Whether ``partial`` (non-empty) is a prefix of, or equal to, a unigram-list word, through the packed prefix set."""
        from .ctc_decode import piece_hash
        h, _ = piece_hash(partial)
        return self._find_pair(self.prefix_keys, self.prefix_cap, h[0], h[1]) >= 0

    def _ngram(self, ctx: int, w: int) -> int:
        key, mask = (ctx << 32) | w, self.ngram_cap - 1
        s = _mix(key) & mask
        for _ in range(self.ngram_cap):
            k = int(self.ngram_keys[s])
            if k == _M64:
                return -1
            if k == key:
                return int(self.ngram_vals[s])
            s = (s + 1) & mask
        return -1

    def initial_state(self, bos: bool) -> Tuple[int, ...]:
        """The context entries before the first word: <s> when ``bos`` and the model lists it, else nothing."""
        st = [-1] * (MAX_ORDER - 1)
        if bos and self.bos >= 0 and self.order >= 2:
            st[0] = self.bos
        return tuple(st)

    def advance(self, state: Sequence[int], w: int) -> Tuple[float, Tuple[int, ...]]:
        """log10 p(word id w | state) by ARPA backoff, and the state after w (lm_cond of the kernel)."""
        e = [w] + [self._ngram(state[k - 1], w) if k < self.order and state[k - 1] >= 0 else -1 for k in range(1, MAX_ORDER)]
        hit = max(k for k in range(MAX_ORDER) if e[k] >= 0)
        lw = float(self.prob[e[hit]])
        for j in range(hit + 1, self.order):
            if state[j - 1] >= 0:
                lw += float(self.backoff[state[j - 1]])
        return lw, tuple(e[k] if k + 1 < self.order else -1 for k in range(MAX_ORDER - 1))

    def advance_word(self, state: Sequence[int], word: str) -> Tuple[float, Tuple[int, ...], bool]:
        """(log10 p term, next state, in vocabulary): an out-of-vocabulary word scores and continues as <unk>; without <unk> it
        scores 0 and empties the context.  unk_score_offset is the search's to add."""
        w = self.lookup_word(word)
        if w >= 0:
            return self.advance(state, w) + (True,)
        if self.unk >= 0:
            return self.advance(state, self.unk) + (False,)
        return 0.0, tuple([-1] * (MAX_ORDER - 1)), False

    def score(self, context_words: Sequence[str], word: str) -> Tuple[float, Tuple[str, ...]]:
        """log10 p(word | context_words) and the context that follows, as words: the last order-1 of context + word, with every
        out-of-vocabulary word read as <unk> (or, when the model lists no <unk>, emptying the context up to and including it)."""
        state, ctx = self.initial_state(False), []
        for cw in context_words:
            _, state, known = self.advance_word(state, cw)
            ctx = ctx + [cw] if known else (ctx + ["<unk>"] if self.unk >= 0 else [])
        lw, _, known = self.advance_word(state, word)
        ctx = ctx + [word] if known else (ctx + ["<unk>"] if self.unk >= 0 else [])
        return lw, tuple(ctx[max(0, len(ctx) - (self.order - 1)):] if self.order > 1 else ())

    def lm_of_text(self, text: str, alpha: float, beta: float, unk_score_offset: float, score_boundary: bool, finish: bool = False) -> float:
        """LM(text) of the contract (float64); with ``finish`` the </s> term of the search's finish is added."""
        state, total, a = self.initial_state(score_boundary), 0.0, alpha * math.log(10.0)
        for w in text.split():
            lw, state, known = self.advance_word(state, w)
            total += a * (lw if known else lw + unk_score_offset) + beta
        if finish and score_boundary and self.eos >= 0:
            total += a * self.advance(state, self.eos)[0]
        return total

    # ---- device ----
    def tables(self, device):
        """The packed tensors on ``device`` (uploaded once): dict of word_keys (cap, 2), word_ids, prefix_keys (cap, 2), ngram_keys,
        ngram_vals, prob, backoff; the 64-bit keys travel as int64 bit patterns."""
        key = str(device)
        if key not in self._dev:
            def up(a):
                return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(device)
            self._dev[key] = {n: up(getattr(self, n)) for n in
                              ("word_keys", "word_ids", "prefix_keys", "ngram_keys", "ngram_vals", "prob", "backoff")}
        return self._dev[key]
