"""Float64 pure-Python restatement of the LM-fused CTC beam search contract (mamba_asr_amd/ctc_decode.py), written
for the tests: its own ARPA reader, a dict-based backoff scorer and the search; nothing here is imported from the package."""
import gzip
import math
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_ref as R  # noqa: E402

INF = math.inf


def _f32(x):
    return struct.unpack("f", struct.pack("f", float(x)))[0]


def read_arpa(path):
    """-> (order, vocabulary in file order, {words tuple: log10 p as fp32}, {words tuple: backoff as fp32, only where given})."""
    with open(path, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    with (gzip.open(path, "rt", encoding="utf-8") if gz else open(path, "r", encoding="utf-8")) as f:
        lines = [ln.strip() for ln in f]
    order, n, vocab, prob, bo = 0, 0, [], {}, {}
    for ln in lines:
        if not ln or ln == "\\data\\" or ln == "\\end\\":
            continue
        if ln.startswith("ngram "):
            order = max(order, int(ln[6:].split("=")[0]))
        elif ln.startswith("\\"):
            n = int(ln[1:].split("-")[0])
        else:
            parts = ln.split()
            words = tuple(parts[1:n + 1])
            prob[words] = _f32(parts[0])
            if len(parts) == n + 2:
                bo[words] = _f32(parts[n + 1])
            if n == 1:
                vocab.append(words[0])
    return order, vocab, prob, bo


class DictLM:
    def __init__(self, path, unigrams=None):
        self.order, self.vocab_list, self.prob, self.bo = read_arpa(path)
        self.vocab = set(self.vocab_list)
        self.unigrams = [w for w in self.vocab_list if w not in ("<s>", "</s>", "<unk>")] if unigrams is None else list(unigrams)

    def trunc(self, ctx):
        k = self.order - 1
        return tuple(ctx[len(ctx) - k:]) if k > 0 and len(ctx) > k else (tuple(ctx) if k > 0 else ())

    def cond(self, ctx, w):
        """log10 p(w | ctx), ctx and w inside the vocabulary: the longest stored n-gram, plus the backoff of every dropped context."""
        ctx = self.trunc(ctx)
        hit = max(k for k in range(len(ctx) + 1) if ctx[len(ctx) - k:] + (w,) in self.prob)
        lw = self.prob[ctx[len(ctx) - hit:] + (w,)]
        for j in range(hit + 1, len(ctx) + 1):
            lw += self.bo.get(ctx[len(ctx) - j:], 0.0)
        return lw

    def start(self, score_boundary):
        return self.trunc(("<s>",)) if score_boundary and "<s>" in self.vocab else ()

    def step(self, ctx, w, unk_score_offset):
        """(lw, next context) of the completed word w."""
        if w in self.vocab:
            return self.cond(ctx, w), self.trunc(tuple(ctx) + (w,))
        if "<unk>" in self.vocab:
            return self.cond(ctx, "<unk>") + unk_score_offset, self.trunc(tuple(ctx) + ("<unk>",))
        return unk_score_offset, ()

    def text_score(self, text, alpha, beta, unk_score_offset, score_boundary):
        """(LM(text), the context after it)."""
        ctx, total = self.start(score_boundary), 0.0
        for w in text.split():
            lw, ctx = self.step(ctx, w, unk_score_offset)
            total += alpha * math.log(10) * lw + beta
        return total, ctx

    def eos_term(self, ctx, alpha, score_boundary):
        return alpha * math.log(10) * self.cond(ctx, "</s>") if score_boundary and "</s>" in self.vocab else 0.0

    def is_prefix(self, p):
        return any(u.startswith(p) for u in self.unigrams)

    def partial_score(self, p, alpha, unk_score_offset):
        if not p or self.is_prefix(p):
            return 0.0
        return alpha * math.log(10) * unk_score_offset * max(1, len(p) / 6)


def final_total(lm, text, acoustic, alpha, beta, unk_score_offset, score_boundary):
    """The finished hypothesis' total from its text alone: acoustic + LM(text) + the </s> term."""
    s, ctx = lm.text_score(text, alpha, beta, unk_score_offset, score_boundary)
    return acoustic + s + lm.eos_term(ctx, alpha, score_boundary)


def _prune_rank(items, prune, limit, margin):
    """R._prune_rank on item[1], recording the smallest margin of a prune, rank or cut decision in margin[0].  One kind of
    decision is left out: two neighbours whose totals are equal AND whose parts (item[2][:3] minus the context: acoustic score,
    LM(text), partial score) are equal bit for bit.  The contract decides such a tie by candidate order, and an implementation
    that adds the same parts gets the same two totals whatever its rounding, so nothing hangs on a margin there.  bf16 inputs
    make these ties common (sums of few-bit numbers are exact in float64); any other tie counts as the margin 0 it is."""
    if not items:
        return []
    mx = max(it[1] for it in items)
    if prune > -INF:
        for it in items:
            margin[0] = min(margin[0], abs(it[1] - (mx + prune)))
    kept = [(i, it) for i, it in enumerate(items) if it[1] >= mx + prune]
    kept.sort(key=lambda x: (-x[1][1], x[0]))
    for a, b in zip(kept[:limit], kept[1:limit + 1]):           # the order of the survivors and the cut behind the last one
        if not (a[1][1] == b[1][1] and a[1][2][:3] == b[1][2][:3]):
            margin[0] = min(margin[0], a[1][1] - b[1][1])
    return [it for _, it in kept[:limit]]


def beam_search_lm(logp, n, vocab, lm, alpha=0.5, beta=1.5, unk_score_offset=-10.0, score_boundary=True, blank=0, beam_size=100,
                   beam_prune_logp=-10.0, token_prune_min_logp=-5.0, prune_history=False, blank_skip_threshold=1.0, topk=1,
                   space_token=" ", spm_token="▁"):
    """-> ([(text, acoustic score, total)] best first, smallest decision margin)."""
    cls = R.classify(vocab, blank, space_token, spm_token)
    skip_log = math.log(blank_skip_threshold)
    a = alpha * math.log(10)
    margin = [INF]
    beams = [("", "", None, 0.0, 0.0, lm.start(score_boundary), 0.0)]       # text, partial, last, acoustic, LM(text), context, partial score
    for t in range(n):
        row = [float(x) for x in logp[t]]
        if any(x != x for x in row):
            raise ValueError(f"NaN at frame {t}")
        if row[blank] > skip_log:
            continue
        amax = max(range(len(row)), key=lambda v: (row[v], -v))
        sel = [v for v in range(len(row)) if row[v] > token_prune_min_logp or v == amax]
        cands = []
        for v in sel:
            kind, clean = cls[v]
            for bi, (text, part, last, s, _, _, _) in enumerate(beams):
                commit = None
                if kind == "blank" or v == last:
                    nt, np_, same = text, part, True
                elif kind == "word":
                    nt, np_, same, commit = R._join(text, part), clean, False, part or None
                else:
                    nt, np_, same = text, part + clean, False
                cands.append(((nt, np_, v), s + row[v], (bi, same, commit)))
        items = []
        for key, ac, (bi, same, commit) in R._merge(cands):
            _, _, _, _, l, ctx, ps = beams[bi]
            if not same:
                if commit is not None:
                    lw, ctx = lm.step(ctx, commit, unk_score_offset)
                    l = l + (a * lw + beta)
                ps = lm.partial_score(key[1], alpha, unk_score_offset)
            items.append([key, ac + l + ps, (ac, l, ps, ctx)])
        ranked = _prune_rank(items, beam_prune_logp, beam_size, margin)
        beams = [(k[0], k[1], k[2], pay[0], pay[1], pay[3], pay[2]) for k, _, pay in ranked]
        if prune_history:
            seen, kept = set(), []
            for b in beams:
                h = (tuple(b[0].split()[-1:]), b[1], b[2])
                if h not in seen:
                    seen.add(h)
                    kept.append(b)
            beams = kept
    fin = []
    for text, part, _, s, l, ctx, _ in beams:
        if part:
            lw, ctx = lm.step(ctx, part, unk_score_offset)
            l = l + (a * lw + beta)
        fin.append((R._join(text, part), s, (l, ctx)))
    items = []
    for text, ac, (l, ctx) in R._merge(fin):
        total = ac + l
        if score_boundary and "</s>" in lm.vocab:
            total += a * lm.cond(ctx, "</s>")
        items.append([text, total, (ac, l, 0.0)])
    return [(text, pay[0], total) for text, total, pay in _prune_rank(items, beam_prune_logp, topk, margin)], margin[0]
