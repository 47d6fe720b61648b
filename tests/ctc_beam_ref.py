"""Float64 pure-Python restatement of the LM-free CTC beam search contract (mamba_asr_amd/ctc_decode.py),
written for the tests: nothing here is imported from the package."""
import math


def _lae(a, b):
    if a == -math.inf and b == -math.inf:
        return -math.inf
    return max(a, b) + math.log1p(math.exp(-abs(a - b)))


def _join(a, b):
    return a if not b else (b if not a else a + " " + b)


def classify(vocab, blank, space_token=" ", spm_token="▁"):
    """-> per token ("blank" | "word" | "char", clean part)."""
    spm = any(p.startswith(spm_token) for p in vocab)
    out = []
    for v, p in enumerate(vocab):
        if v == blank:
            out.append(("blank", ""))
        elif spm and p.startswith(spm_token):
            out.append(("word", p[len(spm_token):]))
        elif not spm and p == space_token:
            out.append(("word", ""))
        else:
            out.append(("char", p))
    return out


def _merge(cands):
    """[(key, score, payload)] in candidate order -> merged list in first-occurrence order, scores folded left."""
    pos, out = {}, []
    for key, s, pay in cands:
        if key in pos:
            k = pos[key]
            out[k][1] = _lae(out[k][1], s)
        else:
            pos[key] = len(out)
            out.append([key, s, pay])
    return out


def _prune_rank(items, prune, limit):
    if not items:
        return []
    mx = max(it[1] for it in items)
    kept = [(i, it) for i, it in enumerate(items) if it[1] >= mx + prune]
    kept.sort(key=lambda x: (-x[1][1], x[0]))
    return [it for _, it in kept[:limit]]


def beam_search(logp, n, vocab, blank=0, beam_size=100, beam_prune_logp=-10.0, token_prune_min_logp=-5.0,
                prune_history=False, blank_skip_threshold=1.0, topk=1, space_token=" ", spm_token="▁"):
    """logp: (T, V) rows of floats (any sequence); n frames decoded -> [(text, score)] best first."""
    cls = classify(vocab, blank, space_token, spm_token)
    skip_log = math.log(blank_skip_threshold)
    beams = [("", "", None, 0.0)]
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
            for text, part, last, s in beams:
                if kind == "blank" or v == last:
                    nt, np_ = text, part
                elif kind == "word":
                    nt, np_ = _join(text, part), clean
                else:
                    nt, np_ = text, part + clean
                cands.append(((nt, np_, v), s + row[v], None))
        ranked = _prune_rank(_merge(cands), beam_prune_logp, beam_size)
        beams = [(k[0], k[1], k[2], s) for k, s, _ in ranked]
        if prune_history:
            seen, kept = set(), []
            for b in beams:
                h = (tuple(b[0].split()[-1:]), b[1], b[2])
                if h not in seen:
                    seen.add(h)
                    kept.append(b)
            beams = kept
    fin = _merge([(_join(text, part), s, None) for text, part, _, s in beams])
    return [(k, s) for k, s, _ in _prune_rank(fin, beam_prune_logp, topk)]


def brute_force(logp, vocab, blank=0, space_token=" ", spm_token="▁"):
    """All V^T alignments of the full (T, V) matrix -> {text: logsumexp of alignment scores}, text by the same class rules."""
    import itertools
    cls = classify(vocab, blank, space_token, spm_token)
    T, V = len(logp), len(logp[0])
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        text, part, last, s = "", "", None, 0.0
        for t, v in enumerate(path):
            s += float(logp[t][v])
            kind, clean = cls[v]
            if not (kind == "blank" or v == last):
                if kind == "word":
                    text, part = _join(text, part), clean
                else:
                    part += clean
            last = v
        key = _join(text, part)
        acc.setdefault(key, []).append(s)
    out = {}
    for k, ss in acc.items():
        m = max(ss)
        out[k] = m + math.log(math.fsum(math.exp(x - m) for x in ss)) if m > -math.inf else m
    return out
