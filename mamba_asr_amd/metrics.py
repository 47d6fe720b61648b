"""Scoring transcripts: word / character error rate with alignments (ErrorRateStats) and token accuracy (AccuracyStats) -- what the
recipes bind as speechbrain.utils.metric_stats.ErrorRateStats (`wer_computer`, `cer_computer`, `error_rate_computer`; reference
train_CTC.py:407-420 append, :625-626 summarize("error_rate"), write_stats at test time) and speechbrain.utils.Accuracy.AccuracyStats
(`acc_computer`).  speechbrain cannot be installed here, so parity with its insertion / deletion / substitution split is not pinned:
the rules below are the contract, and only the total number of edits is independent of the tie rule.

Edit distance (ops.edit_distance, csrc/edit_distance.hip on the GPU; edit_ops_host here, the same bits).  For a
reference a of R tokens and a hypothesis b of H tokens:
  D[i][0] = i;  D[0][j] = j;  sub = D[i-1][j-1] + (a[i-1] != b[j-1]);  del = D[i-1][j] + 1;  ins = D[i][j-1] + 1;
  the move of cell (i, j) is diagonal if sub < ins and sub < del, otherwise delete if del < ins, otherwise insert, and D[i][j] is
  that move's value: a substitution must win strictly, insertion wins the remaining ties.
Backtrace from (R, H): diagonal goes to (i-1, j-1) and is a hit when the tokens are equal, a substitution otherwise; delete goes to
(i-1, j); insert goes to (i, j-1); row 0 is all inserts, column 0 all deletes.  The path in forward order is a string over
'=' (hit), 'S', 'D', 'I'; counts are [ins, del, sub, hits]; dist = D[R][H] = ins + del + sub.  All arithmetic is integer.
WER = 100 (I + D + S) / reference tokens; without any reference token it is 0.0 when there are no edits either (nothing appended,
or empty against empty) and 100.0 when only insertions were scored.  SER = the percentage of utterances with at least one edit.
The GPU kernel takes sequences of up to CM_EDIT_MAX_LEN (1024) tokens; longer pairs, and everything when ``device`` is not a
GPU, are scored by edit_ops_host with identical results.

write_stats format (this project's own):
  %WER 12.50 [ 2 / 16, 1 ins, 0 del, 1 sub ]
  %SER 50.00 [ 1 / 2 ]
  <blank line>
then per utterance, in the order appended,
  <id>, %WER 25.00 [ 2 / 8, 1 ins, 0 del, 1 sub ]
  ref: the three rows of the alignment, one column per path step, columns separated by " ; " and padded to equal width:
  op :   the reference token (<eps> under an insertion), the operation (= S I D), the hypothesis token (<eps> under a deletion)
  hyp:
  <blank line>
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import torch

EPS = "<eps>"


def edit_ops_host(a: Sequence, b: Sequence):
    """The module docstring's recurrence and backtrace on the host, for any comparable tokens -> ([ins, del, sub, hits], dist, ops)."""
    R, H = len(a), len(b)
    prev = list(range(H + 1))
    moves = []
    for i in range(1, R + 1):
        cur, row, ai = [i] + [0] * H, bytearray(H + 1), a[i - 1]
        for j in range(1, H + 1):
            ne = ai != b[j - 1]
            sub, dele, ins = prev[j - 1] + ne, prev[j] + 1, cur[j - 1] + 1
            if sub < ins and sub < dele:
                cur[j], row[j] = sub, 1 if ne else 0
            elif dele < ins:
                cur[j], row[j] = dele, 2
            else:
                cur[j], row[j] = ins, 3
        moves.append(row)
        prev = cur
    dist = prev[H]
    i, j, back = R, H, []
    while i > 0 and j > 0:
        mv = moves[i - 1][j]
        back.append("=SDI"[mv])
        i, j = i - (mv != 3), j - (mv != 2)
    back.extend("D" * i + "I" * j)
    ops = "".join(reversed(back))
    return [ops.count("I"), ops.count("D"), ops.count("S"), ops.count("=")], dist, ops


def score_pairs(refs: List[List[int]], hyps: List[List[int]], ref_index: Optional[List[int]] = None, device=None):
    """Pairs (refs[ref_index[p]], hyps[p]) of integer sequences -> [([ins, del, sub, hits], ops)] per pair.  ``device`` a GPU: one
    ops.edit_distance launch for every pair within CM_EDIT_MAX_LEN; the rest, and everything without a GPU device, on the host."""
    ref_index = list(range(len(hyps))) if ref_index is None else list(ref_index)
    out: List = [None] * len(hyps)
    native = []
    if device is not None and torch.device(device).type == "cuda" and hyps:
        from . import _native as N
        cap = N.CM_EDIT_MAX_LEN
        native = [p for p in range(len(hyps)) if len(hyps[p]) <= cap and len(refs[ref_index[p]]) <= cap]
    if native:
        from . import ops
        used = sorted({ref_index[p] for p in native})
        slot = {r: k for k, r in enumerate(used)}
        sr, sh = max(len(refs[r]) for r in used), max(len(hyps[p]) for p in native)
        rt = torch.tensor([refs[r] + [0] * (sr - len(refs[r])) for r in used], dtype=torch.int32).reshape(len(used), sr)
        ht = torch.tensor([hyps[p] + [0] * (sh - len(hyps[p])) for p in native], dtype=torch.int32).reshape(len(native), sh)
        rl, hl = torch.tensor([len(refs[r]) for r in used], dtype=torch.int32), torch.tensor([len(hyps[p]) for p in native], dtype=torch.int32)
        ri = torch.tensor([slot[ref_index[p]] for p in native], dtype=torch.int32)
        counts, _, _, path, n_ops = ops.edit_distance(*(t.to(device) for t in (rt, rl, ht, hl, ri)), want_ops=True)
        counts, path, n_ops = counts.cpu().tolist(), path.cpu().numpy().astype("uint8"), n_ops.cpu().tolist()
        for k, p in enumerate(native):
            out[p] = (counts[k], path[k, :n_ops[k]].tobytes().decode("ascii"))
    for p in range(len(hyps)):
        if out[p] is None:
            c, _, path = edit_ops_host(refs[ref_index[p]], hyps[p])
            out[p] = (c, path)
    return out


def _trim(x, rel):
    """A padded batch (tensor or list of sequences) with optional relative lengths -> a list of lists."""
    if isinstance(x, torch.Tensor):
        rows = x.detach().cpu().tolist()
        if rel is not None:
            steps = x.shape[1]
            rel = rel.detach().cpu().tolist() if isinstance(rel, torch.Tensor) else list(rel)
            rows = [row[:int(round(r * steps))] for row, r in zip(rows, rel)]
        return rows
    return [list(row) for row in x]


class ErrorRateStats:
    """Word error rate with alignments (constructor and methods of speechbrain's ErrorRateStats as the recipes use them).

    merge_tokens: the tokens of a sequence are concatenated and split again at ``space_token`` (characters -> words).  split_tokens:
    the tokens are joined by ``space_token`` and scored character by character (CER).  device: a GPU device scores every append in
    one ops.edit_distance launch; None or a CPU device scores on the host -- the same numbers either way."""

    def __init__(self, merge_tokens: bool = False, split_tokens: bool = False, space_token: str = "_", device=None):
        self.merge_tokens, self.split_tokens, self.space_token, self.device = bool(merge_tokens), bool(split_tokens), space_token, device
        self.clear()

    def clear(self):
        self.ids, self.scores = [], []

    def _tokens(self, seq):
        seq = [str(t) if self.merge_tokens or self.split_tokens else t for t in seq]
        if self.merge_tokens:
            seq = [w for w in "".join(seq).split(self.space_token) if w]
        if self.split_tokens:
            seq = list(self.space_token.join(seq))
        return seq

    def _prepare(self, batch, rel, ind2lab):
        rows = _trim(batch, rel)
        if ind2lab is not None:
            rows = ind2lab(rows) if callable(ind2lab) else [[ind2lab[int(t)] for t in row] for row in rows]
        return [self._tokens(row) for row in rows]

    def _score(self, refs, hyps, ref_index=None):
        """Token lists -> one record per hypothesis; the labels are interned to int32 for this call."""
        table = {}
        intern = lambda seq: [table.setdefault(t, len(table)) for t in seq]
        ri = list(range(len(hyps))) if ref_index is None else ref_index
        scored = score_pairs([intern(r) for r in refs], [intern(h) for h in hyps], ri, self.device)
        return [{"insertions": c[0], "deletions": c[1], "substitutions": c[2], "hits": c[3], "num_edits": c[0] + c[1] + c[2],
                 "num_ref_tokens": len(refs[ri[p]]), "num_hyp_tokens": len(hyps[p]), "ops": path, "ref_tokens": list(refs[ri[p]]),
                 "hyp_tokens": list(hyps[p])} for p, (c, path) in enumerate(scored)]

    def append(self, ids, predict, target, predict_len=None, target_len=None, ind2lab: Optional[Callable] = None):
        """ids: one key per utterance; predict / target: lists of token lists (words), or padded id tensors trimmed by the relative
        predict_len / target_len; ind2lab: a callable over the batch of id lists, or a mapping per id, applied first."""
        hyps, refs = self._prepare(predict, predict_len, ind2lab), self._prepare(target, target_len, ind2lab)
        ids = list(ids)
        if not len(ids) == len(hyps) == len(refs):
            raise ValueError(f"ErrorRateStats.append: {len(ids)} ids, {len(hyps)} predictions and {len(refs)} targets")
        for key, rec in zip(ids, self._score(refs, hyps)):
            rec["key"] = key
            self.ids.append(key)
            self.scores.append(rec)

    def extend(self, records):
        """Accumulate records scored elsewhere (oracle()'s)."""
        for rec in records:
            self.ids.append(rec["key"])
            self.scores.append(rec)

    def oracle(self, ids, nbest, target, ind2lab: Optional[Callable] = None):
        """nbest: per utterance a list of hypothesis token lists; all of them are scored against the utterance's target in one launch
        (they share the reference through ref_index).  -> per utterance the record of the hypothesis with the fewest edits, the first
        on ties, with "best_index"; nothing is accumulated here: a second ErrorRateStats takes them through extend()."""
        refs = self._prepare(target, None, ind2lab)
        flat, ri = [], []
        for u, hyps in enumerate(nbest):
            rows = self._prepare(hyps, None, ind2lab)
            flat.extend(rows)
            ri.extend([u] * len(rows))
        recs = self._score(refs, flat, ri) if flat else []
        out, pos = [], 0
        for u, (key, hyps) in enumerate(zip(ids, nbest)):
            mine = recs[pos:pos + len(hyps)]
            pos += len(hyps)
            if not mine:
                raise ValueError(f"ErrorRateStats.oracle: utterance {key!r} has no hypotheses")
            k = min(range(len(mine)), key=lambda h: (mine[h]["num_edits"], h))
            out.append(dict(mine[k], key=key, best_index=k))
        return out

    def summarize(self, field=None):
        s = self.scores
        tot = {k: sum(r[k] for r in s) for k in ("insertions", "deletions", "substitutions", "num_edits", "num_ref_tokens", "num_hyp_tokens")}
        bad = sum(1 for r in s if r["num_edits"])
        wer = 100.0 * tot["num_edits"] / tot["num_ref_tokens"] if tot["num_ref_tokens"] else (100.0 if tot["num_edits"] else 0.0)
        self.summary = {"WER": wer, "error_rate": wer, "SER": 100.0 * bad / len(s) if s else 0.0, "insertions": tot["insertions"],
                        "deletions": tot["deletions"], "substitutions": tot["substitutions"], "num_edits": tot["num_edits"],
                        "num_scored_tokens": tot["num_ref_tokens"], "num_ref_tokens": tot["num_ref_tokens"],
                        "num_hyp_tokens": tot["num_hyp_tokens"], "num_scored_sents": len(s), "num_erroneous_sents": bad}
        return self.summary if field is None else self.summary[field]

    def write_stats(self, filestream):
        """The module docstring's format."""
        m = self.summarize()
        filestream.write(f"%WER {m['WER']:.2f} [ {m['num_edits']} / {m['num_scored_tokens']}, {m['insertions']} ins, {m['deletions']} del, "
                         f"{m['substitutions']} sub ]\n")
        filestream.write(f"%SER {m['SER']:.2f} [ {m['num_erroneous_sents']} / {m['num_scored_sents']} ]\n\n")
        for r in self.scores:
            n = r["num_ref_tokens"]
            wer = 100.0 * r["num_edits"] / n if n else (100.0 if r["num_edits"] else 0.0)
            filestream.write(f"{r['key']}, %WER {wer:.2f} [ {r['num_edits']} / {n}, {r['insertions']} ins, {r['deletions']} del, "
                             f"{r['substitutions']} sub ]\n")
            i = j = 0
            cols = []
            for op in r["ops"]:
                a = str(r["ref_tokens"][i]) if op != "I" else EPS
                b = str(r["hyp_tokens"][j]) if op != "D" else EPS
                i, j = i + (op != "I"), j + (op != "D")
                w = max(len(a), len(b), 1)
                cols.append((a.ljust(w), op.ljust(w), b.ljust(w)))
            for name, k in (("ref", 0), ("op ", 1), ("hyp", 2)):
                filestream.write(f"{name}: " + " ; ".join(c[k] for c in cols).rstrip() + "\n")
            filestream.write("\n")


class AccuracyStats:
    """Token accuracy of arg-max predictions (speechbrain.utils.Accuracy.AccuracyStats as the S2S recipes use it).  Plain torch."""

    def __init__(self):
        self.correct, self.total = 0, 0

    def append(self, log_probs, targets, length=None):
        """log_probs (batch, steps, classes), targets (batch, steps), length (batch) relative or None: positions at and past
        round(length * steps) are padding and count nowhere."""
        if log_probs.dim() == 2:
            log_probs, targets = log_probs.unsqueeze(1), targets.reshape(-1, 1)
        steps = targets.shape[1]
        hit = log_probs.detach().argmax(dim=-1) == targets.detach().to(log_probs.device)
        if length is None:
            mask = torch.ones_like(hit)
        else:
            n = torch.round(length.detach().to(hit.device).double() * steps).long()
            mask = torch.arange(steps, device=hit.device)[None, :] < n[:, None]
        self.correct += int((hit & mask).sum())
        self.total += int(mask.sum())

    def summarize(self) -> float:
        return self.correct / self.total if self.total else 0.0
