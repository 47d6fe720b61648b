"""The CTC forced-alignment contract (mamba_asr_amd/ctc_decode.py) in NumPy float64: what cm_ctc_align must return,
bit for bit.  Vectorised over the states with np.where and strict >; Python loops over t only.  Plain module (as
tests/ctc_beam_ref.py)."""
import numpy as np

NEG = -np.inf


def align_one(lp, target, blank):
    """lp (n, V) float array (any float dtype: converted exactly), target a sequence of L ids
    -> (status, score, states (n) int32 or None, starts (L), ends (L), label_logp (L)); the per-label outputs are None unless
    status == 0."""
    lp = np.asarray(lp, dtype=np.float64)
    n, V = lp.shape
    y = np.asarray(target, dtype=np.int64).reshape(-1)
    L = y.shape[0]
    E = 2 * L + 1
    if n == 0:
        if L == 0:
            return 0, 0.0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
        return 1, NEG, None, None, None, None
    e = np.full(E, blank, dtype=np.int64)
    e[1::2] = y
    ok = (e >= 0) & (e < V)                                   # an id outside the vocabulary scores -inf
    x = np.where(ok[None, :], lp[:, np.where(ok, e, 0)], NEG)  # (n, E)
    s = np.arange(E)
    skip = (s % 2 == 1) & (s >= 3)
    skip[3:] &= e[3:] != e[1:-2]
    D = np.full(E, NEG)
    D[:2] = x[0, :2]
    moves = np.zeros((n, E), dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for t in range(1, n):
            c1 = np.concatenate(([NEG], D[:-1]))[:E]
            c2 = np.where(skip, np.concatenate(([NEG, NEG], D[:-2]))[:E], NEG)
            best, mv = D, np.zeros(E, dtype=np.int8)
            g = c1 > best
            best, mv = np.where(g, c1, best), np.where(g, 1, mv)
            g = skip & (c2 > best)
            best, mv = np.where(g, c2, best), np.where(g, 2, mv)
            D = best + x[t]
            moves[t] = mv
        sE = E - 1
        if E >= 2 and D[E - 2] > D[E - 1]:
            sE = E - 2
    score = D[sE]
    if np.isnan(x).any() or np.isnan(score):
        return 2, np.nan, None, None, None, None
    if score == NEG:
        return 1, NEG, None, None, None, None
    states = np.zeros(n, dtype=np.int32)
    st = sE
    for t in range(n - 1, -1, -1):
        states[t] = st
        st -= int(moves[t, st])
    starts, ends, logp = np.full(L, -1, np.int32), np.full(L, -1, np.int32), np.zeros(L, np.float64)
    for j in range(L):
        ts = np.nonzero(states == 2 * j + 1)[0]
        starts[j], ends[j] = ts[0], ts[-1] + 1
        acc = x[ts[0], 2 * j + 1]
        for t in ts[1:]:
            acc = acc + x[t, 2 * j + 1]                        # the left fold, in increasing t
        logp[j] = acc
    return 0, float(score), states, starts, ends, logp


def align_batch(lp, targets, input_lengths, target_lengths, blank=0, rows=None):
    """The six outputs of ops.ctc_align as NumPy arrays: lp (R, T, V), targets (B, S)."""
    lp, targets = np.asarray(lp), np.asarray(targets)
    B, S = targets.shape
    T = lp.shape[1]
    score, status = np.zeros(B, np.float64), np.zeros(B, np.int32)
    states = np.full((B, T), -1, np.int32)
    starts, ends, logp = np.full((B, S), -1, np.int32), np.full((B, S), -1, np.int32), np.zeros((B, S), np.float64)
    for b in range(B):
        n, L = max(min(int(input_lengths[b]), T), 0), max(min(int(target_lengths[b]), S), 0)
        r = b if rows is None else int(rows[b])
        st, sc, ss, a, z, lg = align_one(lp[r, :n], targets[b, :L], blank)
        status[b], score[b] = st, sc
        if st == 0:
            states[b, :n], starts[b, :L], ends[b, :L], logp[b, :L] = ss, a, z, lg
    return score, status, states, starts, ends, logp
