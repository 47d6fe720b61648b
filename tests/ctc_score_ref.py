"""References for the scoring contracts of DESIGN.md §4u, written from their text (helper of tests/test_ctc_score_cpu.py,
test_ctc_greedy_gpu.py, test_edit_distance_gpu.py and test_recipe_eval_{cpu,gpu}.py; not a test file).  Plain Python and NumPy, one
cell and one frame at a time, sharing no code with mamba_asr_amd.

greedy(lp, lengths, blank): per frame the lowest index attaining the maximum (-inf an ordinary value), a frame kept when its index is
not blank and differs from the previous frame's; spans and the float64 left fold of the kept token's own log-probabilities over its
run; a NaN in a frame < n gives status 2 and an empty row.
edit_ops(a, b): the full table D with the move rule (diagonal only when strictly below both others, else delete when strictly below
insert, else insert) and the backtrace from (R, H).  distance_two_rows(a, b): the classic two-row Levenshtein distance, no moves."""
import numpy as np


def greedy_one(lp, n, blank):
    """lp (T, V) float64 array -> (status, tokens, starts, ends, logp)."""
    best = []
    for t in range(n):
        row = lp[t]
        if np.isnan(row).any():
            return 2, [], [], [], []
        k = 0
        for v in range(1, len(row)):
            if row[v] > row[k]:
                k = v
        best.append(k)
    tokens, starts, ends, logp = [], [], [], []
    for t, k in enumerate(best):
        if k == blank:
            continue
        if t == 0 or k != best[t - 1]:
            tokens.append(k), starts.append(t), ends.append(t + 1), logp.append(np.float64(lp[t][k]))
        else:
            ends[-1] = t + 1
            logp[-1] = logp[-1] + np.float64(lp[t][k])
    return 0, tokens, starts, ends, logp


def greedy_one_fast(lp, n, blank):
    """greedy_one with the frame maxima found by NumPy (large V): the first index equal to the row's maximum; NaN is looked for first."""
    x = lp[:n]
    if np.isnan(x).any():
        return 2, [], [], [], []
    best = [int(np.flatnonzero(row == row.max())[0]) for row in x]
    tokens, starts, ends, logp = [], [], [], []
    for t, k in enumerate(best):
        if k == blank:
            continue
        if t == 0 or k != best[t - 1]:
            tokens.append(k), starts.append(t), ends.append(t + 1), logp.append(np.float64(x[t][k]))
        else:
            ends[-1] = t + 1
            logp[-1] = logp[-1] + np.float64(x[t][k])
    return 0, tokens, starts, ends, logp


def greedy_batch(lp, lengths, blank=0, fast=False):
    """lp (B, T, V) float64 -> (tokens, token_len, starts, ends, token_logp, status) as the kernel lays them out: (B, T) int32 rows
    padded with -1, token_logp (B, T) float64 padded with 0.0."""
    B, T, _ = lp.shape
    tokens, starts, ends = (np.full((B, T), -1, dtype=np.int32) for _ in range(3))
    logp = np.zeros((B, T), dtype=np.float64)
    token_len, status = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = max(min(int(lengths[b]), T), 0)
        st, tk, s, e, l = (greedy_one_fast if fast else greedy_one)(lp[b], n, blank)
        status[b], token_len[b] = st, len(tk)
        tokens[b, :len(tk)], starts[b, :len(tk)], ends[b, :len(tk)], logp[b, :len(tk)] = tk, s, e, l
    return tokens, token_len, starts, ends, logp, status


def edit_ops(a, b):
    """-> ([ins, del, sub, hits], D[R][H], path in forward order over '=', 'I', 'D', 'S')."""
    R, H = len(a), len(b)
    D = [[0] * (H + 1) for _ in range(R + 1)]
    M = [[""] * (H + 1) for _ in range(R + 1)]
    for i in range(R + 1):
        D[i][0] = i
    for j in range(H + 1):
        D[0][j] = j
    for i in range(1, R + 1):
        for j in range(1, H + 1):
            sub = D[i - 1][j - 1] + (1 if a[i - 1] != b[j - 1] else 0)
            dele = D[i - 1][j] + 1
            ins = D[i][j - 1] + 1
            if sub < ins and sub < dele:
                D[i][j], M[i][j] = sub, "diag"
            elif dele < ins:
                D[i][j], M[i][j] = dele, "del"
            else:
                D[i][j], M[i][j] = ins, "ins"
    i, j, path = R, H, []
    while i > 0 or j > 0:
        if i == 0:
            path.append("I")
            j -= 1
        elif j == 0:
            path.append("D")
            i -= 1
        elif M[i][j] == "diag":
            path.append("=" if a[i - 1] == b[j - 1] else "S")
            i, j = i - 1, j - 1
        elif M[i][j] == "del":
            path.append("D")
            i -= 1
        else:
            path.append("I")
            j -= 1
    path = "".join(reversed(path))
    return [path.count("I"), path.count("D"), path.count("S"), path.count("=")], D[R][H], path


def distance_two_rows(a, b):
    """Levenshtein distance by the textbook two-row recurrence with min(): no move table, no tie rule."""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (x != y), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[len(b)]


def replay(a, path):
    """Apply a path to the reference -> the hypothesis it describes, with None where the path inserts or substitutes (the caller
    fills those from the hypothesis); also checks that the path consumes the reference exactly."""
    out, i = [], 0
    for op in path:
        if op == "=":
            out.append(a[i])
            i += 1
        elif op == "S":
            out.append(None)
            i += 1
        elif op == "D":
            i += 1
        else:
            assert op == "I", op
            out.append(None)
    assert i == len(a), (i, len(a))
    return out


def check_invariants(a, b, counts, dist, path):
    """What must hold whatever the tie rule chose."""
    ins, dele, sub, hits = counts
    assert ins + dele + sub == dist == distance_two_rows(a, b), (counts, dist, distance_two_rows(a, b))
    assert len(a) == hits + sub + dele and len(b) == hits + sub + ins, (len(a), len(b), counts)
    assert [path.count(c) for c in "IDS="] == list(counts), (path, counts)
    got = replay(a, path)
    assert len(got) == len(b) and all(g is None or g == h for g, h in zip(got, b)), (a, b, path)
    j = 0
    for op, g in zip([o for o in path if o != "D"], got):              # a substitution changes the token, a hit keeps it
        assert (g is None) == (op in "SI")
        if op == "S":
            k = sum(1 for o in path[:_nth(path, j)] if o != "I")
            assert a[k] != b[j], (a, b, path, j)
        j += 1


def _nth(path, j):
    """Index in path of the step that emits hypothesis token j."""
    seen = -1
    for k, o in enumerate(path):
        if o != "D":
            seen += 1
            if seen == j:
                return k
    raise AssertionError((path, j))


def error_rates(refs, hyps):
    """Token lists -> (WER percent, [ins, del, sub], reference tokens) by edit_ops, summed over the pairs."""
    tot, n = [0, 0, 0], 0
    for a, b in zip(refs, hyps):
        c = edit_ops(a, b)[0]
        tot = [x + y for x, y in zip(tot, c[:3])]
        n += len(a)
    return (100.0 * sum(tot) / n if n else 0.0), tot, n
