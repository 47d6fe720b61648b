"""The CTC prefix-score contract restated in NumPy; the working dtype is a parameter, so the same code runs in
fp64 (the oracle) and in fp32 (whose distance from fp64 sets the kernels' tolerance).

State of a prefix g on n frames of one utterance's log-posteriors lp (n, V):
  r_n[t] / r_b[t]  log-probability that frames 0..t emit exactly g and end in a non-blank / in a blank
  psi_g            log prefix probability of g;   last: g's last token, -1 when g is empty.
"""
import numpy as np
import torch

NEG = -np.inf


def lae(a, b):
    """max + log1p(exp(-|a - b|)), lae(-inf, -inf) = -inf; element-wise, in the operands' dtype."""
    a, b = np.asarray(a), np.asarray(b)
    m = np.maximum(a, b)
    with np.errstate(invalid="ignore"):
        d = -np.abs(a - b)
    d = np.where(np.isnan(d), 0, d).astype(m.dtype)
    return np.where(m == NEG, m, m + np.log1p(np.exp(d))).astype(m.dtype)


def lse0(x):
    """log-sum-exp over axis 0 with a maximum shift; -inf where every term is -inf (and for no terms at all)."""
    if x.shape[0] == 0:
        return np.full(x.shape[1:], NEG, dtype=x.dtype)
    m = x.max(axis=0)
    safe = np.where(m == NEG, 0, m).astype(x.dtype)
    with np.errstate(divide="ignore"):
        return np.where(m == NEG, NEG, safe + np.log(np.exp(x - safe).sum(axis=0, dtype=x.dtype))).astype(x.dtype)


def initial(lp, blank):
    """-> (r_n, r_b, psi_g, last) of the empty prefix."""
    n = lp.shape[0]
    return np.full(n, NEG, dtype=lp.dtype), np.cumsum(lp[:, blank], dtype=lp.dtype), lp.dtype.type(0), -1


def psi_all(lp, state, blank):
    """-> (psi (V,) of g + c for every token c, psi[blank] = -inf;  psi_eos = log p(collapsed sequence == g))."""
    r_n, r_b, _, last = state
    n, V = lp.shape
    both = lae(r_n, r_b)
    phi = np.repeat(both[:n - 1, None], V, axis=1)
    if last >= 0:
        phi[:, last] = r_b[:n - 1]
    psi = lse0(phi + lp[1:n])
    if last < 0:
        psi = lae(psi, lp[0])
    psi[blank] = NEG
    return psi, lae(r_n[n - 1], r_b[n - 1])


def advance(lp, state, c, blank):
    """-> the state of g + c (c a non-blank token)."""
    r_n, r_b, _, last = state
    n = lp.shape[0]
    both = lae(r_n, r_b)
    phi = r_b if c == last else both
    psi = psi_all(lp, state, blank)[0][c]
    new_n, new_b = np.full(n, NEG, dtype=lp.dtype), np.full(n, NEG, dtype=lp.dtype)
    if last < 0:
        new_n[0] = lp[0, c]
    for t in range(1, n):
        new_n[t] = lae(new_n[t - 1], phi[t - 1]) + lp[t, c]
        new_b[t] = lae(new_n[t - 1], new_b[t - 1]) + lp[t, blank]
    return new_n, new_b, psi, int(c)


class RefCTCPrefixScorer:
    """The four methods of mamba_asr_amd.s2s_decode.CTCPrefixScorer on the host.  A state is a dict: lp (per utterance, cut to
    its n frames), row_utt and rows (per row: (r_n, r_b, psi_g, last))."""

    def __init__(self, blank_index, eos_index, dtype=np.float64):
        self.blank, self.eos, self.dtype = int(blank_index), int(eos_index), dtype

    def init(self, logp, enc_lens, row_utt=None):
        logp = logp.detach().cpu().numpy()
        T = logp.shape[1]
        n_u = [min(max(int(round(float(x))), 1), T) for x in enc_lens]
        lp = [logp[u, :n].astype(self.dtype) for u, n in enumerate(n_u)]
        row_utt = list(range(len(lp))) if row_utt is None else [int(u) for u in row_utt]
        return {"lp": lp, "row_utt": row_utt, "rows": [initial(lp[u], self.blank) for u in row_utt]}

    def score(self, state, candidates=None):
        out = []
        for u, st in zip(state["row_utt"], state["rows"]):
            psi, psi_eos = psi_all(state["lp"][u], st, self.blank)
            psi[self.eos] = psi_eos
            with np.errstate(invalid="ignore"):
                out.append(np.where(psi == NEG, NEG, psi - st[2]))
        out = torch.from_numpy(np.stack(out))
        if candidates is not None:
            cand = candidates.long().cpu()
            ok = (cand >= 0) & (cand < out.shape[1])
            out = torch.where(ok, out.gather(1, cand.clamp(0, out.shape[1] - 1)), torch.full((), NEG, dtype=out.dtype))
        return out

    def advance(self, state, tokens):
        rows = [st if int(c) == self.eos else advance(state["lp"][u], st, int(c), self.blank)
                for u, st, c in zip(state["row_utt"], state["rows"], tokens.tolist())]
        return {"lp": state["lp"], "row_utt": state["row_utt"], "rows": rows}

    def reorder(self, state, index):
        index = [int(i) for i in index]
        return {"lp": state["lp"], "row_utt": [state["row_utt"][i] for i in index], "rows": [state["rows"][i] for i in index]}


def padded(state, T):
    """-> (r_n (rows, T), r_b (rows, T), psi_g (rows), last (rows)) as arrays; frames past a row's n are NaN (not compared)."""
    rows = state["rows"]
    r_n, r_b = np.full((len(rows), T), np.nan), np.full((len(rows), T), np.nan)
    for i, st in enumerate(rows):
        r_n[i, :len(st[0])], r_b[i, :len(st[1])] = st[0], st[1]
    return r_n, r_b, np.array([float(st[2]) for st in rows]), np.array([st[3] for st in rows])
