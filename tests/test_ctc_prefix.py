"""CTC prefix scoring for joint CTC/attention S2S decoding, the parts that need no GPU:

  * the contract's restatement (tests/ctc_prefix_ref.py) against enumeration of all V^n alignments and against F.ctc_loss
  * S2SGreedySearcher's joint decoding on scripted tables, the restatement injected as ``ctc_scorer``
  * argument validation of cm_ctc_prefix_score / cm_ctc_prefix_advance, their place in the header, the ABI version
"""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_prefix_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = -math.inf


# ----------------------------------------------------------------------------------------------------------
# the restatement is the contract
# ----------------------------------------------------------------------------------------------------------
def _collapse(path, blank=0):
    out, prev = [], None
    for s in path:
        if s != prev and s != blank:
            out.append(s)
        prev = s
    return tuple(out)


def _enumerate(lp):
    """-> {collapsed label sequence: summed probability} over all V^n alignments."""
    n, V = lp.shape
    table = {}
    for path in itertools.product(range(V), repeat=n):
        p = math.exp(sum(lp[t, s] for t, s in enumerate(path)))
        key = _collapse(path)
        table[key] = table.get(key, 0.0) + p
    return table


def _log(p):
    return math.log(p) if p > 0 else NEG


def _state_of(lp, prefix):
    st = R.initial(lp, 0)
    for c in prefix:
        st = R.advance(lp, st, c, 0)
    return st


@pytest.mark.parametrize("n", [1, 2, 5, 6])
def test_restatement_matches_enumeration_of_all_alignments(n):
    V = 4
    rng = np.random.default_rng(100 + n)
    lp = np.log(rng.dirichlet(np.ones(V), size=n))
    table = _enumerate(lp)
    worst = 0.0
    for g in [(), (1,), (1, 1), (2, 3), (3, 3, 1), (1, 2, 1, 2)]:
        st = _state_of(lp, g)
        psi, psi_eos = R.psi_all(lp, st, 0)
        want_g = _log(sum(p for k, p in table.items() if k[:len(g)] == g))
        want_eos = _log(table.get(g, 0.0))
        for got, want in [(float(st[2]), want_g), (float(psi_eos), want_eos)] + \
                [(float(psi[c]), _log(sum(p for k, p in table.items() if k[:len(g) + 1] == g + (c,)))) for c in range(1, V)]:
            if want == NEG:
                assert got == NEG, (g, got)
            else:
                assert abs(got - want) < 1e-12, (g, got, want)
                worst = max(worst, abs(got - want))
        assert psi[0] == NEG
        assert not np.isnan(psi).any() and not np.isnan(st[0]).any() and not np.isnan(st[1]).any()
    print(f"n={n}: max|restatement - enumeration| {worst:.2e}")


def test_restatement_eos_score_is_minus_ctc_loss():
    T, V = 20, 9
    gen = torch.Generator().manual_seed(5)
    logp = torch.log_softmax(torch.randn(2, T, V, generator=gen, dtype=torch.float64) * 2, dim=-1)
    lens = [20, 13]
    targets = [[3, 3, 5, 1, 8, 8, 2], [4, 7, 7]]
    scorer = R.RefCTCPrefixScorer(0, V, np.float64)          # <eos> outside the CTC vocabulary: read psi_eos directly
    for u in range(2):
        lp = logp[u, :lens[u]].numpy()
        st = _state_of(lp, targets[u])
        got = float(R.psi_all(lp, st, 0)[1])
        want = -float(F.ctc_loss(logp[u:u + 1].transpose(0, 1), torch.tensor([targets[u]]), torch.tensor([lens[u]]),
                                 torch.tensor([len(targets[u])]), blank=0, reduction="sum"))
        assert abs(got - want) < 1e-10, (got, want)
    assert scorer.eos == V


def test_restatement_scorer_deltas_and_impossible_prefix():
    """The scorer's view: delta = psi(c) - psi_g, <eos> column, candidates, reorder; a prefix longer than its utterance is
    impossible: every delta -inf, no NaN."""
    V, EOS = 5, 2
    gen = torch.Generator().manual_seed(8)
    logp = torch.log_softmax(torch.randn(2, 4, V, generator=gen), dim=-1)
    s = R.RefCTCPrefixScorer(0, EOS)
    st = s.init(logp, torch.tensor([4.0, 1.0]), row_utt=[0, 1, 0])
    d0 = s.score(st)
    assert d0.shape == (3, V) and bool((d0[:, 0] == NEG).all()) and torch.equal(d0[0], d0[2])
    st = s.advance(st, torch.tensor([3, 3, 4]))
    st = s.advance(st, torch.tensor([4, 4, EOS]))
    d = s.score(st)
    assert not torch.isnan(d).any() and bool((d[1] == NEG).all())        # one frame cannot hold two tokens
    assert st["rows"][2][3] == 4 and st["rows"][0][3] == 4                 # row 2 was advanced by <eos>: it kept (4,)
    cand = torch.tensor([[3, 3, 7], [1, 2, 3], [-1, 4, 0]])
    dc = s.score(st, cand)
    assert torch.equal(dc[0, :2], d[0, [3, 3]]) and dc[0, 2] == NEG and dc[2, 0] == NEG and dc[2, 1] == d[2, 4]
    moved = s.reorder(st, [2, 0])
    assert moved["row_utt"] == [0, 0] and torch.equal(s.score(moved), d[[2, 0]])


# ----------------------------------------------------------------------------------------------------------
# the searcher's joint decoding on scripted tables
# ----------------------------------------------------------------------------------------------------------
BLANK, BOS, EOS, V = 0, 1, 2, 6


def _att_table(rows):
    """rows[t][b] = the decoder's winner at step t for row b: log 0.5 for it, log 0.2 for <eos> (unless it wins), the rest
    share what is left (tests/test_s2s_decode.py `_table`)."""
    steps, batch = len(rows), len(rows[0])
    p = torch.full((steps, batch, V), 0.3 / (V - 2))
    for t in range(steps):
        for b in range(batch):
            p[t, b, EOS] = 0.2
            if rows[t][b] == EOS:
                p[t, b] = 0.5 / (V - 1)
            p[t, b, rows[t][b]] = 0.5
    return torch.log(p)


def _ctc_table(frames):
    """frames[b][t] = the CTC head's winner at frame t of row b (probability 0.9, the others 0.02 each)."""
    p = torch.full((len(frames), len(frames[0]), V), 0.02)
    for b, row in enumerate(frames):
        for t, c in enumerate(row):
            p[b, t, c] = 0.9
    return torch.log(p)


def _searcher(table, ctc=None, **kw):
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher

    def init_fn(enc):
        return {"t": 0}

    def step_fn(tokens, state):
        lp = table[state["t"]]
        state["t"] += 1
        return lp, state

    if ctc is not None:
        kw.update(ctc_scorer=R.RefCTCPrefixScorer(BLANK, EOS), ctc_fn=lambda enc: ctc)
    return S2SGreedySearcher(bos_index=BOS, eos_index=EOS, step_fn=step_fn, init_fn=init_fn, **kw)


def _walk(table, ctc, enc_lens, hyps_with_eos, weight):
    """The joint value of every chosen token, from the restatement stepped along the given sequences."""
    s = R.RefCTCPrefixScorer(BLANK, EOS)
    out = []
    for b, seq in enumerate(hyps_with_eos):
        st = s.init(ctc[b:b + 1], [enc_lens[b]])
        vals = []
        for t, c in enumerate(seq):
            vals.append(float(table[t, b, c]) + weight * float(s.score(st)[0, c]))
            st = s.advance(st, torch.tensor([c]))
        out.append(vals)
    return out


ATT = [[3, 3], [4, EOS], [4, 4], [EOS, 3], [EOS, EOS], [EOS, EOS]]
CTC = [[3, 3, 5, 5, 4, 4], [3, 0, 0, 0, 0, 0]]


def test_ctc_weight_zero_is_todays_searcher_bit_for_bit():
    table, ctc = _att_table(ATT), _ctc_table(CTC)
    enc, lens = torch.zeros(2, 6, 4), torch.ones(2)
    want = _searcher(table)(enc, lens)
    got = _searcher(table, ctc, ctc_weight=0.0)(enc, lens)
    assert got[0] == want[0] == [[3, 4, 4], [3]]
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == b.dtype and torch.equal(a, b)


def test_ctc_term_overturns_the_attention_argmax_and_rows_freeze():
    """Row 0: the decoder wants 3 4 4 <eos>, the CTC head spells 3 5 4: at step 1 the joint argmax is 5 (the decoder's margin
    is log(0.5 / 0.075) = 1.9, the CTC margin about log(0.9 / 0.02) = 3.8).  Row 1 finishes at step 1 and stays frozen."""
    table, ctc = _att_table(ATT), _ctc_table(CTC)
    s = _searcher(table, ctc, ctc_weight=1.0)
    hyps, lengths, scores, log_probs = s(torch.zeros(2, 6, 4), torch.ones(2))
    assert hyps == [[3, 5, 4], [3]] and lengths.tolist() == [3, 1]
    assert log_probs.shape == (2, 4) and log_probs.dtype == torch.float32 and scores.dtype == torch.float32
    want = _walk(table, ctc, [6, 6], [[3, 5, 4, EOS], [3, EOS]], 1.0)
    torch.testing.assert_close(log_probs[0], torch.tensor(want[0]), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(log_probs[1, :2], torch.tensor(want[1]), rtol=1e-5, atol=1e-5)
    assert bool((log_probs[1, 2:] == 0).all())                                  # frozen behind its <eos>
    torch.testing.assert_close(scores, log_probs.sum(1))
    # a smaller weight leaves the decoder's choice standing where 0.2 x the CTC margin stays under the decoder's
    weak = _searcher(table, ctc, ctc_weight=0.2)(torch.zeros(2, 6, 4), torch.ones(2))
    assert weak[0][0][:2] == [3, 4]


def test_eos_floor_holds_with_ctc_on_and_blank_is_never_chosen():
    """The decoder's winner is blank at step 1 and <eos> everywhere else; the floor (0.5 x 6 frames = step 3) bars <eos>, the
    CTC term bars blank (-inf): the tokens come from the CTC head's spelling until the floor is passed."""
    rows = [[EOS], [BLANK], [EOS], [EOS], [EOS], [EOS]]
    table, ctc = _att_table(rows), _ctc_table([[3, 3, 5, 5, 4, 4]])
    s = _searcher(table, ctc, ctc_weight=1.0, min_decode_ratio=0.5)
    hyps, lengths, scores, log_probs = s(torch.zeros(1, 6, 4), torch.ones(1))
    assert hyps == [[3, 5, 4]] and lengths.tolist() == [3] and log_probs.shape == (1, 4)
    assert bool(torch.isfinite(log_probs).all()) and bool(torch.isfinite(scores).all())
    want = _walk(table, ctc, [6], [[3, 5, 4, EOS]], 1.0)
    torch.testing.assert_close(log_probs[0], torch.tensor(want[0]), rtol=1e-5, atol=1e-5)
    # without the CTC term the same table picks blank at step 1
    plain = _searcher(table, min_decode_ratio=0.5)(torch.zeros(1, 6, 4), torch.ones(1))
    assert plain[0][0][1] == BLANK


def test_searcher_arguments():
    from mamba_asr_amd.s2s_decode import CTCPrefixScorer, S2SGreedySearcher
    with pytest.raises(ValueError, match="ctc_fn"):
        S2SGreedySearcher(step_fn=lambda t, s: None, init_fn=lambda e: None, ctc_weight=0.4)
    with pytest.raises(ValueError):
        S2SGreedySearcher(step_fn=lambda t, s: None, init_fn=lambda e: None, ctc_weight=-1.0, ctc_fn=lambda e: e)
    s = S2SGreedySearcher(step_fn=lambda t, s: None, init_fn=lambda e: None, ctc_weight=0.4, ctc_fn=lambda e: e, blank_index=0)
    assert isinstance(s.ctc_scorer, CTCPrefixScorer) and (s.ctc_scorer.blank_index, s.ctc_scorer.eos_index) == (0, 2)
    for name in ("init", "score", "advance", "reorder"):
        assert callable(getattr(s.ctc_scorer, name))


# ----------------------------------------------------------------------------------------------------------
# the C boundary
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


def test_symbols_are_in_the_header_and_the_abi_is_still_12(native):
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    for name in ("cm_ctc_prefix_score", "cm_ctc_prefix_advance"):
        assert re.search(r"^int " + name + r"\(const cm_ctc_prefix_args \*args\);", hdr, re.M), name
        assert name in {s[0] for s in native.SYMBOLS}
        assert hasattr(native.lib(), name)
    assert "typedef struct cm_ctc_prefix_args" in hdr
    assert re.search(r"^#define CM_ABI_VERSION 12$", hdr, re.M)
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12
    tile = int(re.search(r"^#define CM_CTC_PREFIX_TILE_C (\d+)$", hdr, re.M).group(1))
    chunk = int(re.search(r"^#define CM_CTC_PREFIX_TCHUNK (\d+)$", hdr, re.M).group(1))
    assert (tile, chunk) == (native.CM_CTC_PREFIX_TILE_C, native.CM_CTC_PREFIX_TCHUNK)


def test_bad_arguments_are_rejected_before_any_launch(native):
    lib = native.lib()
    for fn in (lib.cm_ctc_prefix_score, lib.cm_ctc_prefix_advance):
        assert fn(None) == -1 and b"NULL" in lib.cm_last_error()
        a = native.CtcPrefixArgs()                                  # all zero
        assert fn(C.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
        a.U, a.T, a.V, a.rows = 2, 8, 5, 3
        a.blank, a.eos = 0, 5
        assert fn(C.byref(a)) == -1 and b"eos" in lib.cm_last_error()
        a.eos = 0
        assert fn(C.byref(a)) == -1 and b"eos" in lib.cm_last_error()      # blank and <eos> must differ
        a.eos = 2
        assert fn(C.byref(a)) == -1 and b"NULL pointer" in lib.cm_last_error()
    # every shared pointer set (host memory: nothing below gets as far as a launch)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value
    a = native.CtcPrefixArgs()
    a.U, a.T, a.V, a.rows, a.blank, a.eos = 2, 8, 5, 3, 0, 2
    a.logp = a.n_u = a.row_utt = a.last = a.r_n = a.r_b = a.psi_g = p
    assert lib.cm_ctc_prefix_score(C.byref(a)) == -1 and b"NULL pointer" in lib.cm_last_error()     # out
    a.out, a.K = p, 4
    assert lib.cm_ctc_prefix_score(C.byref(a)) == -1 and b"candidates" in lib.cm_last_error()       # K without candidates
    a.K, a.candidates = 0, p
    assert lib.cm_ctc_prefix_score(C.byref(a)) == -1 and b"candidates" in lib.cm_last_error()
    a.K = -1
    assert lib.cm_ctc_prefix_score(C.byref(a)) == -1
    assert lib.cm_ctc_prefix_advance(C.byref(a)) == -1 and b"NULL pointer" in lib.cm_last_error()   # tokens / outputs
    a.tokens = a.r_n_out = a.r_b_out = a.psi_out = a.last_out = p
    assert lib.cm_ctc_prefix_advance(C.byref(a)) == -1 and b"alias" in lib.cm_last_error()          # in place is refused


def test_ops_refuse_cpu_tensors_and_bad_shapes(native):
    from mamba_asr_amd import ops
    logp = torch.zeros(2, 8, 5)
    i32 = torch.zeros(2, dtype=torch.int32)
    st = torch.zeros(2, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ctc_prefix_score(logp, i32, i32, i32, st, st, torch.zeros(2), 0, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ctc_prefix_advance(logp, i32, i32, i32, st, st, torch.zeros(2), i32, 0, 2)
    from mamba_asr_amd.s2s_decode import CTCPrefixScorer
    with pytest.raises(ValueError, match="row_utt"):
        CTCPrefixScorer(0, 2).init(logp, torch.tensor([8.0, 8.0]), row_utt=torch.tensor([0, 2]))
