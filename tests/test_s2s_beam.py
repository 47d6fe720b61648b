"""Host logic of mamba_asr_amd.s2s_decode.S2SBeamSearcher, without a GPU: the per-token selection is injected
(``select_fn`` = tests/s2s_beam_ref.select, the contract of ops.beam_select in torch) and the per-token function is a scripted
table.  The toy decoder state carries every row's prefix and has ``reorder``, so a wrong parent shows as a wrong table row."""
import itertools
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2s_beam_ref as R  # noqa: E402

BOS, EOS, V = 1, 2, 6
NEG = -math.inf


class ToyState:
    """prefixes[row]: the tokens fed so far, <bos> included"""

    def __init__(self, prefixes):
        self.prefixes = prefixes

    def reorder(self, index):
        return ToyState([self.prefixes[int(i)] for i in index])


def _beam(fn, beam_size, seen=None, **kw):
    """fn(utterance, prefix without <bos>) -> (V,) log-probabilities of the next token"""
    from mamba_asr_amd.s2s_decode import S2SBeamSearcher

    def init_fn(enc):
        return ToyState([()] * enc.shape[0])

    def step_fn(tokens, state):
        if seen is not None:
            seen.append(tokens.tolist())
        state = ToyState([p + (int(t),) for p, t in zip(state.prefixes, tokens)])
        return torch.stack([fn(r // beam_size, p[1:]) for r, p in enumerate(state.prefixes)]), state

    kw.setdefault("select_fn", R.select)
    return S2SBeamSearcher(bos_index=BOS, eos_index=EOS, step_fn=step_fn, init_fn=init_fn, beam_size=beam_size, **kw)


# ---------------------------------------------------------------------------------------------------------- beam 1 == greedy
def _table(rows):
    """tests/test_s2s_decode.py's scripted table: rows[t][b] = the token that wins at step t for row b -> (steps, batch, V)"""
    steps, batch = len(rows), len(rows[0])
    p = torch.full((steps, batch, V), 0.3 / (V - 2))
    for t in range(steps):
        for b in range(batch):
            p[t, b, EOS] = 0.2
            if rows[t][b] == EOS:
                p[t, b] = 0.5 / (V - 1)
            p[t, b, rows[t][b]] = 0.5
    return torch.log(p)


def _greedy(table, **kw):
    from mamba_asr_amd.s2s_decode import S2SGreedySearcher

    def step_fn(tokens, state):
        lp = table[state["t"]]
        state["t"] += 1
        return lp, state

    return S2SGreedySearcher(bos_index=BOS, eos_index=EOS, step_fn=step_fn, init_fn=lambda enc: {"t": 0}, **kw)


GREEDY_CASES = {
    "first_eos_freezes": ([[3, 4, 5], [EOS, 4, 3], [3, 5, 4], [4, EOS, 4], [5, 3, EOS], [3, 3, 3]], (3, 10), [1.0, 1.0, 1.0],
                          dict(min_decode_ratio=0.0, max_decode_ratio=1.0)),
    "eos_floor_per_row": ([[EOS, EOS]] * 6, (2, 10), [1.0, 0.5], dict(min_decode_ratio=0.3, max_decode_ratio=1.0)),
    "cap": ([[3, 4]] * 20, (2, 12), [0.5, 1.0], dict(min_decode_ratio=0.0, max_decode_ratio=0.5)),
    "eos_at_step_zero": ([[EOS, EOS, EOS]] * 4, (3, 8), [1.0, 1.0, 1.0], dict()),
    "zero_steps": ([[EOS, EOS, EOS]] * 4, (3, 8), [1.0, 1.0, 1.0], dict(max_decode_ratio=0.0)),
}


@pytest.mark.parametrize("case", sorted(GREEDY_CASES))
def test_beam_one_without_normalisation_is_the_greedy_searcher(case):
    rows, (batch, T), lens, kw = GREEDY_CASES[case]
    table = _table(rows)
    enc, lens = torch.zeros(batch, T, 4), torch.tensor(lens)
    want = _greedy(table, **kw)(enc, lens)
    got = _beam(lambda u, prefix: table[len(prefix), u], 1, length_normalization=False, **kw)(enc, lens)
    assert got[0] == want[0]
    for a, b in zip(got[1:], want[1:]):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------- nothing pruned
def _dyadic(seed):
    """prefix -> 4 log-'probabilities', multiples of 2^-8 in [-8, 0): sums of up to five of them are exact in fp32.  Tokens:
    0 and 3 are symbols, 1 = <bos> (never offered), 2 = <eos>."""
    cache = {}

    def fn(u, prefix):
        if prefix not in cache:
            g = torch.Generator().manual_seed(seed * 1000 + sum((c + 1) * 7 ** i for i, c in enumerate(prefix)) + 97 * len(prefix))
            row = -torch.randint(1, 2048, (4,), generator=g).float() / 256.0
            row[BOS] = NEG
            cache[prefix] = row
        return cache[prefix]

    return fn


def _enumerate(fn, cap, norm):
    """every hypothesis the search can end with when nothing is pruned -> [(tokens, final fp32 score)], best first"""
    out = []
    for n in range(cap + 1):
        for seq in itertools.product((0, 3), repeat=n):
            raw = np.float32(0)
            for i, c in enumerate(seq):
                raw = raw + np.float32(fn(0, seq[:i])[c])
            if n < cap:                                                          # closed by <eos> at step n
                raw, n_inc = raw + np.float32(fn(0, seq)[EOS]), n + 1
            else:                                                                # cut by the cap: closed as it is
                n_inc = n
            out.append((list(seq), raw / np.float32(n_inc) if norm else raw))
    out.sort(key=lambda h: -h[1])
    return out


@pytest.mark.parametrize("norm", [False, True])
def test_beam_128_equals_enumeration_of_all_sequences(norm):
    fn, cap = _dyadic(seed=3), 4
    want = _enumerate(fn, cap, norm)
    finals = [float(h[1]) for h in want]
    assert len(set(finals[:6])) == 6, "the table must not tie among the best"
    assert _enumerate(fn, cap, True)[0][0] != _enumerate(fn, cap, False)[0][0], "the table must make normalisation matter"
    enc, lens = torch.zeros(1, 8, 4), torch.ones(1)                              # cap = floor(0.5 * 8) = 4
    kw = dict(max_decode_ratio=0.5, length_normalization=norm)
    hyps, lengths, scores, log_probs = _beam(fn, 128, **kw)(enc, lens)
    assert hyps == [want[0][0]] and lengths.tolist() == [len(want[0][0])]
    assert scores.tolist() == [finals[0]]
    n_inc = min(len(want[0][0]) + 1, cap)
    raw = float(log_probs[0].sum())
    assert (raw / n_inc if norm else raw) == pytest.approx(finals[0], abs=1e-6) and bool((log_probs[0, n_inc:] == 0).all())
    hyps5, lengths5, scores5, log_probs5 = _beam(fn, 128, topk=5, **kw)(enc, lens)
    assert hyps5 == [[h[0] for h in want[:5]]]
    assert scores5.shape == (1, 5) and scores5[0].tolist() == finals[:5]
    assert lengths5.tolist() == [[len(h[0]) for h in want[:5]]] and torch.equal(log_probs5, log_probs)
    # the slow restatement of the same contract agrees
    ranked, _, steps = R.beam_search(lambda prefix: fn(0, tuple(prefix[1:])), 4, 128, BOS, EOS, 0, cap, norm, 5, np.float32)
    assert steps == cap and [h[0] for h in ranked] == hyps5[0] and [float(h[1]) for h in ranked] == finals[:5]


# ---------------------------------------------------------------------------------------------------------- scripted paths
def _rows(spec):
    """{prefix: {token: log-probability}} -> fn; everything not named is -inf"""
    def fn(u, prefix):
        row = torch.full((V,), NEG)
        for c, v in spec.get(prefix, {}).items():
            row[c] = v
        return row
    return fn


def test_beam_two_beats_greedy_on_a_garden_path():
    fn = _rows({(): {3: -0.5, 4: -0.75}, (3,): {5: -4.0, EOS: -5.0}, (4,): {5: -0.25, EOS: -6.0},
                (3, 5): {EOS: -4.0}, (4, 5): {EOS: -0.25}})
    enc, lens = torch.zeros(1, 8, 4), torch.ones(1)
    g = _beam(fn, 1, length_normalization=False)(enc, lens)
    b = _beam(fn, 2, length_normalization=False)(enc, lens)
    assert g[0] == [[3, 5]] and g[2].tolist() == [-8.5]
    assert b[0] == [[4, 5]] and b[2].tolist() == [-1.25] and float(b[2]) > float(g[2])
    assert b[3][0, :3].tolist() == [-0.75, -0.25, -0.25]


TIES = {(): {3: -1.0, 4: -1.5, EOS: -8.0}, (3,): {3: -0.5, EOS: -1.0}, (4,): {3: -0.25},
        (3, 3): {EOS: -0.5}, (4, 3): {EOS: -0.25}}


def test_equal_scores_rank_by_completion_then_slot_and_the_loop_stops_at_beam_finished():
    seen = []
    s = _beam(_rows(TIES), 3, seen, length_normalization=False, topk=4)
    hyps, lengths, scores, log_probs = s(torch.zeros(1, 20, 4), torch.ones(1))   # cap 20
    # finished: [] (-8, step 0), [3] (-2, step 1), [3, 3] (-2, step 2, slot 0), [4, 3] (-2, step 2, slot 1): 4 >= 3 ends the loop
    assert len(seen) == 3 and log_probs.shape == (1, 3)
    assert hyps == [[[3], [3, 3], [4, 3], []]]
    assert scores.tolist() == [[-2.0, -2.0, -2.0, -8.0]] and lengths.tolist() == [[1, 2, 2, 0]]
    assert log_probs.tolist() == [[-1.0, -1.0, 0.0]]
    # the first call gets <bos> everywhere; the slot that took <eos> steps on <eos>
    assert seen[0] == [BOS] * 3 and seen[1] == [3, 4, EOS] and seen[2] == [3, 3, EOS]
    # with normalisation the longer ones win: -2/3 < -2/2
    hyps_n = _beam(_rows(TIES), 3, topk=4)(torch.zeros(1, 20, 4), torch.ones(1))[0]
    assert hyps_n == [[[3, 3], [4, 3], [3], []]]


def test_dead_slots_step_on_eos_and_the_loop_ends_when_nothing_lives():
    seen = []
    fn = _rows({(): {3: -1.0, 4: -2.0}, (3,): {5: -1.0}, (3, 5): {EOS: -1.0}})    # two finite candidates for four slots
    hyps, lengths, scores, log_probs = _beam(fn, 4, seen, length_normalization=False)(torch.zeros(2, 20, 4), torch.ones(2))
    assert seen[1] == [3, 4, EOS, EOS] * 2                                       # the -inf fill is (slot 0, token 0): fed as <eos>
    assert seen[2] == [5, EOS, EOS, EOS] * 2
    assert len(seen) == 3                                                        # one finished of four, but no slot alive: not 20 calls
    assert hyps == [[3, 5], [3, 5]] and scores.tolist() == [-3.0, -3.0]


def test_utterances_do_not_mix():
    a, b = _rows(TIES), _rows({(): {5: -0.5}, (5,): {EOS: -0.5}})
    both = _beam(lambda u, p: (a, b)[u](0, p), 3, topk=2)(torch.zeros(2, 20, 4), torch.ones(2))
    only_a = _beam(a, 3, topk=2)(torch.zeros(1, 20, 4), torch.ones(1))
    assert both[0][0] == only_a[0][0] and both[0][1] == [[5]]
    assert torch.equal(both[2][0], only_a[2][0]) and both[2][1].tolist() == [-0.5, NEG]
    # an utterance that has its beam_size finished hypotheses is over, however long its neighbour goes on: the slot of
    # TIES that is still alive at step 2 would otherwise finish [3, 3, 3] with -1.75 / 4 and win under normalisation
    ties = dict(TIES)
    ties[(3, 3)] = {EOS: -0.5, 3: -0.125}
    ties[(3, 3, 3)] = {EOS: -0.125}
    a = _rows(ties)
    long_b = _rows({(5,) * n: {5: -0.5} for n in range(20)})
    both = _beam(lambda u, p: (a, long_b)[u](0, p), 3, topk=3)(torch.zeros(2, 20, 4), torch.ones(2))
    only_a = _beam(a, 3, topk=3)(torch.zeros(1, 20, 4), torch.ones(1))
    assert both[3].shape == (2, 20) and only_a[3].shape == (1, 3)                # the cap, 20 steps, against 3
    assert both[0][0] == only_a[0][0] and torch.equal(both[2][0], only_a[2][0]) and torch.equal(both[1][0], only_a[1][0])
    assert torch.equal(both[3][0, :3], only_a[3][0]) and bool((both[3][0, 3:] == 0).all())
    assert both[0][1][0] == [5] * 20


def test_ctc_scorer_sees_reorder_before_advance_with_row_utt():
    log = []

    class Stub:
        def init(self, logp, enc_lens, row_utt=None):
            log.append(("init", row_utt.tolist()))
            return {"rows": list(range(len(row_utt)))}

        def score(self, state):
            log.append(("score", list(state["rows"])))
            d = torch.zeros(len(state["rows"]), V)
            d[:, 4] = -10.0                                                      # weight 0.5: token 4 loses 5
            return d

        def reorder(self, state, index):
            log.append(("reorder", [int(i) for i in index]))
            return {"rows": [state["rows"][int(i)] for i in index]}

        def advance(self, state, tokens):
            log.append(("advance", tokens.tolist()))
            return state

    fn = _rows({(): {3: -1.0, 4: -0.5}, (3,): {EOS: -1.0}, (4,): {EOS: -1.0}})
    s = _beam(fn, 2, length_normalization=False, ctc_weight=0.5, ctc_scorer=Stub(), ctc_fn=lambda enc: torch.zeros(2, 20, V))
    hyps, _, scores, log_probs = s(torch.zeros(2, 20, 4), torch.ones(2))
    assert hyps == [[3], [3]] and scores.tolist() == [-2.0, -2.0]
    assert log_probs[0].tolist() == [-1.0, -1.0]                                 # the joint increments
    assert [k for k, _ in log] == ["init", "score", "reorder", "advance", "score", "reorder", "advance"]
    assert log[0][1] == [0, 0, 1, 1]
    assert log[2][1] == [0, 0, 2, 2] and log[3][1] == [3, 4, 3, 4]               # rows u * B + parent, then the new tokens
    assert log[5][1] == [0, 1, 2, 3] and log[6][1] == [EOS] * 4


def test_select_torch_is_the_contract_where_nothing_ties(monkeypatch):
    from mamba_asr_amd import s2s_decode
    g = torch.Generator().manual_seed(5)
    att, delta = torch.randn(6, 37, generator=g), torch.randn(6, 37, generator=g)
    alive = torch.tensor([0.0, -1.0, -0.5, NEG, -2.0, -0.25])
    blocked = torch.tensor([1, 0], dtype=torch.int32)
    for kw in (dict(), dict(delta=delta, weight=0.4), dict(delta=delta, weight=0.4, eos_blocked=blocked)):
        got, want = s2s_decode.select_torch(att, alive, 3, EOS, **kw), R.select(att, alive, 3, EOS, **kw)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and torch.equal(a, b)
    monkeypatch.setenv("CM_BEAM_SELECT", "0")
    s = s2s_decode.S2SBeamSearcher(step_fn=lambda t, s: None, init_fn=lambda e: None)
    assert s.select_fn is s2s_decode.select_torch and s.beam_size == 10 and s.length_normalization and s.topk == 1


def test_what_is_not_provided_raises():
    from mamba_asr_amd.asr import ConMambaASR
    from mamba_asr_amd.s2s_decode import S2SBeamSearcher
    base = dict(step_fn=lambda t, s: None, init_fn=lambda e: None, select_fn=R.select)
    for kw in (dict(using_eos_threshold=True), dict(scorer=object()), dict(lm_weight=0.5), dict(lm_modules=object())):
        with pytest.raises(NotImplementedError, match="not provided"):
            S2SBeamSearcher(**base, **kw)
    for kw in (dict(beam_size=0), dict(beam_size=129), dict(topk=0), dict(temperature=0.0), dict(ctc_weight=0.4)):
        with pytest.raises(ValueError):
            S2SBeamSearcher(**base, **kw)
    with pytest.raises(ValueError, match="modules"):
        S2SBeamSearcher(modules=None)
    with pytest.raises(TypeError):
        S2SBeamSearcher(**base, coverage_penalty=1.5)
    stub = types.SimpleNamespace(cfg=types.SimpleNamespace(num_decoder_layers=1), training=False)
    searcher = S2SBeamSearcher(**base)
    for kw in (dict(beam_size=3), dict(length_normalization=False), dict(temperature=1.15), dict(topk=2)):
        with pytest.raises(ValueError, match="searcher"):
            ConMambaASR.transcribe_s2s(stub, None, None, searcher=searcher, **kw)
    with pytest.raises(ValueError, match="beam_size"):
        ConMambaASR.transcribe_s2s(stub, None, None, temperature=1.15)


# ---------------------------------------------------------------------------------------------------------- the C entry point
def test_cm_beam_select_is_declared_and_validates_on_the_host():
    import ctypes as ct
    import re
    from mamba_asr_amd import _native as N, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "conmamba_hip.h")).read()
    assert re.search(r"^int cm_beam_select\(const cm_beam_select_args \*args\);", hdr, re.M)
    assert re.search(r"^int64_t cm_beam_select_workspace_bytes\(int32_t U, int32_t B, int32_t V\);", hdr, re.M)
    assert re.search(r"^#define CM_ABI_VERSION 12$", hdr, re.M) and N.ABI_VERSION == 12          # additive: the ABI stays
    assert int(re.search(r"^#define CM_BEAM_SELECT_MAX_B (\d+)$", hdr, re.M).group(1)) == N.CM_BEAM_SELECT_MAX_B == 128
    chunk = int(re.search(r"^#define CM_BEAM_SELECT_CHUNK (\d+)$", hdr, re.M).group(1))
    assert chunk == N.CM_BEAM_SELECT_CHUNK
    lib = N.lib()
    ws = lib.cm_beam_select_workspace_bytes
    assert ws(4, 66, 5000) == 4 * 66 * 1 * 66 * 12 and ws(4, 66, chunk + 1) == 4 * 66 * 2 * 66 * 12 and ws(1, 1, 1) == 12
    assert ws(0, 1, 1) == 0 and ws(1, 0, 5) == 0 and ws(1, 129, 5) == 0 and ws(1, 128, 2 ** 24) == 0 and ws(1, 1, 0) == 0
    assert lib.cm_beam_select(None) == -1
    a = N.BeamSelectArgs()
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    a.U, a.B, a.V = 2, 129, 50
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    a.B, a.V = 128, 2 ** 24                                                      # B * V = 2^31
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    a.B, a.V = 4, 50
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"NULL pointer" in lib.cm_last_error()
    buf = (ct.c_uint64 * 64)()
    base = ct.addressof(buf)
    for name in ("att", "alive", "score", "inc", "parent", "token", "workspace"):
        setattr(a, name, base)
    a.att = base + 2
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"misaligned" in lib.cm_last_error()
    a.att, a.workspace = base, base + 4
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"misaligned" in lib.cm_last_error()
    a.workspace, a.workspace_bytes = base, ws(2, 4, 50) - 1
    assert lib.cm_beam_select(ct.byref(a)) == -1 and b"workspace" in lib.cm_last_error()
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.beam_select(torch.zeros(4, 8), torch.zeros(4), 2, 2)
