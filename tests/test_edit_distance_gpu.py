"""cm_edit_distance on the GPU against tests/ctc_score_ref.py: counts, dist, status, ops and n_ops bit for bit, at the sizes where the
kernel changes path -- empty sides, one column, a wave of columns (63, 64, 65), the 32-step move words (15/17, 16/16, 33/31), the
1023-token square and its thin extremes -- over a 2-symbol alphabet (ties in nearly every cell) and a 1000-symbol one, with
identical and disjoint pairs, padding that may not be read, references shared through ref_index, an index outside the references,
guard bands, the oversize refusal and metrics' route around it.  The tie rule is the contract's."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_score_ref as SR  # noqa: E402
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPES = [(0, 0), (0, 3), (3, 0), (1, 1), (15, 17), (16, 16), (33, 31), (63, 64), (64, 65), (65, 63), (1, 1023), (1023, 1), (17, 600)]
PAD = 7777                                                            # an id no sequence holds: reading it would change a count
_REF = {}


def _seqs(R, H, alphabet, seed):
    rng = random.Random(seed * 100003 + R * 1031 + H * 7 + alphabet)
    return [rng.randrange(alphabet) for _ in range(R)], [rng.randrange(alphabet) for _ in range(H)]


def _ref(a, b):
    """tests/ctc_score_ref.edit_ops, computed once per pair."""
    key = (tuple(a), tuple(b))
    if key not in _REF:
        _REF[key] = SR.edit_ops(a, b)
    return _REF[key]


def _pack(seqs, width=None):
    width = max((len(s) for s in seqs), default=0) if width is None else width
    t = torch.full((len(seqs), width), PAD, dtype=torch.int32)
    for k, s in enumerate(seqs):
        t[k, :len(s)] = torch.tensor(s, dtype=torch.int32)
    return t, torch.tensor([len(s) for s in seqs], dtype=torch.int32)


def _run(refs, hyps, ref_index=None, bufs=None, widths=(None, None)):
    from mamba_asr_amd import ops
    rt, rl = _pack(refs, widths[0])
    ht, hl = _pack(hyps, widths[1])
    ri = None if ref_index is None else torch.tensor(ref_index, dtype=torch.int32, device=DEV)
    out = ops.edit_distance(rt.to(DEV), rl.to(DEV), ht.to(DEV), hl.to(DEV), ri, want_ops=True, bufs=bufs)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _compare(got, refs, hyps, ref_index=None, invariants=True):
    counts, dist, status, ops, n_ops = got
    assert counts.dtype == dist.dtype == status.dtype == n_ops.dtype == torch.int32 and ops.dtype == torch.int8
    for p, b in enumerate(hyps):
        a = refs[p if ref_index is None else ref_index[p]]
        want_counts, want_dist, want_path = _ref(a, b)
        k = int(n_ops[p])
        path = bytes(ops[p, :k].numpy().astype(np.uint8)).decode("ascii")
        assert status[p] == 0 and counts[p].tolist() == want_counts and int(dist[p]) == want_dist and path == want_path, \
            (p, len(a), len(b), counts[p].tolist(), want_counts, int(dist[p]), want_dist, path[:80], want_path[:80])
        assert (ops[p, k:] == 0).all()
        if invariants:
            SR.check_invariants(a, b, counts[p].tolist(), int(dist[p]), path)


@pytest.mark.parametrize("alphabet", [2, 1000])
def test_every_shape_in_one_ragged_launch(alphabet):
    """All the shapes as ONE batch: every pair is padded to (1023, 1023) with an id that may not be read."""
    pairs = [_seqs(R, H, alphabet, 1) for R, H in SHAPES]
    refs, hyps = [a for a, _ in pairs], [b for _, b in pairs]
    got = _run(refs, hyps)
    assert got[3].shape == (len(SHAPES), 2046)
    _compare(got, refs, hyps)
    if alphabet == 2:
        c = got[0]
        assert int((c[:, 0] > 0).sum()) >= 5 and int((c[:, 1] > 0).sum()) >= 5 and int((c[:, 2] > 0).sum()) >= 3


@pytest.mark.parametrize("R, H", SHAPES)
def test_every_shape_alone(R, H):
    """Each shape at its own widths (SR = R, SH = H: zero-width tensors, one block of 64 threads, ...), 2-symbol alphabet."""
    a, b = _seqs(R, H, 2, 2)
    got = _run([a], [b])
    assert got[3].shape == (1, R + H)
    _compare(got, [a], [b])


def test_the_largest_square_runs_once():
    for alphabet in (2, 1000):
        a, b = _seqs(1023, 1023, alphabet, 3)
        got = _run([a], [b])
        _compare(got, [a], [b], invariants=alphabet == 2)
    a, b = _seqs(1024, 1024, 3, 3)                                  # the cap itself
    _compare(_run([a], [b]), [a], [b], invariants=False)


def test_identical_disjoint_and_shared_references():
    rng = random.Random(9)
    base = [rng.randrange(50) for _ in range(70)]
    refs = [base, [x + 100 for x in base[:40]], []]
    hyps = [base, [x + 200 for x in base], base[:35] + base[36:], [x + 100 for x in base[:40]], [5, 6], [], base[::-1]]
    ri = [0, 0, 0, 1, 2, 2, 1]
    got = _run(refs, hyps, ri)
    _compare(got, refs, hyps, ri)
    counts = got[0].tolist()
    assert counts[0] == [0, 0, 0, 70] and counts[1] == [0, 0, 70, 0] and counts[2] == [0, 1, 0, 69]      # identical, disjoint, one deletion
    assert counts[3] == [0, 0, 0, 40] and counts[4] == [2, 0, 0, 0] and counts[5] == [0, 0, 0, 0]
    own = _run([refs[r] for r in ri], hyps)                          # the same with the references copied
    for g, o in zip(got, own):
        assert torch.equal(g, o)
    assert _run(refs, hyps, ri)[3].equal(got[3])                     # twice the same


def test_ref_index_out_of_range():
    a, b = _seqs(20, 22, 4, 5)
    got = _run([a, a[:7]], [b, b, b, b], [0, 2, -1, 1])
    counts, dist, status, ops, n_ops = got
    assert status.tolist() == [0, 1, 1, 0] and counts[1].tolist() == [0, 0, 0, 0] == counts[2].tolist()
    assert dist[1] == 0 and n_ops[1] == 0 and n_ops[2] == 0 and (ops[1] == 0).all() and (ops[2] == 0).all()
    for p, r in ((0, a), (3, a[:7])):
        want = _ref(r, b)
        assert counts[p].tolist() == want[0] and bytes(ops[p, :int(n_ops[p])].numpy().astype(np.uint8)).decode() == want[2]


def test_without_ops_the_counts_are_the_same():
    from mamba_asr_amd import ops
    pairs = [_seqs(R, H, 2, 6) for R, H in SHAPES[:10]]
    refs, hyps = [a for a, _ in pairs], [b for _, b in pairs]
    full = _run(refs, hyps)
    rt, rl = _pack(refs)
    ht, hl = _pack(hyps)
    out = ops.edit_distance(rt.to(DEV), rl.to(DEV), ht.to(DEV), hl.to(DEV))
    assert len(out) == 3 and all(torch.equal(o.cpu(), f) for o, f in zip(out, full[:3]))
    with pytest.raises(RuntimeError, match="its own reference"):
        ops.edit_distance(rt[:3].to(DEV), rl[:3].to(DEV), ht.to(DEV), hl.to(DEV))


@pytest.mark.parametrize("SR_, SH_", [(17, 15), (40, 70)])
def test_guard_bands(monkeypatch, SR_, SH_):
    """Outputs inside sentinels, the sequences inside a guard id that differs from every token, the lengths inside a guard that
    reaches the padding, ref_index inside a valid index, the workspace a scratch."""
    import ctypes as ct
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    calls = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, fn, args, units=0: (calls.append((name, args)), real(name, fn, args, units))[1])
    rng = random.Random(SR_)
    refs = [[rng.randrange(3) for _ in range(n)] for n in (SR_, SR_ - 3, 0)]
    hyps = [[rng.randrange(3) for _ in range(n)] for n in (SH_, SH_ - 1, 5, 0, SH_ // 2)]
    ri = [0, 1, 2, 0, 1]
    rt, rl = _pack(refs, SR_)
    ht, hl = _pack(hyps, SH_)
    rt, rl, ht, hl, rit = (t.to(DEV) for t in (rt, rl, ht, hl, torch.tensor(ri, dtype=torch.int32)))
    n = len(hyps)
    a = N.EditDistanceArgs()
    a.N, a.NR, a.SR, a.SH = n, len(refs), SR_, SH_
    nws = int(N.lib().cm_edit_distance_workspace_bytes(ct.byref(a)))
    assert nws > 0 and nws % 16 == 0
    # ops: int8 has no room for the integer sentinel 0xA5; the guarded buffer is uint8 and the kernel gets its int8 view
    shapes = dict(counts=((n, 4), torch.int32), dist=((n,), torch.int32), status=((n,), torch.int32), ops=((n, SR_ + SH_), torch.uint8),
                  n_ops=((n,), torch.int32))

    def run(L):
        r, h = L.ints(rt, PAD + 1), L.ints(ht, PAD + 2)
        rn, hn, idx = L.ints(rl, SR_, unique=False), L.ints(hl, SH_, unique=False), L.ints(rit, 0, unique=False)
        bufs = {name: L.out(name, shape, dt, contiguous=True) for name, (shape, dt) in shapes.items()}
        bufs["workspace"] = L.scratch("workspace", nws // 4).view(torch.uint8)
        bufs["ops"] = bufs["ops"].view(torch.int8)
        got = ops.edit_distance(r, rn, h, hn, idx, want_ops=True, bufs=bufs)
        assert all(t is bufs[name] for t, name in zip(got, ("counts", "dist", "status", "ops", "n_ops")))
        name, args = calls[-1]
        assert name == "cm_edit_distance" and args.workspace_bytes == nws
        for f, t in dict(bufs, refs=r, ref_len=rn, hyps=h, hyp_len=hn, ref_index=idx).items():
            assert getattr(args, f) == t.data_ptr(), f"{f}: the wrapper copied it"
    outs = G.two_step(run, DEV)
    outs["ops"] = outs["ops"].view(torch.int8)
    _compare([outs[k].cpu() for k in ("counts", "dist", "status", "ops", "n_ops")], refs, hyps, ri)


def test_oversize_is_refused_and_metrics_routes_around_it():
    from mamba_asr_amd import _native as N
    from mamba_asr_amd import metrics, ops
    assert N.CM_EDIT_MAX_LEN == 1024
    long_ref, hyp = _seqs(1025, 30, 5, 8)
    rt, rl = _pack([long_ref])
    ht, hl = _pack([hyp])
    with pytest.raises(RuntimeError, match="at most 1024 tokens"):
        ops.edit_distance(rt.to(DEV), rl.to(DEV), ht.to(DEV), hl.to(DEV))
    with pytest.raises(RuntimeError, match="at most 1024 tokens"):
        ops.edit_distance(ht.to(DEV), hl.to(DEV), rt.to(DEV), rl.to(DEV))
    torch.cuda.synchronize()
    calls = []
    real = ops.edit_distance
    try:
        ops.edit_distance = lambda *a, **k: (calls.append(a[2].shape), real(*a, **k))[1]
        a2, b2 = _seqs(40, 44, 5, 9)
        scored = metrics.score_pairs([long_ref, a2], [hyp, b2, long_ref], [0, 1, 1], device=DEV)
    finally:
        ops.edit_distance = real
    assert calls == [(1, 44)]                                        # one launch, for the one pair inside the limits
    for (c, path), (a, b) in zip(scored, [(long_ref, hyp), (a2, b2), (a2, long_ref)]):
        want = _ref(a, b)
        assert (c, path) == (want[0], want[2])
    host = metrics.score_pairs([long_ref, a2], [hyp, b2, long_ref], [0, 1, 1])
    assert host == scored


def test_error_rate_stats_on_the_gpu_equals_the_host():
    from mamba_asr_amd.metrics import ErrorRateStats
    rng = random.Random(12)
    words = ["w%d" % k for k in range(12)]
    refs = [[rng.choice(words) for _ in range(rng.randint(0, 9))] for _ in range(24)]
    hyps = [[rng.choice(words) for _ in range(rng.randint(0, 9))] for _ in range(24)]
    ids = list(range(24))
    for kw in ({}, {"split_tokens": True}):
        dev, host = ErrorRateStats(device=DEV, **kw), ErrorRateStats(**kw)
        dev.append(ids, hyps, refs)
        host.append(ids, hyps, refs)
        assert dev.scores == host.scores and dev.summarize() == host.summarize() and dev.summarize("num_edits") > 0
    nbest = [[h, r[:-1], r] for h, r in zip(hyps, refs)]
    got, want = ErrorRateStats(device=DEV).oracle(ids, nbest, refs), ErrorRateStats().oracle(ids, nbest, refs)
    assert got == want and all(rec["num_edits"] == 0 for rec in got)
    assert [rec["best_index"] for rec in got] == [0 if h == r else (1 if not r else 2) for h, r in zip(hyps, refs)]
