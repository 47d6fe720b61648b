"""cm_ctc_align on the GPU against tests/ctc_align_ref.py: all six outputs bit for bit (torch.equal / exact float64 equality), on
ragged batches at the sizes where the kernel changes path -- a wave of 32 label pairs, half a workgroup, the 1023-label cap, the
16-step move words and the backtrace's blocks -- with random, rounded (ties), -inf and bf16 strided inputs, shared rows, NaN on and
off the lattice, guard bands, and through CTCBeamSearcher.search(text_frames=True) and ConMambaASR.align.

Frames at and past an utterance's length are NaN and target padding is an id >= V in every case: neither may be read.
Every status-0 alignment is cross-checked independently of the reference: score <= -nll64 (1 - 1e-12) + 1e-9 with nll64 from
torch.nn.functional.ctc_loss on the CPU in float64 (a best path never beats the sum over paths), and score == the float64 sum of the
path's own log-probabilities recomputed from states, within 1e-9 (1 + |score|) (the two sums differ in order only)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as AR  # noqa: E402
import ctc_beam_data as D  # noqa: E402
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("score", "status", "states", "starts", "ends", "label_logp")

# name: (V, T, S, [(n, L) per utterance]); labels are drawn from 1 .. V - 1 (V = 2: "aa...", every pair needs a blank between)
CASES = {
    # (T, S) = (1, 0), (1, 1), (5, 0), (2, 1); "aa" in 3 frames exactly fits, in 2 it cannot; empty utterances
    "tiny_v2": (2, 5, 2, [(1, 0), (1, 1), (5, 0), (2, 1), (3, 2), (2, 2), (0, 0), (0, 1), (5, 2), (5, 1)]),
    "t1_s0": (3, 1, 0, [(1, 0), (0, 0)]),
    "t1_s1": (3, 1, 1, [(1, 1), (1, 0), (0, 1)]),
    "t5_s0": (4, 5, 0, [(5, 0), (3, 0)]),
    "t2_s1": (4, 2, 1, [(2, 1), (1, 1), (2, 0)]),
    "s31": (31, 80, 31, [(80, 31), (64, 31), (33, 20), (30, 31)]),
    "s32": (31, 80, 32, [(80, 32), (79, 31), (66, 32)]),
    "s33": (31, 81, 33, [(81, 33), (80, 32), (70, 33), (16, 0)]),
    "s511": (31, 600, 511, [(600, 511), (540, 500)]),
    "s512": (31, 600, 512, [(600, 512), (599, 511), (17, 3)]),
    "s1023": (31, 1100, 1023, [(1100, 1023), (1090, 1000)]),
    "t15": (31, 15, 20, [(15, 7), (15, 5), (9, 4)]),
    "t16": (31, 16, 20, [(16, 7), (15, 6), (16, 0)]),
    "t17": (31, 17, 20, [(17, 8), (16, 7), (1, 1)]),
    "t33": (31, 33, 20, [(33, 20), (32, 15), (33, 12), (21, 20)]),
    "t1000": (31, 1000, 20, [(1000, 20), (977, 19), (500, 20)]),
    "v5000": (5000, 33, 20, [(33, 20), (31, 14), (17, 8)]),
}
QUICK = ["tiny_v2", "s33", "t17", "t33"]


def _case(name, seed=0, kind="random"):
    """-> lp (B, T, V) float32 on the host (NaN at and past every length), targets (B, S) int64 (padding V + 3), lengths."""
    V, T, S, specs = CASES[name]
    g = torch.Generator().manual_seed(1000 * seed + sum(map(ord, name)))
    B = len(specs)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * 2.0, dim=-1)
    if kind == "round":
        lp = torch.round(lp)                                        # small integers: exact ties abound
    targets = torch.full((B, S), V + 3, dtype=torch.int64)
    for b, (n, L) in enumerate(specs):
        targets[b, :L] = torch.randint(1, V, (L,), generator=g)
        lp[b, n:] = float("nan")
    il = torch.tensor([n for n, _ in specs], dtype=torch.int32)
    tl = torch.tensor([L for _, L in specs], dtype=torch.int32)
    return lp, targets, il, tl


def _run(lp, targets, il, tl, blank=0, rows=None, bufs=None):
    from mamba_asr_amd import ops
    out = ops.ctc_align(lp, targets.to(DEV), il.to(DEV), tl.to(DEV), blank=blank, rows=None if rows is None else rows.to(DEV), bufs=bufs)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.numpy() if torch.is_tensor(g) else g
        w = w.numpy() if torch.is_tensor(w) else w
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | ((g != g) & (w != w))))
            raise AssertionError(f"{what}: {name} differs at {len(bad)} place(s); first {tuple(bad[0])}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}")


def _cross_check(lp64, targets, il, tl, out, blank, rows=None, nll=True):
    """The two independent checks of the module docstring on every status-0 utterance.  -> how many there were."""
    score, status, states, starts, ends, logp = [o.numpy() for o in out]
    done = 0
    for b in range(targets.shape[0]):
        if status[b] != 0:
            continue
        n, L = int(il[b]), int(tl[b])
        x = lp64[b if rows is None else int(rows[b]), :n]
        e = np.full(2 * L + 1, blank)
        e[1::2] = targets[b, :L].numpy()
        st = states[b, :n]
        assert (states[b, n:] == -1).all() and (st >= 0).all() and (st <= 2 * L).all()
        path = math.fsum(float(x[t, e[st[t]]]) for t in range(n))
        blanks = math.fsum(float(x[t, blank]) for t in range(n) if st[t] % 2 == 0)
        assert abs(score[b] - path) <= 1e-9 * (1 + abs(score[b])), (b, score[b], path)
        assert abs(score[b] - (logp[b, :L].sum() + blanks)) <= 1e-9 * (1 + abs(score[b])), (b, score[b], logp[b, :L].sum() + blanks)
        if nll and n > 0 and np.isfinite(x).all():
            loss = torch.nn.functional.ctc_loss(torch.from_numpy(x.copy())[:, None, :], targets[b:b + 1, :L], torch.tensor([n]),
                                                torch.tensor([L]), blank=blank, reduction="none")
            nll64 = float(loss[0])
            assert score[b] <= -nll64 * (1 - 1e-12) + 1e-9, (b, score[b], nll64)
        done += 1
    return done


def _check(name, kind="random", dtype=torch.float32, strided=False, seed=0):
    lp, targets, il, tl = _case(name, seed, kind)
    if dtype != torch.float32:
        lp = lp.to(dtype)
    dev = lp.to(DEV)
    if strided:                                                     # a view of a larger tensor: row, time and column offsets
        B, T, V = lp.shape
        big = torch.full((B + 1, T + 3, V + 5), float("nan"), dtype=dtype, device=DEV)
        big[1:, 2:T + 2, 3:V + 3] = dev
        dev = big[1:, 2:T + 2, 3:V + 3]
        assert not dev.is_contiguous() and dev.stride(2) == 1
    got = _run(dev, targets, il, tl)
    lp64 = lp.double().numpy()                                      # exact from fp32 and from bf16
    want = AR.align_batch(lp64, targets.numpy(), il.tolist(), tl.tolist())
    _same(got, want, f"{name}/{kind}/{dtype}")
    n0 = _cross_check(lp64, targets, il, tl, got, 0)
    return got, n0


@pytest.mark.parametrize("kind", ["random", "round"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_of_the_reference(name, kind):
    got, n0 = _check(name, kind)
    status = got[1].tolist()
    if name == "tiny_v2":
        assert status == [0, 0, 0, 0, 0, 1, 0, 1, 0, 0]            # "aa": 3 frames fit exactly, 2 cannot; n = 0 with L > 0 cannot
        assert got[2][4, :3].tolist() == [1, 2, 3] and got[0][6] == 0.0 and got[0][5] == -math.inf
    else:
        assert n0 >= 1 and n0 == status.count(0) and set(status) <= {0, 1}, status


@pytest.mark.parametrize("name", QUICK + ["s512", "v5000"])
def test_bf16_strided_view(name):
    got, n0 = _check(name, "random", torch.bfloat16, strided=True)
    assert n0 >= 1
    _check(name, "round", torch.float32, strided=True)


def _one_path(T, L, V, g):
    """A lattice with exactly one finite path: frame t admits the path's symbol alone."""
    y = torch.randint(1, V, (L,), generator=g)
    ext = [0]
    for v in y.tolist():
        ext += [v, 0]
    must = [2 * j + 1 for j in range(L)]                            # every label once; blanks where a repeat needs one, then the rest
    states = []
    for j, s in enumerate(must):
        if j and ext[s] == ext[s - 2]:
            states.append(s - 1)
        states.append(s)
    states = [0] * (T - len(states) - 1) + states + [2 * L]
    assert len(states) == T
    lp = torch.full((T, V), -math.inf)
    for t, s in enumerate(states):
        lp[t, ext[s]] = -float(torch.rand((), generator=g)) - 0.25
    return lp, y, states


def test_minus_infinity_columns_and_single_finite_path():
    g = torch.Generator().manual_seed(11)
    V, T, S = 7, 40, 12
    lp = torch.log_softmax(torch.randn(5, T, V, generator=g), dim=-1)
    targets = torch.full((5, S), V + 1, dtype=torch.int64)
    for b in range(5):
        targets[b] = torch.randint(1, V, (S,), generator=g)
    one, y, states = _one_path(T, S, V, g)
    lp[0], targets[0] = one, y
    lp[1][:, 3] = -math.inf                                          # a label column: infeasible if the target holds it
    lp[2][5:9, 0] = -math.inf                                        # blank forbidden for a while
    lp[3][:, 0] = -math.inf                                          # no blanks at all
    lp[4][:, 0] = -math.inf
    il = torch.tensor([T, T, T, T, S], dtype=torch.int32)
    tl = torch.tensor([S, S, S, S, S], dtype=torch.int32)
    targets[4] = torch.tensor([1, 2, 3, 4, 5, 6, 1, 2, 3, 4, 5, 6])   # T == L, no repeats: the diagonal is the only path
    lp[4, S:] = float("nan")
    got = _run(lp.to(DEV), targets, il, tl)
    lp64 = lp.double().numpy()
    _same(got, AR.align_batch(lp64, targets.numpy(), il.tolist(), tl.tolist()), "-inf")
    assert got[1][0] == 0 and got[2][0].tolist() == states
    assert got[1][4] == 0 and got[2][4, :S].tolist() == list(range(1, 2 * S, 2))
    y3 = targets[3].tolist()                                         # without blanks: feasible exactly when no label repeats at once
    assert int(got[1][3]) == (1 if any(a == b for a, b in zip(y3, y3[1:])) else 0)
    assert int(got[1][1]) == (1 if 3 in targets[1].tolist() else 0)
    assert _cross_check(lp64, targets, il, tl, got, 0, nll=False) >= 2


def test_nonzero_blank_index():
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(3)
    V, T, S, blank = 9, 30, 8, 4
    lp = torch.log_softmax(torch.randn(2, T, V, generator=g), dim=-1)
    targets = torch.tensor([[0, 1, 1, 8, 5, 5, 5, 3], [8, 8, 0, 2, 11, 11, 11, 11]])
    il, tl = torch.tensor([30, 22], dtype=torch.int32), torch.tensor([8, 4], dtype=torch.int32)
    lp[1, 22:] = float("nan")
    got = _run(lp.to(DEV), targets, il, tl, blank=blank)
    _same(got, AR.align_batch(lp.double().numpy(), targets.numpy(), il.tolist(), tl.tolist(), blank=blank), "blank 4")
    assert got[1].tolist() == [0, 0] and _cross_check(lp.double().numpy(), targets, il, tl, got, blank) == 2
    assert ops.ctc_align(lp.double().to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV), blank=blank)[0].cpu().equal(got[0])   # cast to fp32


def test_rows_share_frames():
    """rows with repeats and a permutation: utterance b reads log_probs row rows[b]; three rows serve five label sequences."""
    lp, targets, il, tl = _case("t33")
    lp = lp[:3]
    lp[:, :] = torch.where(torch.isnan(lp), torch.full_like(lp, -1.0), lp)      # all 33 frames usable by every sequence
    rows = torch.tensor([2, 0, 0, 1, 2], dtype=torch.int32)
    tg = torch.stack([targets[0], targets[1], targets[0], targets[2], targets[3]])
    tls = torch.tensor([20, 15, 20, 12, 20], dtype=torch.int32)
    ils = torch.tensor([33, 32, 33, 30, 33], dtype=torch.int32)
    got = _run(lp.to(DEV), tg, ils, tls, rows=rows)
    lp64 = lp.double().numpy()
    _same(got, AR.align_batch(lp64, tg.numpy(), ils.tolist(), tls.tolist(), rows=rows.tolist()), "rows")
    assert _cross_check(lp64, tg, ils, tls, got, 0, rows=rows.tolist()) == 5
    own = _run(lp.to(DEV)[[2, 0, 0, 1, 2]].contiguous(), tg, ils, tls)          # the same with the frames copied
    _same(got, own, "rows vs copies")
    bad = _run(lp.to(DEV), tg, ils, tls, rows=torch.tensor([2, 0, 3, -1, 2], dtype=torch.int32))
    assert bad[1].tolist() == [0, 0, 1, 1, 0]                        # a row outside log_probs: no alignment, nothing read


def test_nan_on_and_off_the_lattice():
    lp, targets, il, tl = _case("t33")
    for b in range(4):
        targets[b, :int(tl[b])] = torch.randint(1, 21, (int(tl[b]),), generator=torch.Generator().manual_seed(b))
    tl[3] = 10                                                       # 10 labels in 21 frames: feasible whatever repeats
    plain = _run(lp.to(DEV), targets, il, tl)
    assert plain[1].tolist() == [0, 0, 0, 0]
    off = lp.clone()
    off[:, :, 25:] = float("nan")                                    # columns outside {blank} + targets (labels are 1 .. 20)
    _same(_run(off.to(DEV), targets, il, tl), plain, "NaN off the lattice")
    for t, v in ((5, 0), (0, int(targets[1, 0])), (31, int(targets[1, 14]))):    # blank; the first label at frame 0; the last label at the last frame
        on = lp.clone()
        on[1, t, v] = float("nan")
        got = _run(on.to(DEV), targets, il, tl)
        assert got[1].tolist() == [0, 2, 0, 0] and math.isnan(float(got[0][1]))
        assert (got[2][1] == -1).all() and (got[3][1] == -1).all() and (got[4][1] == -1).all() and (got[5][1] == 0).all()
        _same(got, AR.align_batch(on.double().numpy(), targets.numpy(), il.tolist(), tl.tolist()), f"NaN at ({t}, {v})")
        for k in range(6):
            keep = [0, 2, 3]
            assert torch.equal(got[k][keep], plain[k][keep]), (NAMES[k], t, v)


@pytest.mark.parametrize("name", ["s33", "t33", "t1000"])
def test_alone_as_in_the_batch_and_twice_the_same(name):
    lp, targets, il, tl = _case(name, kind="round")
    dev = lp.to(DEV)
    got = _run(dev, targets, il, tl)
    _same(_run(dev, targets, il, tl), got, "second run")
    for b in range(lp.shape[0]):
        alone = _run(dev[b:b + 1], targets[b:b + 1], il[b:b + 1], tl[b:b + 1])
        _same(alone, [o[b:b + 1] for o in got], f"utterance {b} alone")


# ----------------------------------------------------------------------------------------------------------
# guard bands
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T, S", [(17, 3), (33, 33)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_bands(monkeypatch, T, S, dtype):
    """Outputs inside sentinels, log_probs a strided view inside NaN rows, columns and utterances, targets and lengths inside guard
    values that name poison (a label whose column is NaN, a length that reaches NaN frames / padding), the workspace a scratch."""
    import ctypes as ct
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    calls = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, fn, args, units=0: (calls.append((name, args)), real(name, fn, args, units))[1])
    V, B = 12, 3
    g = torch.Generator().manual_seed(T * 100 + S)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g), dim=-1).to(dtype)
    lp[:, :, V - 1] = float("nan")                                   # the guard label's column
    il = torch.tensor([T, T - 1, T // 2], dtype=torch.int32)         # (frames at and past n are NaN; the guard length is T)
    tl = torch.tensor([S, S - 1, min(S, T // 4)], dtype=torch.int32)
    targets = torch.full((B, S), V + 3, dtype=torch.int64)
    for b in range(B):
        y = torch.randperm(V - 2, generator=g)[:1] + 1
        seq = [(int(y) + k) % (V - 2) + 1 for k in range(int(tl[b]))]   # no repeats next to each other: S labels fit S frames
        targets[b, :int(tl[b])] = torch.tensor(seq, dtype=torch.int64)
        lp[b, int(il[b]):] = float("nan")
    lp, targets, il, tl = lp.to(DEV), targets.to(DEV), il.to(DEV), tl.to(DEV)
    a = N.CtcAlignArgs()
    a.batch, a.T, a.S = B, T, S
    nws = int(N.lib().cm_ctc_align_workspace_bytes(ct.byref(a)))
    shapes = dict(score=((B,), torch.float64), status=((B,), torch.int32), states=((B, T), torch.int32), starts=((B, S), torch.int32),
                  ends=((B, S), torch.int32), label_logp=((B, S), torch.float64))

    def run(L):
        x = L.cols(lp, align=2, rows=4)
        tg, n, k = L.ints(targets, V - 1), L.ints(il, T, unique=False), L.ints(tl, S, unique=False)
        bufs = {name: L.out(name, shape, dt, contiguous=True) for name, (shape, dt) in shapes.items()}
        bufs["workspace"] = L.scratch("workspace", nws // 4).view(torch.uint8)
        got = ops.ctc_align(x, tg, n, k, bufs=bufs)
        assert all(t is bufs[name] for t, name in zip(got, NAMES))
        name, args = calls[-1]
        assert name == "cm_ctc_align" and args.workspace_bytes == nws
        for f, t in dict(bufs, log_probs=x, targets=tg, input_lengths=n, target_lengths=k).items():
            assert getattr(args, f) == t.data_ptr(), f"{f}: the wrapper copied it"
    outs = G.two_step(run, DEV)
    assert outs["status"].tolist() == [0, 0, 0]
    want = AR.align_batch(lp.cpu().double().numpy(), targets.cpu().numpy(), il.tolist(), tl.tolist())
    _same([outs[n].cpu() for n in NAMES], want, "guarded")


# ----------------------------------------------------------------------------------------------------------
# CTCAligner, CTCBeamSearcher.search(text_frames=True), ConMambaASR.align
# ----------------------------------------------------------------------------------------------------------
def test_aligner_objects():
    from mamba_asr_amd.ctc_decode import CTCAligner
    vocab = ["<blank>", " ", "a", "b", "c", "<unk>"]
    al = CTCAligner(0, vocab)
    g = torch.Generator().manual_seed(9)
    lp = torch.log_softmax(torch.randn(3, 24, 6, generator=g), dim=-1)
    ids = [[1, 2, 3, 1, 1, 5, 4, 1, 2], [], [2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]]     # the third needs 25 frames
    out = al(lp.to(DEV), ids, lengths=[24, 10, 24])
    assert [o.status for o in out] == [0, 0, 1]
    st, score, states, starts, ends, logp = AR.align_one(lp[0].numpy(), ids[0], 0)
    o = out[0]
    assert o.score == score and o.tokens == ids[0] and o.token_frames == list(zip(starts.tolist(), ends.tolist())) and o.token_logp == logp.tolist()
    assert (o.words, o.word_frames, o.word_logp) == al.words(ids[0], starts.tolist(), ends.tolist(), logp.tolist())
    assert o.words == ["ab", "<unk>c", "a"] and o.word_frames[0] == (int(starts[1]), int(ends[2]))
    assert out[1].score == AR.align_one(lp[1, :10].numpy(), [], 0)[1] and out[1].tokens == [] and out[1].words == []
    assert out[2].score == -math.inf and out[2].tokens == [] and out[2].word_frames == []
    padded = torch.tensor([ids[0], [0] * 9, [2] * 9])
    again = al(lp.to(DEV), padded.to(DEV), torch.tensor([9, 0, 9]), wav_lens=torch.tensor([1.0, 10 / 24, 1.0]))
    assert again[0] == out[0] and again[1] == out[1] and again[2].status == 0
    bad = lp.clone()
    bad[0, 3, 0] = float("nan")
    with pytest.raises(ValueError, match="utterance 0"):
        al(bad.to(DEV), ids, lengths=[24, 10, 24])
    with pytest.raises(ValueError, match="1023"):
        al(lp.to(DEV), [[2] * 1024, [], []])


def _check_text_frames(s, lp, lengths, tokens, token_len, num_hyps):
    from mamba_asr_amd.ctc_decode import group_words
    plain = s(lp.to(DEV), lengths=lengths)
    assert all(h.text_frames is None for hs in plain for h in hs)
    hyps = s.search(lp.to(DEV), lengths=lengths, text_frames=True)
    assert [[(h.text, h.score, h.lm_score) for h in hs] for hs in hyps] == [[(h.text, h.score, h.lm_score) for h in hs] for hs in plain]
    words = 0
    for u, hs in enumerate(hyps):
        assert len(hs) == int(num_hyps[u])
        for h, hyp in enumerate(hs):
            spans = hyp.text_frames
            assert len(spans) == len(hyp.text.split()), (u, h, hyp.text, spans)
            flat = [x for span in spans for x in span]
            assert all(0 <= a < z <= lengths[u] for a, z in spans) and flat == sorted(flat)       # inside [0, n], ordered, disjoint
            tok = tokens[u, h, :int(token_len[u, h])].tolist()
            assert s.compose(tok) == hyp.text
            st, _, _, starts, ends, logp = AR.align_one(lp[u, :lengths[u]].double().numpy(), tok, s.blank_index)
            assert st == 0
            assert spans == group_words(tok, starts.tolist(), ends.tolist(), logp.tolist(), s.classes, s.clean)[1]
            words += len(spans)
    return hyps, words


def test_searcher_text_frames_topk3():
    import test_ctc_beam_stream_gpu as BS
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    s = CTCBeamSearcher(vocab_list=D.SPM_VOCAB, **dict(D.RECIPE, topk=3))
    lengths = [40, 0, 29]
    lp = torch.stack([D.competing(40, BS.V, 100 + b) for b in range(3)])
    lp[1] = float("nan")
    lp[2, 29:] = float("nan")
    tokens, token_len, _, num_hyps = BS._whole(s, torch.nan_to_num(lp, nan=-50.0), lengths)
    hyps, words = _check_text_frames(s, lp, lengths, tokens, token_len, num_hyps)
    assert [len(hs) for hs in hyps] == [3, 1, 3] and hyps[1][0].text_frames == [] and words >= 6


def test_searcher_text_frames_lm_fused(tmp_path):
    import ctc_lm_data as LD
    import test_ctc_lm_stream_gpu as LS
    path = LD.make_arpa(tmp_path / "m.arpa", seed=4, **LS.RICH)[0]
    s = LS._whole_searcher(path, **dict(D.RECIPE, topk=2))
    lengths = [40, 29]
    lp = LS._batch(D.competing, lengths, 40, 100)
    tokens, token_len, _, _, num_hyps = LS._whole(s, lp, lengths, width=40)
    hyps, words = _check_text_frames(s, lp, lengths, tokens, token_len, num_hyps)
    assert words >= 2 and hyps[0][0].lm_score != hyps[0][0].score


def test_asr_align():
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs
    from mamba_asr_amd.ctc_decode import CTCAligner
    ns = [16000, 9977]
    model = ConMambaASR(ASRConfig("align", num_encoder_layers=2)).to(DEV).eval()
    wav, ones = synthetic_wavs(2, ns[0], 7, DEV)
    with torch.no_grad():
        model.calibrate(wav, ones)
    wav[1, ns[1]:] = float("nan")
    vocab = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "<unk>", "-"]
    assert len(vocab) == model.cfg.output_neurons
    al = CTCAligner(0, vocab)
    ids = [[2, 3, 1, 4, 5, 6], [7, 1, 1, 8]]
    assert model.row_seconds == 0.04
    model.train()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = model.align(wav, torch.tensor(ns, device=DEV), ids, None, al)
    assert model.training                                            # the caller's mode is restored
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        enc, row_lens = model.encode(wav, torch.tensor(ns, device=DEV), ragged=True)
        lp = torch.log_softmax(model.ctc_lin(enc), dim=-1)
    assert list(row_lens) == [26, 16]
    want = al(lp, ids, lengths=row_lens)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.status == 0 and (g.score, g.tokens, g.token_frames, g.token_logp, g.words, g.word_frames, g.word_logp) == \
            (w.score, w.tokens, w.token_frames, w.token_logp, w.words, w.word_frames, w.word_logp)
        dur = ns[b] / 16000
        assert g.token_times == [(a * 0.04, min(z * 0.04, dur)) for a, z in w.token_frames]
        assert g.word_times == [(a * 0.04, min(z * 0.04, dur)) for a, z in w.word_frames]
        assert all(0 <= a < z <= dur for a, z in g.word_times) and len(g.word_times) == 2
        ref = AR.align_one(lp[b, :row_lens[b]].double().cpu().numpy(), ids[b], 0)
        assert g.score == ref[1] and g.token_frames == list(zip(ref[3].tolist(), ref[4].tolist()))
    assert got[1].token_times[-1][1] <= ns[1] / 16000 < 16 * 0.04    # the last row's nominal end lies past the audio: clipped
