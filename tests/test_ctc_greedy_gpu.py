"""cm_ctc_greedy on the GPU against tests/ctc_score_ref.py: all six outputs bit for bit (torch.equal-style array equality, exact
float64), on ragged batches at the sizes where the kernels change path -- V around a wave (63, 64, 65) and around the 16-byte
vectors (2, 31, 5000, 5001), T around the 16-frame tile, the 256-frame scan block and its carry (1000, 1025) -- with random,
rounded (ties), all-blank, one-token, alternating and -inf inputs, bf16 views with lp_ts > V at an odd element offset, NaN inside
and outside a length, guard bands, and through CTCGreedyDecoder against dataio.ctc_greedy_decode.

Frames at and past an utterance's length are NaN in every case: they may not be read."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_score_ref as SR  # noqa: E402
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("tokens", "token_len", "starts", "ends", "token_logp", "status")
VS = [2, 31, 63, 64, 65, 5000, 5001]
TS = [1, 15, 16, 17, 63, 64, 65, 1000, 1025]
KINDS = ["random", "round", "all_blank", "one_token", "token_blank", "token_token", "neg_inf"]


def _lengths(T):
    """Ragged: the whole row, nothing, about half, one short of the row."""
    return [T, 0, (T + 1) // 2, max(T - 1, 0)]


def _case(T, V, kind="random", seed=0, blank=0):
    """-> lp (4, T, V) float32 on the host, NaN at and past every length, and the lengths."""
    g = torch.Generator().manual_seed(seed * 7919 + T * 31 + V)
    lens = _lengths(T)
    B = len(lens)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * 2.0, dim=-1)
    tok = (blank + 1) % V
    if kind == "round":
        lp = torch.round(lp)                                         # small integers: ties in most frames
    elif kind == "all_blank":
        lp[:, :, blank] = 1.0
    elif kind == "one_token":
        lp[:, :, tok] = 1.0
    elif kind == "token_blank":
        lp[:, 0::2, tok] = 1.0
        lp[:, 1::2, blank] = 1.0
    elif kind == "token_token":
        lp[:, 0::2, tok] = 1.0
        lp[:, 1::2, (tok + 1) % V if (tok + 1) % V != blank else (tok + 2) % V] = 1.0
    elif kind == "neg_inf":
        lp[:, 0::3] = -math.inf                                      # whole frames of -inf: index 0
        lp[:, 1::3, : V // 2] = -math.inf                            # half frames: the maximum lies in the upper half
    for b, n in enumerate(lens):
        lp[b, n:] = float("nan")
    return lp, lens


def _run(lp, lens, blank=0, bufs=None):
    from mamba_asr_amd import ops
    out = ops.ctc_greedy(lp, torch.tensor(lens, dtype=torch.int32, device=DEV), blank=blank, bufs=bufs)
    torch.cuda.synchronize()
    return [o.cpu() for o in out]


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g = g.numpy() if torch.is_tensor(g) else g
        w = w.numpy() if torch.is_tensor(w) else w
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what}: {name} differs at {len(bad)} place(s); first {tuple(bad[0])}: {g[tuple(bad[0])]!r} vs {w[tuple(bad[0])]!r}")


def _check(T, V, kind="random", dtype=torch.float32, strided=False, blank=0, seed=0):
    lp, lens = _case(T, V, kind, seed, blank)
    lp = lp.to(dtype)
    dev = lp.to(DEV)
    if strided:                                                      # a view of a larger tensor: lp_ts > V, an odd element offset
        B = lp.shape[0]
        big = torch.full((B + 1, T + 2, V + 6), float("nan"), dtype=dtype, device=DEV)
        big[1:, 1:T + 1, 3:V + 3] = dev
        dev = big[1:, 1:T + 1, 3:V + 3]
        assert not dev.is_contiguous() and dev.stride(2) == 1 and dev.stride(1) > V and (T % 2 == 0 or dev.storage_offset() % 2 == 1)
    got = _run(dev, lens, blank)
    want = SR.greedy_batch(lp.double().numpy(), lens, blank, fast=V > 100)      # exact from fp32 and from bf16
    _same(got, want, f"T={T} V={V} {kind} {dtype} strided={strided}")
    assert got[5].tolist() == [0, 0, 0, 0] and got[1][1] == 0
    return got, lp, lens


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("V", VS[:5])
def test_every_vocabulary_width(V, dtype):
    got, _, _ = _check(65, V, "random", dtype)
    assert int(got[1].sum()) > 0
    _check(17, V, "round", dtype, seed=1)


@pytest.mark.parametrize("T", TS)
def test_every_length(T):
    got, _, _ = _check(T, 31, "random")
    _check(T, 31, "round", torch.bfloat16, seed=2)
    if T >= 15:
        assert int(got[1][0]) > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("T, V", [(17, 31), (65, 65)])
def test_every_kind_of_input(T, V, kind):
    got, _, lens = _check(T, V, kind)
    tokens, token_len, starts, ends, logp, _ = got
    n = lens[0]
    if kind == "all_blank":
        assert token_len.tolist() == [0, 0, 0, 0] and (tokens == -1).all() and (logp == 0).all()
    elif kind == "one_token":
        assert token_len.tolist() == [1, 0, 1, 1] and tokens[0, 0] == 1 and (starts[0, 0], ends[0, 0]) == (0, n) and logp[0, 0] == float(n)
    elif kind == "token_blank":
        assert token_len[0] == (n + 1) // 2 and (tokens[0, :token_len[0]] == 1).all() and starts[0, :3].tolist() == [0, 2, 4]
    elif kind == "token_token":
        assert token_len[0] == n and ends[0, :n].tolist() == list(range(1, n + 1))
    elif kind == "neg_inf":
        assert (tokens[0, :token_len[0]] != 0).all()
        got1, _, _ = _check(T, V, kind, blank=1)                     # blank 1: the all -inf frames decode to token 0, log-probability -inf
        assert (got1[0][0, :got1[1][0]] == 0).any() and (got1[4][0] == -math.inf).any()
    if kind in ("round", "neg_inf"):
        _check(T, V, kind, torch.bfloat16)


@pytest.mark.parametrize("V", [63, 64, 65])
def test_bf16_strided_view_at_an_odd_offset(V):
    _check(33, V, "random", torch.bfloat16, strided=True)
    _check(33, V, "round", torch.float32, strided=True, seed=3)


def test_largest_shapes_run_once():
    got, _, _ = _check(1025, 5001, "random", torch.bfloat16, strided=True)    # odd width, odd offset: head, vectors and tail
    assert int(got[1][0]) > 256                                               # the compaction crosses scan blocks
    _check(1000, 5000, "round", torch.float32)


def test_nan_inside_a_length_marks_that_row_only():
    lp, lens = _case(65, 65)
    plain = _run(lp.to(DEV), lens)
    for t, v in ((0, 0), (31, 64), (lens[2] - 1, 17)):
        bad = lp.clone()
        bad[2, t, v] = float("nan")
        got = _run(bad.to(DEV), lens)
        assert got[5].tolist() == [0, 0, 2, 0] and got[1][2] == 0
        assert (got[0][2] == -1).all() and (got[2][2] == -1).all() and (got[3][2] == -1).all() and (got[4][2] == 0).all()
        _same(got, SR.greedy_batch(bad.double().numpy(), lens, 0), f"NaN at ({t}, {v})")
        for k in range(6):
            assert torch.equal(got[k][[0, 1, 3]], plain[k][[0, 1, 3]]), NAMES[k]


def test_twice_the_same_and_alone_as_in_the_batch():
    lp, lens = _case(65, 31, "round")
    dev = lp.to(DEV)
    got = _run(dev, lens)
    _same(_run(dev, lens), got, "second run")
    for b in range(4):
        alone = _run(dev[b:b + 1], lens[b:b + 1])
        _same(alone, [o[b:b + 1] for o in got], f"utterance {b} alone")


@pytest.mark.parametrize("T, V", [(17, 31), (65, 65)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_guard_bands(monkeypatch, T, V, dtype):
    """Outputs inside sentinels, log_probs a strided view inside NaN rows, columns and utterances, the lengths inside guard values
    that reach NaN frames, the workspace a scratch."""
    import ctypes as ct
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    calls = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, fn, args, units=0: (calls.append((name, args)), real(name, fn, args, units))[1])
    lens = [T, T - 1, (T + 1) // 2, 1]
    lp = torch.log_softmax(torch.randn(4, T, V, generator=torch.Generator().manual_seed(T + V)) * 2.0, dim=-1)
    for b, n in enumerate(lens):
        lp[b, n:] = float("nan")
    lp, il = lp.to(dtype).to(DEV), torch.tensor(lens, dtype=torch.int32, device=DEV)
    a = N.CtcGreedyArgs()
    a.batch, a.T, a.V = 4, T, V
    nws = int(N.lib().cm_ctc_greedy_workspace_bytes(ct.byref(a)))
    assert nws == 4 * T * 4
    shapes = dict(tokens=((4, T), torch.int32), token_len=((4,), torch.int32), starts=((4, T), torch.int32), ends=((4, T), torch.int32),
                  token_logp=((4, T), torch.float64), status=((4,), torch.int32))

    def run(L):
        x = L.cols(lp, align=2, rows=4)
        n = L.ints(il, T, unique=False)
        bufs = {name: L.out(name, shape, dt, contiguous=True) for name, (shape, dt) in shapes.items()}
        bufs["workspace"] = L.scratch("workspace", nws // 4).view(torch.uint8)
        got = ops.ctc_greedy(x, n, bufs=bufs)
        assert all(t is bufs[name] for t, name in zip(got, NAMES))
        name, args = calls[-1]
        assert name == "cm_ctc_greedy" and args.workspace_bytes == nws
        for f, t in dict(bufs, log_probs=x, input_lengths=n).items():
            assert getattr(args, f) == t.data_ptr(), f"{f}: the wrapper copied it"
    outs = G.two_step(run, DEV)
    want = SR.greedy_batch(lp.cpu().double().numpy(), lens, 0)
    _same([outs[n].cpu() for n in NAMES], want, "guarded")


def test_decoder_object_against_dataio_and_the_host_path():
    from mamba_asr_amd import dataio
    from mamba_asr_amd.ctc_decode import CTCGreedyDecoder
    vocab = ["<blank>", " "] + [chr(ord("a") + i) for i in range(26)] + ["'", "<unk>", "-"]
    dec = CTCGreedyDecoder(0, vocab)
    g = torch.Generator().manual_seed(4)
    for dtype in (torch.float32, torch.bfloat16):
        lp = torch.log_softmax(torch.randn(5, 80, len(vocab), generator=g) * 3.0, dim=-1).to(dtype)
        wav_lens = torch.tensor([1.0, 0.5, 0.26, 0.0, 0.99])
        got = dec.tokens(lp.to(DEV), wav_lens.to(DEV))
        # dataio's torch.argmax on the host returns the first maximal index; on the device torch leaves ties open (bf16 has them)
        assert got == dataio.ctc_greedy_decode(lp.float(), wav_lens, 0) == dec.tokens(lp, wav_lens) and got[3] == [] and got[0]
        if dtype == torch.float32:
            assert got == dataio.ctc_greedy_decode(lp.to(DEV), wav_lens.to(DEV), 0)
        hyps, host = dec(lp.to(DEV), wav_lens.to(DEV)), dec(lp, wav_lens)
        assert hyps == host                                          # tokens, text, word frames and the float64 score, bit for bit
        assert hyps[0].text == dec.compose(got[0]) and len(hyps[0].text_frames) == len(hyps[0].text.split())
    bad = lp.clone()
    bad[1, 5, 7] = float("nan")
    with pytest.raises(ValueError, match="utterance 1"):
        dec.tokens(bad.to(DEV), wav_lens)
    with pytest.raises(RuntimeError, match="GPU only"):
        from mamba_asr_amd import ops
        ops.ctc_greedy(lp, torch.tensor([1] * 5))
