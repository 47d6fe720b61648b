"""The causal ConMamba encoder streamed with per-slot lengths (GPU): forward_streaming(..., lens=...) on the golden
case of tests/test_streaming_encoder_gpu.py -- 2 layers, d_model 256, x (4, 96, 256) -- where every slot follows ITS OWN chunking
through one sequence of batched calls: (96), 16 x 6, (1, 2, 3, 5, 29, 31, 25), and (40, 56) with idle calls in between.

Call width.  Chunks of 96 and 56 rows do not fit a call of t = 40 rows, so the sequence runs twice: at t = 96 with the chunkings as
listed, and at t = 40 with every chunk above 40 rows cut into pieces of at most 40 (96 -> 40, 40, 16; 56 -> 40, 16), which adds the
case of a slot that fills the call while the others do not.  The reference is the same in both: the whole-utterance fused run, and
the comparison is torch.equal.  In every call the rows of src at and past lens[b] are NaN."""
import pytest
import torch

import streaming_ref as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
CHUNKINGS = [(96,), (16,) * 6, (1, 2, 3, 5, 29, 31, 25), (40, 0, 0, 56)]
LAYER = ["cm_ffn_fused", "cm_conv_xproj_uni_slots", "cm_scan_cl_fwd_slots", "cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu_causal_slots", "cm_ffn_fused"]


@pytest.fixture(scope="module")
def case():
    from mamba_asr_amd import fused
    enc, x = R.causal_large()
    enc, x = enc.to("cuda"), x.to("cuda")
    with torch.no_grad():
        whole = fused.encoder_forward(enc, x, dtype=BF16, streams=1)
    return enc, x, whole


def cut(chunks, t):
    """The chunking with every chunk above t rows cut into pieces of at most t; idle calls (0) stay."""
    out = []
    for n in chunks:
        out += [0] if n == 0 else [min(t, n - i) for i in range(0, n, t)]
    return out


def schedule(chunkings, t):
    """-> the calls as tuples of per-slot lengths; a slot that has finished idles."""
    per_slot = [cut(c, t) for c in chunkings]
    calls = max(len(c) for c in per_slot)
    return [tuple(c[i] if i < len(c) else 0 for c in per_slot) for i in range(calls)]


def run_slots(enc, xs, calls, t, ctx, resets=None):
    """xs: per slot its utterance (T_b, D).  Feeds every slot its next lens[b] rows per call, NaN behind them -> per slot the
    concatenated valid output rows.  ``resets``: {call index: [slots]} reset before that call, their utterance starting over from
    ``xs_after`` = resets["xs"][slot]."""
    B, D = len(xs), xs[0].shape[1]
    pos, outs = [0] * B, [[] for _ in range(B)]
    xs = list(xs)
    with torch.no_grad():
        for i, call in enumerate(calls):
            for slot in (resets or {}).get(i, []):
                ctx.reset(rows=[slot])
                xs[slot], pos[slot], outs[slot] = resets["xs"][slot], 0, []
            src = torch.full((B, t, D), NAN, device="cuda")
            for b, n in enumerate(call):
                src[b, :n] = xs[b][pos[b]:pos[b] + n]
            out, none = enc.forward_streaming(src, ctx, lens=torch.tensor(call, dtype=torch.int32, device="cuda"))
            assert none is None and out.shape == (B, t, D) and out.dtype == torch.float32
            for b, n in enumerate(call):
                outs[b].append(out[b, :n])
                pos[b] += n
    return [torch.cat(o) for o in outs], pos


@pytest.mark.parametrize("t", [96, 40])
def test_every_slot_at_its_own_pace_equals_the_whole_utterance(case, t):
    enc, x, whole = case
    calls = schedule(CHUNKINGS, t)
    if t == 96:                                                             # the chunkings as listed, one chunk per call
        assert [tuple(c) for c in zip(*calls)][:3] == [(96,) + (0,) * 6, (16,) * 6 + (0,), (1, 2, 3, 5, 29, 31, 25)] and len(calls) == 7
    assert all(max(c) <= t for c in calls) and any(0 in c and max(c) > 0 for c in calls)
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    got, pos = run_slots(enc, [x[b] for b in range(4)], calls, t, ctx)
    assert pos == [96] * 4
    for b in range(4):
        err = (got[b] - whole[b]).abs()
        print(f"t {t}, slot {b} {CHUNKINGS[b]}: torch.equal {torch.equal(got[b], whole[b])}, max|diff| {float(err.max()):.3e}")
    for b in range(4):
        assert torch.equal(got[b], whole[b]), f"slot {b} (chunking {CHUNKINGS[b]}) at call width {t}"


def test_a_slot_reset_mid_stream_equals_its_utterance_alone(case):
    """Slot 1 is reset before call 2 and restarted on another utterance in chunks of its own while the others continue: its rows are
    that utterance streamed alone (lock step, batch 1, the same chunks), the others' are theirs."""
    enc, x, whole = case
    new = R._synth().synth_input("g_causal.new", (1, 64, 256), 256).to("cuda")
    t = 40
    calls = [(40, 16, 1, 40), (40, 16, 2, 0), (16, 7, 3, 0), (0, 33, 5, 40), (0, 0, 29, 16), (0, 24, 31, 0), (0, 0, 25, 0)]
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    got, pos = run_slots(enc, [x[b] for b in range(4)], calls, t, ctx, resets={2: [1], "xs": {1: new[0]}})
    assert pos == [96, 64, 96, 96]
    for b in (0, 2, 3):
        assert torch.equal(got[b], whole[b]), f"slot {b} noticed the reset of slot 1"
    alone_ctx = enc.make_streaming_context(None, batch_size=1, dtype=BF16)
    outs, t0 = [], 0
    with torch.no_grad():
        for n in (7, 33, 24):
            outs.append(enc.forward_streaming(new[:, t0:t0 + n], alone_ctx)[0])
            t0 += n
    alone = torch.cat(outs, dim=1)[0]
    err = (got[1] - alone).abs()
    print(f"slot 1 after its reset vs the utterance streamed alone: max|diff| {float(err.max()):.3e}")
    assert torch.equal(got[1], alone), "the reset left something of the old utterance in slot 1, or the neighbours reached it"


def test_idle_calls_leave_every_state_tensor_as_it_was(case):
    """lens = 0 for every slot, twice in a row (two buffer swaps): ssm_state, conv_state and dw_state of every layer keep their bits,
    although src is NaN throughout."""
    enc, x, whole = case
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    zero = torch.zeros(4, dtype=torch.int32, device="cuda")
    with torch.no_grad():
        enc.forward_streaming(x[:, :37], ctx)                                   # every state non-trivial
        before = [(l.ssm_state.clone(), l.conv_state.clone(), l.dw_state.clone()) for l in ctx.layers]
        assert all(float(t.abs().max()) > 0 for s in before for t in s)
        for _ in range(2):
            enc.forward_streaming(torch.full((4, 40, 256), NAN, device="cuda"), ctx, lens=zero)
            for l, s in zip(ctx.layers, before):
                assert torch.equal(l.ssm_state, s[0]) and torch.equal(l.conv_state, s[1]) and torch.equal(l.dw_state, s[2])
        out, _ = enc.forward_streaming(x[:, 37:], ctx)                          # and the stream goes on as if nothing had happened
    assert torch.equal(out, whole[:, 37:])


def test_route_of_a_per_slot_bf16_chunk(case, monkeypatch):
    """The same six launches per layer as the lock-step route, three of them the per-slot entry points: no library GEMM inside a
    layer, no torch.cat of history rows, no host synchronisation (torch's sync debug mode raises on one)."""
    from mamba_asr_amd import fused, ops
    enc, x, whole = case
    calls = {"gemm": 0, "cat": 0}

    def counted(name, key):
        real = getattr(fused, name) if key == "gemm" else torch.cat

        def f(*a, **k):
            calls[key] += 1
            return real(*a, **k)
        return f

    for name in ("_out_proj", "_in_proj", "_ffn"):
        monkeypatch.setattr(fused, name, counted(name, "gemm"))
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    lens = torch.tensor([16, 0, 7, 40], dtype=torch.int32, device="cuda")
    src = x[:, :40].contiguous()
    with torch.no_grad():
        enc.forward_streaming(src, ctx, lens=lens)                              # caches, packed weights
    monkeypatch.setattr(torch, "cat", counted("cat", "cat"))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with torch.no_grad():
            enc.forward_streaming(src, ctx, lens=lens)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            enc.forward_streaming(src, ctx, lens=lens)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    print("launches of one per-slot bf16 chunk:", names)
    assert names == LAYER * 2, names
    assert calls == {"gemm": 0, "cat": 0}, calls


def test_lens_is_checked(case):
    enc, x, whole = case
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=BF16)
    with torch.no_grad():
        for bad in (torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(3, dtype=torch.int32, device="cuda"),
                    torch.zeros(4, dtype=torch.int32), [1, 2, 3, 4]):
            with pytest.raises(RuntimeError, match="lens must be a contiguous int32 tensor"):
                enc.forward_streaming(x[:, :8], ctx, lens=bad)


def test_fp32_generic_route_against_lock_step_alone(case):
    """fp32 takes the generic route (histories gathered per slot in torch, the scan through cm_scan_cl_fwd_slots): every slot against the
    lock-step generic route on that slot alone, batch 1, the same chunks.  Bound: rtol 1e-5, atol 1e-5 -- the project's bound for the same
    fp32 operations at another batch size (tests/test_streaming_encoder_gpu.py, the prefix-causal check)."""
    enc, x, whole = case
    t = 40
    calls = schedule(CHUNKINGS, t)
    ctx = enc.make_streaming_context(None, batch_size=4, dtype=torch.float32)
    got, pos = run_slots(enc, [x[b] for b in range(4)], calls, t, ctx)
    assert pos == [96] * 4
    for b in range(4):
        alone = enc.make_streaming_context(None, batch_size=1, dtype=torch.float32)
        outs, t0 = [], 0
        with torch.no_grad():
            for n in (n for n in cut(CHUNKINGS[b], t) if n):
                outs.append(enc.forward_streaming(x[b:b + 1, t0:t0 + n], alone)[0])
                t0 += n
        want = torch.cat(outs, dim=1)[0]
        print(f"fp32 generic, slot {b}: max|diff| {float((got[b] - want).abs().max()):.3e}")
        torch.testing.assert_close(got[b], want, rtol=1e-5, atol=1e-5)
