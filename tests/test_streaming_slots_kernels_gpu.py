"""The three time-mixing kernels of a streamed causal layer with per-slot lengths (GPU): cm_conv_xproj_uni_slots,
cm_scan_cl_fwd_slots and cm_glu_dwconv_ln_gelu_causal_slots against the lock-step entry point run on each slot ALONE with
t = lens[b], bit for bit (torch.equal): the valid output rows, the new row histories, the scan state.

B = 4, t = 40, bf16, d_model 256 (d_inner 512).  Four chained calls -- each starts from the histories / state the one before left --
whose lengths cover {0, 1, 2, 3} (the 3-row conv history edge), {15, 16, 17} (the scan's 16-step block and the conv's 16-step tile),
{29, 30, 31} (the 30-row depthwise history edge, next to the 32-step tile) and 40 (the whole chunk, a ragged second tile); the last
call idles a slot that HAS a history and feeds a full chunk behind short ones.

Modes: "alone" as above; "nan": every input row at and past lens[b] is NaN, and the valid rows, histories and state keep the plain
launch's bits; "guards" (tests/guard_bands.py): outputs, histories and state inside sentinels, inputs inside NaN, same bits, nothing
outside written."""
import functools

import pytest
import torch

import guard_bands as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
TT = G.TIME_TILE
COLS = dict(rows=TT, left=G.LEFT, right=G.RIGHT)
NAN = float("nan")
B, T, D, E, K = 4, 40, 256, 512, 31
LENS = [(0, 1, 2, 3), (15, 16, 17, 40), (29, 30, 31, 40), (40, 0, 31, 16)]
MODES = ["alone", "nan", "guards"]


assert {0, 1, 2, 3, 15, 16, 17, 29, 30, 31, 40} <= {n for call in LENS for n in call}, "the lengths must cover every edge"
assert all(len(call) == B and max(call) <= T for call in LENS)


def dev(t):
    return t.to(DEV)


def lens_of(call):
    return torch.tensor(call, dtype=torch.int32, device=DEV)


def nan_behind(t, call):
    """t (B, T, W) with every row at and past call[b] NaN."""
    t = t.clone()
    for b, n in enumerate(call):
        t[b, n:] = NAN
    return t


def same_valid(got, want, call, name):
    for b, n in enumerate(call):
        assert torch.equal(got[b, :n], want[b, :n]), f"{name}: slot {b}, rows [0, {n}) changed"


def guarded_run(run, plain):
    guard = G.Launch(True, DEV)
    run(guard)
    torch.cuda.synchronize()
    guard.g.check(plain)


# ---------------------------------------------------------------------------------------------------- cm_conv_xproj_uni_slots
@functools.lru_cache(maxsize=None)
def conv_case():
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(4101)
    xz = [dev(torch.randn(B, T, 2 * E, generator=g).to(BF16)) for _ in LENS]     # x is the first half of [x | z] rows, as in the encoder
    w, bias = dev(torch.randn(E, 4, generator=g) * 0.5), dev(torch.randn(E, generator=g) * 0.1)
    wxp = ops.PackedWeight(dev((torch.randn(48, E, generator=g) / E ** 0.5).to(BF16)))
    return dict(xz=xz, w=w, bias=bias, wxp=wxp)


def conv_slots(c, xz, hist, lens):
    from mamba_asr_amd import ops

    def run(L):
        x = L.cols(xz, dead=(E, 2 * E))[:, :, :E]
        ops.conv_xproj_uni(x, L.vec(c["w"]), L.vec(c["bias"]), c["wxp"], out=L.out("u", (B, T, E), BF16, **COLS),
                           xdbl=L.out("xdbl", (B, T, 48), BF16, **COLS), x_hist=L.flat(hist, 3),
                           x_hist_out=L.out("x_hist_out", (B, 3, E), BF16, rows=G.ROW_TILE, contiguous=True), lens=lens)
    return run


@pytest.mark.parametrize("mode", MODES)
def test_conv_xproj_uni_slots(mode):
    from mamba_asr_amd import ops
    c = conv_case()
    hist = torch.zeros(B, 3, E, dtype=BF16, device=DEV)
    for xz, call in zip(c["xz"], LENS):
        plain = G.Launch(False, DEV)
        conv_slots(c, xz, hist, lens_of(call))(plain)
        out = plain.outs
        if mode == "alone":
            for b, n in enumerate(call):
                if n == 0:
                    assert torch.equal(out["x_hist_out"][b], hist[b]), f"slot {b} idles: its history must be carried into the spare"
                    continue
                u1, h1 = torch.empty(1, n, E, dtype=BF16, device=DEV), torch.empty(1, 3, E, dtype=BF16, device=DEV)
                x1 = ops.conv_xproj_uni(xz[b:b + 1, :n, :E], c["w"], c["bias"], c["wxp"], out=u1, x_hist=hist[b:b + 1].contiguous(), x_hist_out=h1)
                assert torch.equal(out["u"][b, :n], u1[0]), f"u, slot {b}, lens {n}"
                assert torch.equal(out["xdbl"][b, :n], x1[0]), f"xdbl, slot {b}, lens {n}"
                assert torch.equal(out["x_hist_out"][b], h1[0]), f"x_hist_out, slot {b}, lens {n}"
        elif mode == "nan":
            poisoned = G.Launch(False, DEV)
            conv_slots(c, nan_behind(xz, call), hist, lens_of(call))(poisoned)
            same_valid(poisoned.outs["u"], out["u"], call, "u")
            same_valid(poisoned.outs["xdbl"], out["xdbl"], call, "xdbl")
            assert torch.equal(poisoned.outs["x_hist_out"], out["x_hist_out"]), "rows at and past lens[b] reached x_hist_out"
        else:
            guarded_run(conv_slots(c, xz, hist, lens_of(call)), out)
        hist = out["x_hist_out"]


def test_conv_xproj_uni_slots_clamps_and_refuses():
    """lens above t is t, below 0 is 0 (clamped on the device); aliased histories are refused before launch."""
    from mamba_asr_amd import ops
    c = conv_case()
    xz = c["xz"][0]
    hist = dev(torch.randn(B, 3, E, generator=torch.Generator().manual_seed(5)).to(BF16))
    a, b_ = G.Launch(False, DEV), G.Launch(False, DEV)
    conv_slots(c, xz, hist, lens_of((T + 7, -3, T, 0)))(a)
    conv_slots(c, xz, hist, lens_of((T, 0, T, 0)))(b_)
    for k in a.outs:
        assert torch.equal(a.outs[k], b_.outs[k]), k
    keep = hist.clone()
    with pytest.raises(RuntimeError, match="x_hist"):
        ops.conv_xproj_uni(xz[:, :, :E], c["w"], c["bias"], c["wxp"], out=torch.empty(B, T, E, dtype=BF16, device=DEV), x_hist=hist, x_hist_out=hist,
                           lens=lens_of((1, 2, 3, 4)))
    torch.cuda.synchronize()
    assert torch.equal(hist, keep)


# ------------------------------------------------------------------------------------------------------- cm_scan_cl_fwd_slots
@functools.lru_cache(maxsize=None)
def scan_case():
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(4102)
    rank = 9
    xz = [dev(torch.randn(B, T, 2 * E, generator=g).to(BF16)) for _ in LENS]     # z is the second half
    u = [dev(torch.randn(B, T, E, generator=g).to(BF16)) for _ in LENS]
    xd = []
    for _ in LENS:
        t = torch.randn(B, T, 48, generator=g)
        t[:, :, rank:16] = 0.0
        xd.append(dev(t.to(BF16)))
    A = dev(-torch.exp(torch.randn(E, 16, generator=g) * 0.3))
    W = ops.pad_dt_weight(dev(torch.randn(E, rank, generator=g) * 0.3))
    Dv, bias = dev(torch.randn(E, generator=g)), dev(torch.randn(E, generator=g) - 1)
    return dict(xz=xz, u=u, xd=xd, A=A, W=W, D=Dv, bias=bias)


def scan_dir(c, u, xd, out, state, vec=lambda t: t):
    return dict(u=u, xdbl=xd, A=vec(c["A"]), D=vec(c["D"]), delta_bias=vec(c["bias"]), dt_weight=vec(c["W"]), out=out, h0=state, h_last=state)


def scan_slots(c, xz, u, xd, state, lens):
    from mamba_asr_amd import ops

    def run(L):
        st = L.out("state", (B, E, 16), F32, fill=state, rows=E, contiguous=True)          # h0 and h_last: the streamed state, in place
        y = L.out("y", (B, T, E), BF16, fill=0.0, **COLS)                                    # rows at and past lens[b] are not written
        ops.scan_cl_fwd([scan_dir(c, L.cols(u), L.cols(xd), y, st, L.vec)], z=L.cols(xz, dead=(0, E))[:, :, E:], delta_softplus=True,
                        time_chunks=1, lens=lens)
    return run


@pytest.mark.parametrize("mode", MODES)
def test_scan_cl_fwd_slots(mode):
    from mamba_asr_amd import ops
    c = scan_case()
    state = torch.zeros(B, E, 16, dtype=F32, device=DEV)
    for xz, u, xd, call in zip(c["xz"], c["u"], c["xd"], LENS):
        plain = G.Launch(False, DEV)
        scan_slots(c, xz, u, xd, state, lens_of(call))(plain)
        out = plain.outs
        for b, n in enumerate(call):
            assert not bool(out["y"][b, n:].any()), f"slot {b}: an output row at or past lens {n} was written"
        if mode == "alone":
            for b, n in enumerate(call):
                if n == 0:
                    assert torch.equal(out["state"][b], state[b]), f"slot {b} idles: its state must pass through"
                    continue
                s1, y1 = state[b:b + 1].clone(), torch.empty(1, n, E, dtype=BF16, device=DEV)
                ops.scan_cl_fwd([scan_dir(c, u[b:b + 1, :n], xd[b:b + 1, :n], y1, s1)], z=xz[b:b + 1, :n, E:], delta_softplus=True, time_chunks=1)
                assert torch.equal(out["y"][b, :n], y1[0]), f"y, slot {b}, lens {n}"
                assert torch.equal(out["state"][b], s1[0]), f"state, slot {b}, lens {n}"
        elif mode == "nan":
            poisoned = G.Launch(False, DEV)
            scan_slots(c, nan_behind(xz, call), nan_behind(u, call), nan_behind(xd, call), state, lens_of(call))(poisoned)
            assert torch.equal(poisoned.outs["y"], out["y"]), "rows at and past lens[b] reached an output row"
            assert torch.equal(poisoned.outs["state"], out["state"]), "rows at and past lens[b] reached the state"
        else:
            guarded_run(scan_slots(c, xz, u, xd, state, lens_of(call)), out)
        state = out["state"]
    assert bool(torch.isfinite(state).all()) and float(state.abs().max()) > 0


# ----------------------------------------------------------------------------------------- cm_glu_dwconv_ln_gelu_causal_slots
DW = [(BF16, 256, True), (BF16, 256, False), (F32, 64, False)]      # the encoder's launch (rows kernel + Linear); without; the generic kernel


@functools.lru_cache(maxsize=None)
def dw_case(dtype, d, lin):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(4103 + d + lin)
    inp = [dev(torch.randn(B, T, d, generator=g).to(dtype)) for _ in LENS]        # gated rows (glu_done), as cm_ln_pw_glu leaves them
    w, bs = torch.randn(d, K, generator=g) / 6, torch.randn(d, generator=g) * 0.1
    lg, lb = 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    c = dict(inp=inp, w=dev(w), wt=dev(w.t().contiguous()), bs=dev(bs), lg=dev(lg), lb=dev(lb))
    if lin:
        c["lwp"] = ops.PackedWeight(dev((torch.randn(d, d, generator=g) / 16).to(BF16)))
        c["lbias"] = dev(torch.randn(d, generator=g) * 0.1)
    return c


def dw_launch(c, inp, vec=lambda t: t, **kw):
    from mamba_asr_amd import ops
    if "lwp" in c:
        kw.update(lin_w=c["lwp"], lin_b=vec(c["lbias"]))
    return ops.glu_dwconv_ln_gelu(inp, vec(c["w"]), vec(c["bs"]), vec(c["lg"]), vec(c["lb"]), 1e-5, weight_t=vec(c["wt"]), glu_done=True, causal=True, **kw)


def dw_slots(c, inp, hist, lens, dtype, d):
    def run(L):
        dw_launch(c, L.flat(inp, TT), L.vec, hist=L.flat(hist, TT), hist_out=L.out("hist_out", (B, K - 1, d), dtype, rows=TT, contiguous=True),
                  out=L.out("out", (B, T, d), dtype, rows=TT, contiguous=True), lens=lens)
    return run


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype,d,lin", DW, ids=["bf16_d256_lin", "bf16_d256", "fp32_d64_generic"])
def test_glu_dwconv_causal_slots(dtype, d, lin, mode):
    c = dw_case(dtype, d, lin)
    hist = torch.zeros(B, K - 1, d, dtype=dtype, device=DEV)
    for inp, call in zip(c["inp"], LENS):
        plain = G.Launch(False, DEV)
        dw_slots(c, inp, hist, lens_of(call), dtype, d)(plain)
        out = plain.outs
        if mode == "alone":
            for b, n in enumerate(call):
                if n == 0:
                    assert torch.equal(out["hist_out"][b], hist[b]), f"slot {b} idles: its history must be carried into the spare"
                    continue
                h1 = torch.empty(1, K - 1, d, dtype=dtype, device=DEV)
                o1 = dw_launch(c, inp[b:b + 1, :n], hist=hist[b:b + 1].contiguous(), hist_out=h1)
                assert torch.equal(out["out"][b, :n], o1[0]), f"out, slot {b}, lens {n}"
                assert torch.equal(out["hist_out"][b], h1[0]), f"hist_out, slot {b}, lens {n}"
                assert torch.equal(h1[0], torch.cat([hist[b], inp[b, :n]])[-(K - 1):])
        elif mode == "nan":
            poisoned = G.Launch(False, DEV)
            dw_slots(c, nan_behind(inp, call), hist, lens_of(call), dtype, d)(poisoned)
            same_valid(poisoned.outs["out"], out["out"], call, "out")
            assert torch.equal(poisoned.outs["hist_out"], out["hist_out"]), "rows at and past lens[b] reached hist_out"
        else:
            guarded_run(dw_slots(c, inp, hist, lens_of(call), dtype, d), out)
        hist = out["hist_out"]
