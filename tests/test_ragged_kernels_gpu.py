"""The kernels of the whole-utterance route with per-utterance lengths (GPU): cm_conv_xproj_lens, cm_scan_cl_fwd_lens,
cm_glu_dwconv_ln_gelu_lens, cm_cnn_front_lens, cm_fbank_wav_lens + cm_fbank_finish_lens.

One launch per kernel: bf16, B = 12, T_max = 70, lens = 0, 1, 2, 3 (the width-4 conv), 15, 16, 17 (the 16-step tiles and scan blocks,
the 15-row halo of the k = 31 conv), 31, 32, 33 (the 32-step tiles), 69, 70 (a ragged last tile, the whole batch row), E = 512, D = 256.
Every input row at and past lens[b] is NaN, the inputs sit inside NaN and the outputs inside sentinels (tests/guard_bands.py), so the
launch is checked for writing only inside its buffers.  For every b with lens[b] > 0 the valid rows are torch.equal to the entry
point without lengths (cm_conv_xproj, cm_scan_cl_fwd with time_chunks = 1, cm_glu_dwconv_ln_gelu, cm_cnn_front, cm_fbank_wav +
cm_fbank_finish) launched on that utterance ALONE with seqlen = lens[b].  The scan's rows at and past lens[b] keep their sentinel.

The front end: sample counts from 640 in steps of 253 (no multiple of the hop), so that the frame counts T_b = 5 .. 19 are odd and
even, so are T1_b = ceil(T_b / 2), and T_max = 19 is no multiple of 4; an utterance of 0 samples; and one whose loudest frame is frame
T_b -- a click in its last 40 samples, 10 samples in front of that frame's centre -- which fails when the top_db maximum runs over
every frame of the padded batch (asserted: the launch without lengths, padding zeroed, gives other features for it)."""
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
B, T, D, E, K = 12, 70, 256, 512, 31
LENS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 69, 70]
assert len(LENS) == B and max(LENS) == T


def dev(t):
    return t.to(DEV)


def lens_of(call):
    return torch.tensor(call, dtype=torch.int32, device=DEV)


def nan_behind(t, call):
    """t (B, T, ...) with everything at and past call[b] NaN."""
    t = t.clone()
    for b, n in enumerate(call):
        t[b, n:] = NAN
    return t


def untouched(L):
    torch.cuda.synchronize()
    for name, (buf, _, outside) in L.g.items.items():
        G.assert_untouched(buf, outside, name)


# ---------------------------------------------------------------------------------------------------------- cm_conv_xproj_lens
def test_conv_xproj_lens():
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(5101)
    xz = dev(torch.randn(B, T, 2 * E, generator=g).to(BF16))                     # x is the first half of [x | z] rows, as in the encoder
    wf, bf = dev(torch.randn(E, 4, generator=g) * 0.5), dev(torch.randn(E, generator=g) * 0.1)
    wb, bb = dev(torch.randn(E, 4, generator=g) * 0.5), dev(torch.randn(E, generator=g) * 0.1)
    wxf = ops.PackedWeight(dev((torch.randn(48, E, generator=g) / E ** 0.5).to(BF16)))
    wxb = ops.PackedWeight(dev((torch.randn(48, E, generator=g) / E ** 0.5).to(BF16)))
    L = G.Launch(True, DEV)
    x = L.cols(nan_behind(xz, LENS), dead=(E, 2 * E))[:, :, :E]
    uf, ub = L.out("u_fwd", (B, T, E), BF16, **COLS), L.out("u_bwd", (B, T, E), BF16, **COLS)
    xd = L.out("xdbl", (B, T, 96), BF16, **COLS)
    ops.conv_xproj(x, L.vec(wf), L.vec(bf), L.vec(wb), L.vec(bb), wxf, wxb, out_f=uf, out_b=ub, xdbl=xd, lens=lens_of(LENS))
    untouched(L)
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        f1, b1 = torch.empty(1, n, E, dtype=BF16, device=DEV), torch.empty(1, n, E, dtype=BF16, device=DEV)
        x1 = ops.conv_xproj(xz[b:b + 1, :n, :E], wf, bf, wb, bb, wxf, wxb, out_f=f1, out_b=b1)
        assert bool(torch.isfinite(x1.float()).all())
        assert torch.equal(uf[b, :n], f1[0]), f"u_fwd, utterance {b}, lens {n}"
        assert torch.equal(ub[b, :n], b1[0]), f"u_bwd, utterance {b}, lens {n}"
        assert torch.equal(xd[b, :n], x1[0]), f"xdbl, utterance {b}, lens {n}"
    # lengths are clamped on the device: above T is T, below 0 is 0
    o = [torch.zeros(B, T, E, dtype=BF16, device=DEV) for _ in range(2)]
    xc = ops.conv_xproj(xz[:, :, :E], wf, bf, wb, bb, wxf, wxb, out_f=o[0], out_b=o[1], xdbl=torch.zeros(B, T, 96, dtype=BF16, device=DEV),
                        lens=lens_of([T + 9, -4] + LENS[2:]))
    f1, b1 = torch.empty(1, T, E, dtype=BF16, device=DEV), torch.empty(1, T, E, dtype=BF16, device=DEV)
    x1 = ops.conv_xproj(xz[:1, :, :E], wf, bf, wb, bb, wxf, wxb, out_f=f1, out_b=b1)
    assert torch.equal(o[0][0], f1[0]) and torch.equal(o[1][0], b1[0]) and torch.equal(xc[0], x1[0])
    assert not bool(o[0][1].any()) and not bool(o[1][1].any()) and not bool(xc[1].any())


# --------------------------------------------------------------------------------------------------------- cm_scan_cl_fwd_lens
@pytest.mark.parametrize("ndir", [2, 1])
def test_scan_cl_fwd_lens(ndir):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(5102)
    rank = 9
    xz = dev(torch.randn(B, T, 2 * E, generator=g).to(BF16))                     # z is the second half
    u = dev(torch.randn(B, T, 2 * E, generator=g).to(BF16))                      # [u_fwd | u_bwd]
    xdt = torch.randn(B, T, 96, generator=g)
    xdt[:, :, rank:16] = 0.0
    xdt[:, :, 48 + rank:64] = 0.0
    xd = dev(xdt.to(BF16))
    par = [dict(A=dev(-torch.exp(torch.randn(E, 16, generator=g) * 0.3)), W=ops.pad_dt_weight(dev(torch.randn(E, rank, generator=g) * 0.3)),
                D=dev(torch.randn(E, generator=g)), bias=dev(torch.randn(E, generator=g) - 1)) for _ in range(2)]

    def dirs(u_, xd_, y_, vec=lambda t: t):
        # one direction: the REVERSE one, the one whose start depends on the length
        sel = range(2) if ndir == 2 else [1]
        return [dict(u=u_[:, :, i * E:(i + 1) * E], xdbl=xd_[:, :, 48 * i:48 * (i + 1)], A=vec(par[i]["A"]), D=vec(par[i]["D"]),
                     delta_bias=vec(par[i]["bias"]), dt_weight=vec(par[i]["W"]), out=y_[:, :, i * E:(i + 1) * E], reverse=bool(i)) for i in sel]

    L = G.Launch(True, DEV)
    y = L.out("y", (B, T, 2 * E), BF16, **COLS)
    ops.scan_cl_fwd(dirs(L.cols(nan_behind(u, LENS)), L.cols(nan_behind(xd, LENS)), y, L.vec), z=L.cols(nan_behind(xz, LENS), dead=(0, E))[:, :, E:],
                    delta_softplus=True, lens=lens_of(LENS), whole=True)
    untouched(L)
    cols = slice(0, 2 * E) if ndir == 2 else slice(E, 2 * E)
    for b, n in enumerate(LENS):
        assert bool((y[b, n:, cols] == G.SENTINEL).all()), f"utterance {b}: an output row at or past lens {n} was written"
        if n == 0:
            continue
        y1 = torch.empty(1, n, 2 * E, dtype=BF16, device=DEV)
        ops.scan_cl_fwd(dirs(u[b:b + 1, :n], xd[b:b + 1, :n], y1), z=xz[b:b + 1, :n, E:], delta_softplus=True, time_chunks=1)
        assert bool(torch.isfinite(y1[:, :, cols].float()).all())
        assert torch.equal(y[b, :n, cols], y1[0, :, cols]), f"y, utterance {b}, lens {n}"
    if ndir == 1:
        assert bool((y[:, :, :E] == G.SENTINEL).all())


def test_scan_cl_fwd_lens_refuses():
    """Chunked launches and carried state are outside the contract: refused before anything is launched."""
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(5)
    u, xd = dev(torch.randn(2, 40, 64, generator=g).to(BF16)), dev(torch.randn(2, 40, 48, generator=g).to(BF16))
    dd = dict(u=u, xdbl=xd, A=dev(-torch.rand(64, 16, generator=g)), D=None, delta_bias=None, dt_weight=ops.pad_dt_weight(dev(torch.randn(64, 4, generator=g))),
              out=torch.zeros_like(u), reverse=True)
    lens = lens_of([3, 40])
    with pytest.raises(RuntimeError, match="unchunked"):
        ops.scan_cl_fwd([dd], z=u, lens=lens, whole=True, time_chunks=2)
    with pytest.raises(RuntimeError, match="carried state"):
        ops.scan_cl_fwd([dict(dd, h0=torch.zeros(2, 64, 16, device=DEV))], z=u, lens=lens, whole=True)
    torch.cuda.synchronize()
    assert not bool(dd["out"].any())


# -------------------------------------------------------------------------------------------------- cm_glu_dwconv_ln_gelu_lens
DW = [(BF16, 256, True), (BF16, 256, False), (BF16, 512, False), (BF16, 64, False), (F32, 64, False)]


@pytest.mark.parametrize("dtype,d,lin", DW, ids=["bf16_d256_lin", "bf16_d256", "bf16_d512", "bf16_d64_generic", "fp32_d64_generic"])
def test_glu_dwconv_lens(dtype, d, lin):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(5103 + d + lin)
    inp = dev(torch.randn(B, T, d, generator=g).to(dtype))                       # gated rows (glu_done), as cm_ln_pw_glu leaves them
    w, bs = dev(torch.randn(d, K, generator=g) / 6), dev(torch.randn(d, generator=g) * 0.1)
    lg, lb = dev(1.0 + 0.1 * torch.randn(d, generator=g)), dev(0.1 * torch.randn(d, generator=g))
    wt = w.t().contiguous()
    kw = {}
    if lin:
        kw = dict(lin_w=ops.PackedWeight(dev((torch.randn(d, d, generator=g) / 16).to(BF16))), lin_b=dev(torch.randn(d, generator=g) * 0.1))

    def launch(x, vec=lambda t: t, **more):
        k2 = dict(kw, lin_b=vec(kw["lin_b"])) if lin else {}
        return ops.glu_dwconv_ln_gelu(x, vec(w), vec(bs), vec(lg), vec(lb), 1e-5, weight_t=vec(wt), glu_done=True, **k2, **more)

    L = G.Launch(True, DEV)
    out = L.out("out", (B, T, d), dtype, rows=TT, contiguous=True)
    launch(L.flat(nan_behind(inp, LENS), TT), L.vec, out=out, lens=lens_of(LENS))
    untouched(L)
    for b, n in enumerate(LENS):
        if n == 0:
            continue
        o1 = launch(inp[b:b + 1, :n])
        assert bool(torch.isfinite(o1.float()).all())
        assert torch.equal(out[b, :n], o1[0]), f"out, utterance {b}, lens {n}"
    # the GLU form (2 d wide input) of both kernels
    inp2 = dev(torch.randn(B, T, 2 * d, generator=g).to(dtype))
    o2 = ops.glu_dwconv_ln_gelu(nan_behind(inp2, LENS), w, bs, lg, lb, 1e-5, weight_t=wt, lens=lens_of(LENS), **kw)
    for b, n in enumerate(LENS):
        if n:
            assert torch.equal(o2[b, :n], ops.glu_dwconv_ln_gelu(inp2[b:b + 1, :n], w, bs, lg, lb, 1e-5, weight_t=wt, **kw)[0]), f"GLU form, utterance {b}, lens {n}"


# ----------------------------------------------------------------------------------------------------------- the front end
HOP, NFFT, NMEL = 160, 512, 80
NS = [640 + 253 * i for i in range(10)] + [0, 160 * 9 + 150]                      # 640 .. 2917; nothing; the click
S_MAX = max(NS) + 1                                                                # even: the kernel's 8-byte sample loads take the view as it is
FRAMES = [1 + n // HOP if n else 0 for n in NS]
T_MAX = 1 + S_MAX // HOP
CLICK = len(NS) - 1
assert T_MAX % 4 and {t % 2 for t in FRAMES[:10]} == {0, 1} and {((t + 1) // 2) % 2 for t in FRAMES[:10]} == {0, 1} and min(FRAMES[:10]) == 5
assert all(n % HOP for n in NS[1:] if n) and 253 % HOP and FRAMES[CLICK] < T_MAX


@functools.lru_cache(maxsize=None)
def wav_case():
    from mamba_asr_amd import sb_compat as sb
    g = torch.Generator().manual_seed(5104)
    wav = 0.1 * torch.randn(len(NS), S_MAX, generator=g)
    n = NS[CLICK]
    wav[CLICK, n - 40:n] = 300.0 * torch.randn(40, generator=g)                   # 10 .. 50 samples in front of the centre of frame T_b
    fb = sb.Fbank(n_fft=NFFT, n_mels=NMEL).to(DEV)
    mean, std = dev(torch.randn(NMEL, generator=g)), dev(1.0 + torch.rand(NMEL, generator=g))
    return dev(wav), fb, mean, std


def fbank(wav, fb, mean, std, **kw):
    from mamba_asr_amd import ops
    return ops.fbank_from_wav(wav, fb.window, fb.n_fft, fb.hop, fb.fbank, fb.amin, fb.top_db, mean, std, **kw)


def test_fbank_lens():
    wav, fb, mean, std = wav_case()
    nb = len(NS)
    assert fb.hop == HOP
    L = G.Launch(True, DEV)
    bufs = dict(db=L.out("db", (nb, T_MAX, NMEL), F32, rows=16, contiguous=True), umax=L.out("umax", (nb,), F32, rows=64, contiguous=True),
                umax_part=L.out("umax_part", (nb, (T_MAX + 15) // 16), F32, rows=64, contiguous=True))
    db = fbank(L.flat(nan_behind(wav, NS), 512), fb, mean, std, lens=lens_of(NS), bufs=bufs)
    untouched(L)
    zeroed = nan_behind(wav, NS).nan_to_num(0.0)
    padded = fbank(zeroed, fb, mean, std)                                          # no lengths, silence behind every utterance
    for b, n in enumerate(NS):
        if n == 0:
            assert bool((db[b] == G.SENTINEL).all()), "an utterance of 0 samples has no frame"
            continue
        t = FRAMES[b]
        solo = fbank(wav[b:b + 1, :n].contiguous(), fb, mean, std)
        assert solo.shape[1] == t and bool(torch.isfinite(solo).all())
        assert torch.equal(db[b, :t], solo[0]), f"features, utterance {b}, {n} samples, {t} frames"
    t = FRAMES[CLICK]
    assert not torch.equal(padded[CLICK, :t], db[CLICK, :t]), "the click must make frame T_b the loudest: the case does not discriminate"
    quiet = [b for b in range(10) if torch.equal(padded[b, :FRAMES[b]], db[b, :FRAMES[b]])]
    print("utterances whose features the zero padding alone does not change:", quiet)


def test_cnn_front_lens():
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(5105)
    nb = len(NS)
    feats = dev(torch.randn(nb, T_MAX, 80, generator=g))
    w1, b1 = dev(torch.randn(64, 1, 3, 3, generator=g) / 3), dev(torch.randn(64, generator=g) * 0.1)
    g1, bt1 = dev(1.0 + 0.1 * torch.randn(40 * 64, generator=g)), dev(0.1 * torch.randn(40 * 64, generator=g))
    w2 = dev((torch.randn(32, 3, 3, 64, generator=g) / 24).to(BF16))
    b2 = dev(torch.randn(32, generator=g) * 0.1)
    g2, bt2 = dev(1.0 + 0.1 * torch.randn(20 * 32, generator=g)), dev(0.1 * torch.randn(20 * 32, generator=g))
    t2 = ((T_MAX + 1) // 2 + 1) // 2
    L = G.Launch(True, DEV)
    out = L.out("rows", (nb, t2, 640), BF16, rows=8, contiguous=True)
    ops.cnn_front(L.flat(nan_behind(feats, FRAMES), 16), w1, L.vec(b1), L.vec(g1), L.vec(bt1), 1e-5, w2, L.vec(b2), L.vec(g2), L.vec(bt2), 1e-5, 0.01,
                  lens=lens_of(FRAMES), out=out)
    untouched(L)
    for b, t in enumerate(FRAMES):
        r = ((t + 1) // 2 + 1) // 2
        assert bool((out[b, r:] == G.SENTINEL).all()), f"utterance {b}: a row at or past {r} was written"
        if t == 0:
            continue
        solo = ops.cnn_front(feats[b:b + 1, :t], w1, b1, g1, bt1, 1e-5, w2, b2, g2, bt2, 1e-5, 0.01)
        assert solo.shape[1] == r and bool(torch.isfinite(solo.float()).all())
        assert torch.equal(out[b, :r], solo[0]), f"rows, utterance {b}, {t} frames, {r} rows"
