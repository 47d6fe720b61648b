"""The two kernels the streamed causal encoder adds (GPU): cm_conv_xproj_uni and cm_glu_dwconv_ln_gelu_causal, whole sequences
against torch fp64 on the kernel's own rounded inputs, then the same sequence in chunks through the history input, bit for bit.

Bounds: tests/test_row_kernels_fp64.py's.  fp32 results: rtol 2e-3; bf16 results: against the fp64 result rounded to bf16, rtol 2e-2;
both atol 2e-4 x max(1, max|ref|).  Each stage is held to fp64 on the operands the kernel rounded: the x_proj GEMM's operand is the u
the kernel stored (itself held to fp64), the depthwise conv's operand is the gated row rounded to the I/O dtype (what hist / hist_out
hold), the closing Linear's operand is the bf16 activation tile the same launch stores without the epilogue (itself held to fp64).
An fp64 chain that rounds the intermediate itself does not meet the absolute term at outputs near zero: a bf16 operand that lands
on the other side of a rounding boundary moves a 256-term dot product by up to 5e-4 (measured: 2.0x the allowance)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16


def check(what, got, ref64):
    bf = got.dtype == BF16
    want = (ref64.to(BF16) if bf else ref64).double().cpu()
    rtol, atol = (2e-2 if bf else 2e-3), 2e-4 * max(1.0, float(want.abs().max()))
    err = (got.detach().double().cpu() - want).abs()
    ratio = float((err / (atol + rtol * want.abs())).max())
    print(f"{what}: max|err| {float(err.max()):.3e}, max err / allowance {ratio:.3f}")
    assert got.shape == want.shape and ratio <= 1.0, (what, float(err.max()), ratio)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---------------------------------------------------------------------------------------------------- cm_conv_xproj_uni
@pytest.mark.parametrize("dim,rw", [(64, 48), (512, 48), (512, 64)], ids=["d64", "d512", "d512_dt32"])
def test_conv_xproj_uni_whole_and_chunked(dim, rw):
    from mamba_asr_amd import ops
    b, T = 2, 37
    g = gen(100 + dim + rw)
    xz = torch.randn(b, T, 2 * dim, generator=g).to(BF16).to(DEV)              # x is the first half of wider rows, as in the encoder
    x = xz[:, :, :dim]
    w, bias = (torch.randn(dim, 4, generator=g) * 0.5).to(DEV), (torch.randn(dim, generator=g) * 0.1).to(DEV)
    wx = (torch.randn(rw, dim, generator=g) / dim ** 0.5).to(BF16).to(DEV)
    wxp = ops.PackedWeight(wx)

    def run(xs, hist=None, hist_out=None, variant=0):
        u = torch.empty(xs.shape, dtype=BF16, device=DEV)
        xdbl = ops.conv_xproj_uni(xs, w, bias, wxp, out=u, x_hist=hist, x_hist_out=hist_out, variant=variant)
        return u, xdbl

    u, xdbl = run(x)
    # fp64: 3 zero rows in front, taps k = 0..3 on x[t-3+k]; SiLU; the GEMM on the u the kernel stored
    xp = F.pad(x.double().cpu(), (0, 0, 3, 0))
    conv = bias.double().cpu() + sum(w.double().cpu()[:, k] * xp[:, k:k + T] for k in range(4))
    check(f"conv_xproj_uni u dim {dim}", u, conv * torch.sigmoid(conv))
    check(f"conv_xproj_uni xdbl dim {dim} rw {rw}", xdbl, u.double().cpu() @ wx.double().cpu().t())
    u1, xdbl1 = run(x, variant=1)                                              # the 16-step tiles pinned
    assert torch.equal(u1, u)
    check("xdbl, pinned tile variant vs default", xdbl1, xdbl.double())
    # NULL history == zero history
    zeros = torch.zeros(b, 3, dim, dtype=BF16, device=DEV)
    uz, xz_ = run(x, hist=zeros)
    assert torch.equal(uz, u) and torch.equal(xz_, xdbl)
    # the same sequence in chunks
    hist, spare = torch.zeros_like(zeros), torch.full_like(zeros, float("nan"))
    us, xs, t0 = [], [], 0
    seen = torch.cat([zeros, x], dim=1)
    for n in (1, 2, 3, 5, 26):
        uc, xc = run(x[:, t0:t0 + n], hist=hist, hist_out=spare, variant=1)
        t0 += n
        assert torch.equal(spare, seen[:, t0:t0 + 3]), f"x_hist_out after {t0} steps"
        hist, spare = spare, hist
        us.append(uc), xs.append(xc)
    assert t0 == T
    assert torch.equal(torch.cat(us, 1), u), "u of the chunks != u of the whole"
    assert torch.equal(torch.cat(xs, 1), xdbl1), "xdbl of the chunks != xdbl of the whole (16-step tiles pinned)"
    # default tile choice: within the bf16 bound of the whole (the same kernel at these sizes)
    uc, xc = run(x[:, 11:], hist=x[:, 8:11].contiguous(), hist_out=spare)
    assert torch.equal(uc, u[:, 11:])
    check("xdbl, chunk at the default variant vs whole", xc, xdbl[:, 11:].double())
    # aliasing is refused before launch, and leaves the buffer alone
    keep = hist.clone()
    with pytest.raises(RuntimeError, match="x_hist"):
        run(x[:, :4], hist=hist, hist_out=hist)
    torch.cuda.synchronize()
    assert torch.equal(hist, keep)


# ------------------------------------------------------------------------------------------ cm_glu_dwconv_ln_gelu_causal
def _ln64(t, g, b, eps):
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + eps) * g + b


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / 2 ** 0.5))


CASES = [(BF16, 256, True, False), (BF16, 256, True, True), (BF16, 256, False, False), (BF16, 256, False, True),
         (BF16, 512, True, False), (torch.float32, 64, False, False), (torch.float32, 64, True, False), (BF16, 144, True, False)]


@pytest.mark.parametrize("dtype,D,glu_done,lin", CASES,
                         ids=[f"{'bf16' if d == BF16 else 'fp32'}_d{D}_{'gated' if gd else 'glu'}{'_lin' if l else ''}" for d, D, gd, l in CASES])
def test_glu_dwconv_causal_whole_and_chunked(dtype, D, glu_done, lin):
    from mamba_asr_amd import ops
    b, T, K = 2, 70, 31
    g = gen(7000 + D + 2 * glu_done + lin)
    inp = torch.randn(b, T, D if glu_done else 2 * D, generator=g).to(dtype).to(DEV)
    w, bs = (torch.randn(D, K, generator=g) / 6).to(DEV), (torch.randn(D, generator=g) * 0.1).to(DEV)
    lg, lb = (1.0 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    kw = dict(weight_t=w.t().contiguous(), glu_done=glu_done, causal=True)
    if lin:
        lw, lbias = (torch.randn(D, D, generator=g) / 16).to(BF16).to(DEV), (torch.randn(D, generator=g) * 0.1).to(DEV)
        kw.update(lin_w=ops.PackedWeight(lw), lin_b=lbias)
    run = lambda t, **k: ops.glu_dwconv_ln_gelu(t, w, bs, lg, lb, 1e-5, **kw, **k)
    zeros = torch.zeros(b, K - 1, D, dtype=dtype, device=DEV)
    last = torch.full_like(zeros, float("nan"))
    out = run(inp, hist_out=last)
    # fp64: row 0 sees 30 zero rows and nothing from the future
    i64 = inp.double().cpu()
    gated = i64 if glu_done else (i64[..., :D] * torch.sigmoid(i64[..., D:])).to(dtype).double()
    gp = F.pad(gated, (0, 0, K - 1, 0))
    conv = bs.double().cpu() + sum(w.double().cpu()[:, k] * gp[:, k:k + T] for k in range(K))
    act = _gelu64(_ln64(conv, lg.double().cpu(), lb.double().cpu(), 1e-5))
    what = f"glu_dwconv_causal {dtype} dim {D} glu_done {glu_done} lin {lin}"
    if lin:
        # the Linear's operand is the bf16 activation tile: the same launch without the epilogue stores it (held to fp64 here, and
        # in its own case above), so the GEMM stage is checked on the operand the kernel rounded
        act_k = ops.glu_dwconv_ln_gelu(inp, w, bs, lg, lb, 1e-5, weight_t=kw["weight_t"], glu_done=glu_done, causal=True)
        check(what + ": activations", act_k, act)
        check(what, out, act_k.double().cpu() @ lw.double().cpu().t() + lbias.double().cpu())
    else:
        check(what, out, act)
    check("hist_out of the whole sequence", last, gated[:, T - (K - 1):])
    if glu_done:
        assert torch.equal(last, inp[:, T - (K - 1):])
    assert torch.equal(run(inp), out) and torch.equal(run(inp, hist=zeros), out)       # no hist_out wanted; NULL == zero history
    # causality: the future does not reach the past
    changed = inp.clone()
    changed[:, 40:] = torch.randn(b, T - 40, inp.shape[-1], generator=g).to(dtype).to(DEV)
    assert torch.equal(run(changed)[:, :40], out[:, :40])
    # chunks across the 32-step tile edge and the 30-row history edge, both ways
    hist, spare = zeros.clone(), torch.full_like(zeros, float("nan"))
    outs, t0 = [], 0
    for n in (1, 7, 30, 31, 1):
        outs.append(run(inp[:, t0:t0 + n], hist=hist, hist_out=spare))
        t0 += n
        # the history after t0 steps is what a whole run over the first t0 steps leaves
        ref_hist = torch.empty_like(zeros)
        run(inp[:, :t0], hist_out=ref_hist)
        assert torch.equal(spare, ref_hist), f"hist_out after {t0} steps"
        if glu_done:
            assert torch.equal(spare, torch.cat([zeros, inp[:, :t0]], dim=1)[:, t0:])
        hist, spare = spare, hist
    assert t0 == T
    assert torch.equal(torch.cat(outs, 1), out), "the chunks' outputs != the whole's"
    keep = hist.clone()
    with pytest.raises(RuntimeError, match="hist"):
        run(inp[:, :5], hist=hist, hist_out=hist)
    torch.cuda.synchronize()
    assert torch.equal(hist, keep)
