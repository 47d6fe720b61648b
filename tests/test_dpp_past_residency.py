"""The kernels whose reductions go through cm_common.h's DPP helpers (cm_group_sum, cm_group_bcast, cm_dpp), at grids of at least
twice the workgroups an MI355X holds at once (256 CUs x the blocks per CU of the launch bounds), against float64 restatements,
row by row, and run twice for equal bits.

Why: cm_ffn_fused once read a packed-FP32 result by DPP too early; lanes 48-63 then saw a register left by an earlier workgroup.
That needs a launch with more workgroups than are resident, and it touches one lane group in eight, so a relative-L2 bound over
a small grid cannot see it.  tests/test_isa_dpp_hazard.py checks the ISA for the pattern; these tests check the results.  Every
bound holds per element, and a failure names the rows (with their index mod 8 and mod 16) that broke it."""
import pytest
import torch

from oracle import conmamba_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rows_within(got, ref, rtol, atol, what):
    """Every element of every row within atol + rtol |ref| of the float64 reference; the last dimension is the row."""
    g = got.detach().to(DEV, torch.float64).reshape(-1, got.shape[-1])
    r = ref.detach().to(DEV, torch.float64).reshape(-1, ref.shape[-1])
    assert g.shape == r.shape, (g.shape, r.shape)
    err = (g - r).abs()
    excess = (err - (atol + rtol * r.abs())).amax(dim=1)
    bad = (excess > 0).nonzero().flatten().cpu()
    worst = float(err.amax())
    print(f"{what}: {g.shape[0]} rows, max|err| {worst:.3e}, max row excess over the bound {float(excess.max()):.3e}")
    if bad.numel():
        mod8 = torch.bincount(bad % 8, minlength=8).tolist()
        mod16 = torch.bincount(bad % 16, minlength=16).tolist()
        i = int(excess.argmax())
        raise AssertionError(f"{what}: {bad.numel()} of {g.shape[0]} rows out of bounds (rows mod 8: {mod8}; mod 16: {mod16}); "
                             f"first {bad[:8].tolist()}; worst row {i}: max|err| {float(err[i].max()):.3e}")


def same_bits(a, b, what):
    if torch.equal(a, b):
        return
    diff = (a != b).reshape(-1, a.shape[-1]).any(dim=1).nonzero().flatten().cpu()
    raise AssertionError(f"{what}: {diff.numel()} rows differ between two identical launches (rows mod 8: "
                         f"{torch.bincount(diff % 8, minlength=8).tolist()}); first {diff[:8].tolist()}")


def _ln64(t, p):
    t = t.double()
    mu = t.mean(-1, keepdim=True)
    var = ((t - mu) ** 2).mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(var + p[2]) * p[0].double() + p[1].double()


def _gelu64(t):
    return 0.5 * t * (1.0 + torch.erf(t / 2 ** 0.5))


# ------------------------------------------------------------------------------------------------ cm_glu_dwconv_ln_gelu

@pytest.mark.parametrize("D,lin", [(256, False), (256, True), (512, False)], ids=["d256", "d256_lin", "d512"])
def test_dwconv_rows_past_residency(D, lin):
    """dwconv_rows_kernel at the benchmark's 64 x 1000 rows: 32-step tiles, so 64 x 32 = 2048 workgroups, 2x the 256 x 4 resident
    at dim 256 (launch bounds (256, 4)) and 4x the 256 x 2 at dim 512.  GLU'd bf16 input -> depthwise conv 31 -> LayerNorm -> GELU
    (-> the Linear epilogue with LIN, the default bf16 forward's path) vs float64."""
    from mamba_asr_amd import ops
    b, L = 64, 1000
    g = torch.Generator(device="cpu").manual_seed(6400 + D + lin)
    gated = torch.randn(b, L, D, generator=g).bfloat16().to(DEV)
    w, bs = (torch.randn(D, 31, generator=g) / 6).to(DEV), (torch.randn(D, generator=g) * 0.1).to(DEV)
    lg, lb = (1.0 + 0.1 * torch.randn(D, generator=g)).to(DEV), (0.1 * torch.randn(D, generator=g)).to(DEV)
    wt = w.t().contiguous()
    kw = {}
    if lin:
        lw, lbias = (torch.randn(D, D, generator=g) / 16).bfloat16().to(DEV), (torch.randn(D, generator=g) * 0.1).to(DEV)
        kw = dict(lin_w=ops.PackedWeight(lw), lin_b=lbias)
    run = lambda: ops.glu_dwconv_ln_gelu(gated, w, bs, lg, lb, 1e-5, weight_t=wt, glu_done=True, **kw)
    out = run()
    out2 = run()
    torch.cuda.synchronize()
    # float64: 'same' depthwise convolution as 31 shifted products
    xp = torch.nn.functional.pad(gated.double().transpose(1, 2), (15, 15))
    conv = bs.double()[None, :, None] + sum(w.double()[None, :, k, None] * xp[:, :, k:k + L] for k in range(31))
    act = _gelu64(_ln64(conv.transpose(1, 2), (lg, lb, 1e-5)))
    del xp, conv
    same_bits(out, out2, f"dwconv dim {D}{' LIN' if lin else ''}")
    if lin:
        want = act @ lw.double().t() + lbias.double()
        rows_within(out, want, 1.6e-2, 1e-2, f"dwconv + Linear dim {D}")
    else:
        rows_within(out, act, 1.6e-2, 1e-2, f"dwconv dim {D}")


# ------------------------------------------------------------------------------------------------------------ cm_ffn_fused

@pytest.mark.parametrize("addend,proj", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "addend", "proj", "addend_proj"])
@pytest.mark.parametrize("layout", [32, -32])                # -32: layout 32 with 32-token workgroups
def test_ffn_fused32_past_residency(layout, addend, proj):
    """ffn_fused32_kernel (launch bounds (256, 2): 512 resident) at 66000 rows: 1032 workgroups of 64 tokens, or 2063 of 32, with
    the ragged last tile.  LayerNorm -> W1 -> GELU -> W2 -> scaled residual (+ addend) -> norm1 -> norm2 (-> in_proj) vs float64
    with the kernel's bf16 rounding points (GEMM operands), every output row."""
    from mamba_asr_amd import ops
    rows, hidden, D = 66000, 1024, 256
    g = torch.Generator(device="cpu").manual_seed(660 + 10 * layout + 2 * addend + proj)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(DEV)
    x = rn(rows, D, scale=2.0) + 0.5
    add = rn(rows, D).bfloat16() if addend else None
    w1, b1 = rn(hidden, D, scale=D ** -0.5).bfloat16(), rn(hidden, scale=0.1)
    w2, b2 = rn(D, hidden, scale=hidden ** -0.5).bfloat16(), rn(D, scale=0.1)
    ln = lambda: (1.0 + 0.1 * rn(D), 0.1 * rn(D), 1e-5)
    pre, n1, n2 = ln(), (ln() if addend else None), ln()
    wp, bp = (rn(1024, D, scale=1 / 16).bfloat16(), rn(1024, scale=0.1)) if proj else (None, None)
    tokens = {32: 64, -32: 32}[layout]
    w1p, w2p = ops.PackedWeight(w1, 32), ops.PackedWeight(w2, 32)
    wpp = ops.PackedWeight(wp, 32) if proj else None

    def run():
        xo = x.clone()
        _, second = ops.ffn_fused(xo, pre, w1p, b1, w2p, b2, alpha=0.5, addend=add, add_scale=0.7, norm1=n1, norm2=n2,
                                  want_h=not proj, h_dtype=torch.bfloat16, tokens=tokens, proj_w=wpp, proj_b=bp)
        return xo, second

    xo, second = run()
    xo2, second2 = run()
    torch.cuda.synchronize()
    name = f"ffn32 tokens {tokens}{' addend' if addend else ''}{' proj' if proj else ''}"
    same_bits(xo, xo2, name + " stream")
    same_bits(second, second2, name + (" in_proj" if proj else " h"))
    # float64 with the kernel's rounding points
    xin = x.double() + (0.7 * add.double() if addend else 0.0)
    hn = _ln64(xin, pre).bfloat16().double()
    hid = _gelu64(hn @ w1.double().t() + b1.double()).bfloat16().double()
    r = xin + 0.5 * (hid @ w2.double().t() + b2.double())
    del hn, hid
    if addend:
        r = _ln64(r, n1)
    h = _ln64(r, n2)
    rows_within(xo, r, 2e-3, 4e-3, name + " stream")
    if proj:
        rows_within(second, h.bfloat16().double() @ wp.double().t() + bp.double(), 8e-3, 8e-3, name + " in_proj")
    else:
        rows_within(second, h, 1e-2, 2e-2, name + " h")


# --------------------------------------------------------------------------------------------------- cm_selective_scan_bwd

@pytest.mark.parametrize("reverse", [False, True])
def test_selective_scan_bwd_past_residency(reverse):
    """scan_bwd_kernel, dstate 16 (64 channels per workgroup, launch bounds (256, 1): 256 resident) at batch 64 x dim 512:
    8 x 64 = 512 workgroups, two 64-step checkpoint chunks, vs the oracle's analytic gradients in float64; du, ddelta, dz per
    (batch, channel) row, dB, dC per (batch, state) row, the batch-summed dA, dD, ddelta_bias per channel."""
    from mamba_asr_amd import ops
    b, e, l, n = 64, 512, 128, 16
    gen = torch.Generator().manual_seed(6451 + reverse)
    u = torch.randn(b, e, l, generator=gen)
    dl = torch.randn(b, e, l, generator=gen) * 0.5
    A = -torch.exp(torch.randn(e, n, generator=gen) * 0.3)
    B, C = torch.randn(b, n, l, generator=gen), torch.randn(b, n, l, generator=gen)
    D, z, bias = torch.randn(e, generator=gen), torch.randn(b, e, l, generator=gen), torch.randn(e, generator=gen) - 1
    dout = torch.randn(b, e, l, generator=gen)
    f = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    gu, gdl, gA, gB, gC, gD, gz, gbias, gdout = (t.to(DEV) for t in (u, dl, A, B, C, D, z, bias, dout))
    _, x, _ = ops.selective_scan_fwd(gu, gdl, gA, gB, gC, gD, gz, gbias, True, reverse=reverse, need_out=False)
    run = lambda: ops.selective_scan_bwd(gu, gdl, gA, gB, gC, gD, gz, gbias, gdout, x, True, reverse=reverse)[:8]
    got = run()
    again = run()
    torch.cuda.synchronize()
    names = ("du", "ddelta", "dA", "dB", "dC", "dD", "ddelta_bias", "dz")
    for k, t1, t2 in zip(names, got, again):
        same_bits(t1, t2, f"scan bwd {k}")
    r = O.selective_scan_bwd(f(u), f(dl), A, f(B), f(C), D, f(z), bias, f(dout), True)
    du, dd, dA, dB, dC, dD, dbias, dz = got
    for k, gt, ref in (("du", du, f(r["du"])), ("ddelta", dd, f(r["ddelta"])), ("dz", dz, f(r["dz"])),
                       ("dB", dB[:, 0], f(r["dB"])), ("dC", dC[:, 0], f(r["dC"])), ("dA", dA.reshape(1, -1), r["dA"].reshape(1, -1)),
                       ("dD", dD.reshape(1, -1), r["dD"].reshape(1, -1)),
                       ("ddelta_bias", dbias.reshape(1, -1), r["ddelta_bias"].reshape(1, -1))):
        rows_within(gt, ref, 2e-3, 2e-4 * max(ref.abs().max().item(), 1.0), f"scan bwd{' reverse' if reverse else ''} {k}")
