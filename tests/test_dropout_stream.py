"""Every dropout-carrying kernel against the HOST restatement of the dropout stream (oracle.conmamba_oracle.drop_keep, a
restatement of csrc/cm_dropout.h): masks come from the host, never from a kernel under test.

  * cm_bias_act_dropout_fwd: the stored mask equals the host mask bit for bit, and y is the fp64 value on the host mask
    (fp32 / bf16, act none / GELU, with and without the fp32 residual, rows not a multiple of 16, dim 8 .. 2048);
  * cm_bias_act_dropout_bwd with a seed and no mask, at graph-replay epochs 0, 1, 2^40 + 3: zeros exactly where the host
    dropped, survivors = alpha dy scale act'(a + b) in fp64, dbias = fp64 column sums of the stored da;
  * cm_ffn_fused (training) and cm_ffn_bwd_fused with both dropouts live: every output against an fp64 chain on host masks;
  * a 32k-row spot check of both element-wise kernels' decisions.
"""
import math

import pytest
import torch

from oracle import conmamba_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(a, b, rtol, atol):
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol * scale)


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def host_keep(seed, shape, p, epoch=0):
    keep, sc = O.drop_keep(seed, shape, p, epoch)
    return torch.from_numpy(keep), sc


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu64_grad(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


class _Epoch:
    """ops.SEED_EPOCH set to a device word holding ``epoch`` (None: no word, the host seed alone)."""

    def __init__(self, epoch):
        self.epoch = epoch

    def __enter__(self):
        from mamba_asr_amd import ops
        self.old = ops.SEED_EPOCH
        ops.SEED_EPOCH = None if self.epoch is None else torch.tensor([self.epoch], dtype=torch.int64, device=DEV)
        return self

    def __exit__(self, *exc):
        from mamba_asr_amd import ops
        torch.cuda.synchronize()
        ops.SEED_EPOCH = self.old


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_bias_act_dropout_fwd_stored_mask_is_the_host_mask(dtype):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(7 if dtype == torch.float32 else 8)
    worst = 0.0
    n = 0
    for dim in (8, 24, 256, 1000, 2048):
        for rows in (37, 64):
            for p, act, with_res in ((p, act, r) for p in (0.05, 0.1, 0.5, 0.9999) for act in (0, 1) for r in (0, 1)):
                n += 1
                seed = int(torch.randint(0, 2 ** 62, (1,), generator=g))
                a = torch.randn(rows, dim, generator=g).to(dtype)
                b = 0.1 * torch.randn(dim, generator=g)
                res = torch.randn(rows, dim, generator=g) if with_res else None
                y, m = ops.bias_act_dropout_fwd(a.to(DEV), b.to(DEV), act=act, p=p, res=None if res is None else res.to(DEV),
                                                alpha=0.5, seed=seed, store_mask=True)
                keep, sc = host_keep(seed, (rows, dim), p)
                tag = (dtype, dim, rows, p, act, with_res)
                assert m.dtype == torch.uint8 and torch.equal(m.cpu(), keep.to(torch.uint8)), tag
                t = a.double() + b.double()
                t = gelu64(t) if act else t
                d = t * keep.double() * sc
                ref = res.double() + 0.5 * d if with_res else d
                y = y.cpu().double()
                if with_res:
                    assert torch.equal(y[~keep], res.double()[~keep]), tag                # a dropped element leaves the stream alone
                else:
                    assert torch.equal(y == 0, ~keep), tag
                # fp32: erf GELU; bf16 result: the rounded x sigmoid(x P(x^2)) form (|error| < 3e-4 absolute) + one bf16 rounding
                rt, at = (1e-5, 1e-5) if dtype == torch.float32 else (8e-3, 1e-3)
                close(y, ref, rt, at)
                worst = max(worst, rel_l2(y, ref))
    print(f"bias_act_dropout_fwd {dtype}: {n} cases, worst relative L2 error {worst:.1e}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("epoch", [0, 1, 2 ** 40 + 3])
def test_bias_act_dropout_bwd_rederives_the_host_mask(dtype, epoch):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(epoch % 1000 + (dtype == torch.bfloat16))
    worst = 0.0
    for dim, rows, p, act in ((24, 301, 0.1, 1), (256, 1000, 0.1, 1), (1000, 77, 0.5, 0), (2048, 129, 0.05, 1)):
        seed = int(torch.randint(0, 2 ** 62, (1,), generator=g))
        a = torch.randn(rows, dim, generator=g).to(dtype)
        b = 0.1 * torch.randn(dim, generator=g)
        dy = torch.randn(rows, dim, generator=g)
        with _Epoch(epoch):
            da, dbias = ops.bias_act_dropout_bwd(dy.to(DEV), None, p, a=a.to(DEV), bias=b.to(DEV), act=act, alpha=0.5,
                                                 out_dtype=dtype, seed=seed)
        keep, sc = host_keep(seed, (rows, dim), p, epoch)
        tag = (dtype, epoch, dim, rows, p, act)
        da = da.cpu().double()
        assert torch.equal(da == 0, ~keep), tag
        grad = gelu64_grad(a.double() + b.double()) if act else 1.0
        ref = 0.5 * dy.double() * keep.double() * sc * grad
        rt, at = (1e-4, 1e-5) if dtype == torch.float32 else (8e-3, 5e-4)
        close(da, ref, rt, at)
        worst = max(worst, rel_l2(da, ref))
        close(dbias.cpu(), da.sum(0), 1e-5, 1e-5)                                   # what the GEMMs see: the stored da
    print(f"bias_act_dropout_bwd {dtype} epoch {epoch}: worst relative L2 error {worst:.1e}")


def _ffn_case(rows, hidden, seed):
    g = torch.Generator().manual_seed(seed)
    D = 256
    x = torch.randn(rows, D, generator=g)
    lnw, lnb = 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    w1 = (torch.randn(hidden, D, generator=g) / 16).bfloat16()
    w2 = (torch.randn(D, hidden, generator=g) / hidden ** 0.5).bfloat16()
    b1, b2 = 0.1 * torch.randn(hidden, generator=g), 0.1 * torch.randn(D, generator=g)
    dout = torch.randn(rows, D, generator=g)
    return x, lnw, lnb, w1, w2, b1, b2, dout


bf = lambda t: t.bfloat16().double()                                            # the product's roundings, applied in the chain


@pytest.mark.parametrize("rows,hidden,epoch", [(300, 1024, None), (1000, 2048, 5)])
def test_ffn_fused_training_forward_and_backward_on_host_masks(rows, hidden, epoch):
    """cm_ffn_fused (train) and cm_ffn_bwd_fused, p1 = 0.1 after the GELU and p2 = 0.2 after the second Linear, against an fp64
    chain that applies the HOST masks and rounds to bf16 where the product stores bf16."""
    from mamba_asr_amd import ops
    x, lnw, lnb, w1, w2, b1, b2, dout = _ffn_case(rows, hidden, rows + hidden)
    p1, p2, s1, s2, alpha = 0.1, 0.2, 0x5EED_0001 + rows, 0x5EED_0002 + hidden, 0.5
    ep = epoch or 0
    k1, sc1 = host_keep(s1, (rows, hidden), p1, ep)
    k2, sc2 = host_keep(s2, (rows, 256), p2, ep)
    m1, m2 = k1.double() * sc1, k2.double() * sc2
    with _Epoch(epoch):
        xo = torch.empty(rows, 256, device=DEV)
        _, (pre, xn, stats) = ops.ffn_fused(x.to(DEV), (lnw.to(DEV), lnb.to(DEV), 1e-5), w1.to(DEV), b1.to(DEV), w2.to(DEV), b2.to(DEV),
                                            alpha=alpha, x_out=xo, train=(p1, p2, s1, s2))
        da2, da1, act, dh, db1, db2 = ops.ffn_bwd_fused(dout.to(DEV), ops.PackedWeight(w2.t().contiguous().to(DEV)),
                                                        ops.PackedWeight(w1.t().contiguous().to(DEV)), pre, alpha, p1, p2, s1, s2)
    xo, pre = xo.cpu().double(), pre.cpu().double()
    # forward chain in fp64 on the host masks; GEMM 1 from the kernel's own bf16 LN output and pre-activation (pinned against
    # torch in tests/test_scan_rows_bwd.py::test_ffn_fused_training_forward), so that a mask error is not lost in a bf16 flip
    x64 = x.double()
    xn_ref = torch.nn.functional.layer_norm(x64, (256,), lnw.double(), lnb.double(), 1e-5)
    close(xn.cpu(), xn_ref, 1e-2, 1e-2)
    close(pre, xn.cpu().double() @ w1.double().t() + b1.double(), 1e-2, 1e-2)
    act_ref = bf(gelu64(pre) * m1)
    y2 = (act_ref @ w2.double().t() + b2.double()) * m2
    xo_ref = x64 + alpha * y2
    assert torch.equal(xo[~k2], x64[~k2])                                           # second dropout: the host's decisions, exactly
    assert float((xo[k2] != x64[k2]).double().mean()) > 0.99
    close(xo, xo_ref, 1e-2, 1e-2)
    errs = {"x_out": rel_l2(xo - x64, xo_ref - x64)}
    # backward chain
    da2_ref = alpha * dout.double() * m2
    da2_b = bf(da2_ref)
    dg = da2_b @ w2.double()
    da1_ref = dg * m1 * gelu64_grad(pre)
    dh_ref = bf(da1_ref) @ w1.double()
    da2, da1, act, dh = (t.cpu().double() for t in (da2, da1, act, dh))
    assert torch.equal(da2 == 0, ~k2) and torch.equal(da1 == 0, ~k1) and torch.equal(act[~k1], torch.zeros_like(act[~k1]))
    close(da2, da2_ref, 4e-3, 1e-5)
    close(act, act_ref, 1e-2, 4e-3)
    close(da1, da1_ref, 3e-2, 1e-2)
    close(dh, dh_ref, 3e-2, 1.5e-2)
    close(db2.cpu(), da2_b.sum(0), 1e-3, 1e-4)
    close(db1.cpu(), bf(da1_ref).sum(0), 2e-2, 4e-3)
    errs.update(da2=rel_l2(da2, da2_ref), act=rel_l2(act, act_ref), da1=rel_l2(da1, da1_ref), dh=rel_l2(dh, dh_ref),
                db1=rel_l2(db1, bf(da1_ref).sum(0)), db2=rel_l2(db2, da2_b.sum(0)))
    print(f"ffn fused train rows {rows} hidden {hidden} epoch {epoch}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    bad = {k: v for k, v in errs.items() if v > 1e-2}
    assert not bad, bad


def test_32k_row_spot_check():
    """The element-wise forward's stored mask and the fused backward's first-dropout zeros at 32768 rows, epoch 3."""
    from mamba_asr_amd import ops
    rows, seed, p = 32768, 0xC0FFEE_1234, 0.1
    with _Epoch(3):
        z = torch.ones(rows, 512, device=DEV, dtype=torch.bfloat16)
        _, m = ops.bias_act_dropout_fwd(z, None, act=0, p=p, seed=seed, store_mask=True)
        dout = torch.ones(rows, 256, device=DEV)
        pre = torch.ones(rows, 256, device=DEV, dtype=torch.bfloat16)
        w = ops.PackedWeight(torch.full((256, 256), 1.0 / 256, dtype=torch.bfloat16, device=DEV))
        da2, *_ = ops.ffn_bwd_fused(dout, w, w, pre, 1.0, 0.0, p, 0, seed + 1)
    keep, _ = host_keep(seed, (rows, 512), p, 3)
    assert torch.equal(m.cpu(), keep.to(torch.uint8))
    keep2, _ = host_keep(seed + 1, (rows, 256), p, 3)
    assert torch.equal((da2 != 0).cpu(), keep2)
