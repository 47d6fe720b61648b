"""cm_ctc_loss (csrc/ctc.hip) vs torch.nn.functional.ctc_loss in fp64 on the CPU (what speechbrain's ctc_loss wraps, reference
train_CTC.py:405): per-utterance negative log-likelihoods and the gradient w.r.t. the log-probabilities, ragged input / target
lengths, repeated labels, an utterance with no valid alignment (zero_infinity), empty targets; bit-reproducible."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _ref(lp, tg, il, tl, blank=0):
    lp64 = lp.double().requires_grad_(True)
    nll = F.ctc_loss(lp64.transpose(0, 1), tg, il, tl, blank, reduction="none", zero_infinity=True)
    (g,) = torch.autograd.grad(nll.sum(), lp64)
    return nll.detach(), g


@pytest.mark.parametrize("b,t,v,s,seed", [(4, 50, 31, 12, 0), (3, 200, 31, 60, 1), (2, 1000, 31, 500, 2), (5, 64, 8, 20, 3), (2, 30, 5000, 9, 4), (2, 600, 5000, 400, 5),
                                          (3, 900, 1000, 511, 6)])
def test_ctc_loss_and_gradient_vs_torch(b, t, v, s, seed):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(seed)
    lp = torch.log_softmax(torch.randn(b, t, v, generator=g) * 2, -1)
    # few classes: many repeated neighbours; the long-target cases (seed >= 5) draw from 300 classes: repeats at a distance
    tg = torch.randint(1, min(v, 6 if seed < 5 else 300), (b, s), generator=g)
    il = torch.tensor([t - (7 * i) % max(1, t // 3) for i in range(b)], dtype=torch.int32)
    tl = torch.tensor([max(0, s - (5 * i) % (s + 1)) for i in range(b)], dtype=torch.int32)
    if b >= 3:
        il[1], tl[1] = min(t, 5), min(s, 12)                                    # more labels than frames: no alignment
        tl[2] = 0                                                               # empty target
    want_nll, want_g = _ref(lp, tg, il, tl)
    nll, grad = ops.ctc_loss_grad(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))
    torch.testing.assert_close(nll.cpu().double(), want_nll, rtol=2e-5, atol=2e-4)
    # fp32 log-space tables: alpha + beta + nll - lp cancels numbers of size |nll| (up to ~2000 here), so a posterior carries
    # an absolute error of a few ulp(|nll|); torch's own fp32 GPU kernel is compared on the same footing below
    tol = 2e-5 + 1.5e-6 * float(want_nll.abs().max())
    torch.testing.assert_close(grad.cpu().double(), want_g, rtol=1e-4, atol=tol)
    lpg = lp.to(DEV).requires_grad_(True)
    tnll = F.ctc_loss(lpg.transpose(0, 1), tg.to(DEV), il.to(DEV), tl.to(DEV), 0, reduction="none", zero_infinity=True)
    (tgrad,) = torch.autograd.grad(tnll.sum(), lpg)
    err_native = float((grad.cpu().double() - want_g).abs().max())
    err_torch = float((tgrad.cpu().double() - want_g).abs().max())
    print(f"CTC gradient max |error| vs fp64: native {err_native:.2e}, torch fp32 GPU kernel {err_torch:.2e}")
    assert err_native <= max(3.0 * err_torch, tol)
    nll2, grad2 = ops.ctc_loss_grad(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))
    assert torch.equal(nll, nll2) and torch.equal(grad, grad2)


def test_sb_ctc_loss_wrapper_native_vs_torch(monkeypatch):
    """sb_compat.ctc_loss ('batchmean', relative lengths) through the native op == through torch, value and gradient."""
    from mamba_asr_amd import sb_compat as sb
    g = torch.Generator().manual_seed(9)
    lp0 = torch.log_softmax(torch.randn(4, 120, 31, generator=g), -1)
    tg = torch.randint(1, 31, (4, 25), generator=g)
    il, tl = torch.tensor([1.0, 0.8, 0.55, 0.9]), torch.tensor([1.0, 0.6, 0.4, 0.8])
    res = {}
    for native in (True, False):
        monkeypatch.setattr(sb, "USE_NATIVE_CTC", native)
        lp = lp0.to(DEV).requires_grad_(True)
        loss = sb.ctc_loss(lp, tg.to(DEV), il.to(DEV), tl.to(DEV), 0, reduction="batchmean")
        (gr,) = torch.autograd.grad(loss, lp)
        res[native] = (loss.detach(), gr)
    torch.testing.assert_close(res[True][0], res[False][0], rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(res[True][1], res[False][1], rtol=1e-4, atol=1e-5)


def _nonfinite_case(v, s, t=60, seed=11):
    """Eight utterances, each with one kind of non-finite log-probability (or none), and the expected outcome under
    F.ctc_loss(zero_infinity=True): NaN or +inf on the lattice -> NaN loss and NaN gradient rows; an all -inf frame -> no
    alignment -> loss 0, gradient 0 (the only case zero_infinity zeroes); -inf at one target label -> finite loss, NaN at that
    gradient element; NaN in a padding frame or +inf at an absent class -> finite loss."""
    g = torch.Generator().manual_seed(seed)
    b = 8
    lp = torch.log_softmax(torch.randn(b, t, v, generator=g) * 2, -1)
    tg = torch.randint(1, v - 1, (b, s), generator=g)                          # class v - 1 never occurs in a target
    il = torch.full((b,), t, dtype=torch.int32)
    il[6] = t - 10
    tl = torch.full((b,), s, dtype=torch.int32)
    nan, inf = float("nan"), float("inf")
    lp[1, 17, tg[1, 3]] = nan                                                   # NaN at a target label
    lp[2, 5, 0] = nan                                                           # NaN at the blank
    lp[3, 30, tg[3, 0]] = inf                                                   # +inf at a target label
    lp[4, 12, tg[4, 2]] = -inf                                                  # -inf at a target label (other paths remain)
    lp[5, 40, :] = -inf                                                         # an all -inf frame: no alignment
    lp[6, t - 3, tg[6, 1]] = nan                                                # NaN past the utterance's length
    lp[7, 9, v - 1] = inf                                                       # +inf at a class absent from the target
    return lp, tg, il, tl


@pytest.mark.parametrize("v,s", [(31, 12), (5, 30)])
def test_ctc_nonfinite_log_probs_vs_torch(v, s):
    """NaN propagates (it used to come back as loss 0 / gradient 0, like an infeasible alignment); zero_infinity zeroes +inf
    only.  (31, 12) runs the list-walk gradient kernel, (5, 30) the per-class one."""
    from mamba_asr_amd import ops
    lp, tg, il, tl = _nonfinite_case(v, s)
    want_nll, want_g = _ref(lp, tg, il, tl)
    assert torch.isnan(want_nll).tolist() == [False, True, True, True, False, False, False, False]
    assert float(want_nll[5]) == 0.0
    nll, grad = ops.ctc_loss_grad(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))
    nll, grad = nll.cpu().double(), grad.cpu().double()
    assert torch.equal(torch.isnan(nll), torch.isnan(want_nll)), (nll, want_nll)
    torch.testing.assert_close(nll, want_nll, rtol=2e-5, atol=2e-4, equal_nan=True)
    assert torch.equal(torch.isnan(grad), torch.isnan(want_g))
    assert torch.equal(torch.isinf(grad), torch.isinf(want_g))
    tol = 2e-5 + 1.5e-6 * float(want_nll.nan_to_num(0.0).abs().max())
    torch.testing.assert_close(grad, want_g, rtol=1e-4, atol=tol, equal_nan=True)
    assert torch.equal(grad[5], torch.zeros_like(grad[5]))
    nll2, grad2 = ops.ctc_loss_grad(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV))      # deterministic, NaNs included
    assert torch.equal(nll2.cpu().double().nan_to_num(7.0), nll.nan_to_num(7.0))
    assert torch.equal(grad2.cpu().double().nan_to_num(7.0), grad.nan_to_num(7.0))


@pytest.mark.parametrize("poison", ["nan", "-inf frame"])
def test_sb_ctc_loss_wrapper_nonfinite_vs_torch_fp64(poison):
    """sb_compat.ctc_loss ('batchmean', relative lengths) on the native op against F.ctc_loss in fp64 on the CPU: a NaN in one
    utterance makes the batch loss NaN (Brain's non-finite check then skips the step); an infeasible utterance adds 0."""
    from mamba_asr_amd import sb_compat as sb
    assert sb.USE_NATIVE_CTC
    g = torch.Generator().manual_seed(13)
    lp0 = torch.log_softmax(torch.randn(4, 120, 31, generator=g), -1)
    tg = torch.randint(1, 31, (4, 25), generator=g)
    il, tl = torch.tensor([1.0, 0.8, 0.55, 0.9]), torch.tensor([1.0, 0.6, 0.4, 0.8])
    if poison == "nan":
        lp0[1, 10, 0] = float("nan")
    else:
        lp0[2, 20, :] = float("-inf")
    lp = lp0.to(DEV).requires_grad_(True)
    loss = sb.ctc_loss(lp, tg.to(DEV), il.to(DEV), tl.to(DEV), 0, reduction="batchmean")
    (gr,) = torch.autograd.grad(loss, lp)
    ref = lp0.double().requires_grad_(True)
    t = lp0.shape[1]
    rl = F.ctc_loss(ref.transpose(0, 1), tg, torch.round(il * t).int(), torch.round(tl * tg.shape[1]).int(), 0, reduction="sum",
                    zero_infinity=True) / 4
    (rg,) = torch.autograd.grad(rl, ref)
    assert bool(torch.isnan(loss)) == bool(torch.isnan(rl)) == (poison == "nan")
    torch.testing.assert_close(loss.detach().cpu().double(), rl.detach(), rtol=2e-5, atol=2e-4, equal_nan=True)
    assert torch.equal(torch.isnan(gr.cpu()), torch.isnan(rg))
    torch.testing.assert_close(gr.cpu().double(), rg, rtol=1e-4, atol=1e-5, equal_nan=True)
