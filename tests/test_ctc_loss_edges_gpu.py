"""cm_ctc_loss (csrc/ctc.hip) at its edges, every case inside guard bands (tests/guard_bands.py, G.two_step): a blank that is not class
0, both sides of the switch between the two gradient kernels, S = 0 (for one utterance and for the whole batch), 1, 63, 64, 65, 511
and the refused 512, T at the boundaries of the alpha / beta kernel's 8-step prefetch groups, input lengths 0 and 1, the feasibility
boundary of targets with repeats, V = 2, 64, 65.

Reference and tolerances are tests/test_ctc_native.py's: F.ctc_loss in fp64 on the CPU (its _ref); nll rtol 2e-5, atol 2e-4; gradient
rtol 1e-4, atol 2e-5 + 1.5e-6 max|nll|.  T <= 80 keeps |nll| small (the S = 511 case alone needs T = 1030).  On top of the tolerance
the header's exact zeros are compared with torch.equal in every case: the gradient of frames t >= input_lengths[b], and the whole
gradient (and loss 0) of an utterance without an alignment.

Guards: log_probs inside NaN with every frame at or past input_lengths[b] NaN as well; targets inside elements holding a valid class
that is absent from every target, the entries at or past target_lengths[b] too (read, it would take posterior mass from that class's
gradient); nll and grad inside sentinels; the alpha / beta tables in a scratch of exactly cm_ctc_workspace_floats.  Before any launch
the reference alone must say that each utterance is what the case claims: feasible, infeasible or empty.
"""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402
import test_ctc_native as TN  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, I32 = torch.float32, torch.int32
WORST = [0.0, 0.0]                      # the largest error / allowance of nll and of the gradient over the cases run so far


class _Spy:
    """ops._launch wrapped: the argument struct of every native launch (the addresses the kernel was really given)."""

    def __init__(self, monkeypatch):
        from mamba_asr_amd import ops
        self.calls = []
        real = ops._launch

        def launch(name, fn, args, units=0):
            self.calls.append((name, args))
            return real(name, fn, args, units)
        monkeypatch.setattr(ops, "_launch", launch)


def by_class(v, s):
    """Which gradient kernel cm_ctc_loss launches (csrc/ctc.hip, cm_ctc_loss): per-class reductions cost about 14 V issue slots per
    (utterance, step), the list walk about 3 S ceil(S / 64); the per-class kernel runs when 14 V <= 3 S ceil(S / 64)."""
    return 14 * v <= 3 * s * ((s + 63) // 64)


def _case(b, t, v, s, il, tl, blank=0, seed=0, repeats=True, targets=None):
    """-> (lp (b, t, v) fp32 log-softmax, targets (b, s) int64, il, tl int32, blank, absent): ``absent`` is a class that is neither the
    blank nor in any target (V = 2 has none: the one label class stands in).  repeats=False: no two neighbours are equal, so an
    utterance is feasible exactly when its frames are at least its labels."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * t + v + s)
    lp = torch.log_softmax(torch.randn(b, t, v, generator=g) * 2, -1)
    labels = [c for c in range(v) if c != blank]
    absent = labels[-1]
    pool = torch.tensor(labels[:-1] if v > 2 else labels)
    if targets is not None:
        tg = torch.tensor(targets, dtype=torch.int64)
    elif repeats or len(pool) < 2:
        tg = pool[torch.randint(0, len(pool), (b, s), generator=g)]
    else:
        idx = torch.randint(0, len(pool), (b, 1), generator=g)
        step = torch.randint(1, len(pool), (b, max(s, 1)), generator=g)
        tg = pool[((idx + torch.cumsum(step, 1)) % len(pool))[:, :s]]
    assert tg.shape == (b, s) and (v == 2 or not bool((tg == absent).any())) and not bool((tg == blank).any())
    return lp, tg.long(), torch.tensor(il, dtype=I32), torch.tensor(tl, dtype=I32), blank, absent


def _check(case, kinds, monkeypatch, side=None):
    """The reference's own verdict on the case, then plain and guarded launch, the file's tolerances and the exact zeros."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    lp, tg, il, tl, blank, absent = case
    b, t, v = lp.shape
    s = tg.shape[1]
    want_nll, want_g = TN._ref(lp, tg, il, tl, blank)
    raw = F.ctc_loss(lp.double().transpose(0, 1), tg, il, tl, blank, reduction="none", zero_infinity=False)
    verdict = ["empty" if int(tl[i]) == 0 else "infeasible" if math.isinf(float(raw[i])) else "feasible" for i in range(b)]
    assert verdict == list(kinds), (verdict, kinds)
    assert bool(torch.isfinite(want_nll).all()) and bool(torch.isfinite(want_g).all())
    for i, kind in enumerate(verdict):
        assert bool((want_g[i, int(il[i]):] == 0).all())
        if kind == "infeasible":
            assert float(want_nll[i]) == 0.0 and not bool(want_g[i].any())
        if kind == "feasible":
            assert float(want_nll[i]) > 0.0
    if side is not None:
        assert by_class(v, s) == (side == "per class"), (v, s, side)
    lp_k, tg_k = lp.clone(), tg.clone()
    for i in range(b):
        lp_k[i, int(il[i]):] = float("nan")
        tg_k[i, int(tl[i]):] = absent
    lp_k, tg_k, il_d, tl_d = lp_k.to(DEV), tg_k.to(DEV), il.to(DEV), tl.to(DEV)
    nws = int(N.lib().cm_ctc_workspace_floats(b, t, s))
    assert nws == 2 * b * t * (2 * s + 1)
    spy = _Spy(monkeypatch)

    def run(L):
        x = L.around(lp_k, rows=t)                                   # one utterance of NaN either side: an alpha / beta workgroup's reach
        tgv = L.ints(tg_k, absent, rows=2, unique=False) if s else tg_k
        ilv, tlv = L.ints(il_d, 0, unique=False), L.ints(tl_d, 0, unique=False)
        bufs = {"nll": L.out("nll", (b,), F32), "grad": L.out("grad", (b, t, v), F32, contiguous=True, rows=t, align=4),
                "workspace": L.scratch("workspace", nws)}
        nll, grad = ops.ctc_loss_grad(x, tgv, ilv, tlv, blank, bufs=bufs)
        assert nll is bufs["nll"] and grad is bufs["grad"]
        name, a = spy.calls[-1]
        assert name == "cm_ctc_loss" and a.workspace_floats == nws
        for f, w in dict(log_probs=x, targets=tgv if s else None, input_lengths=ilv, target_lengths=tlv, **bufs).items():
            assert (getattr(a, f) or None) == (None if w is None else w.data_ptr()), f"{f}: the wrapper copied it"
    outs = G.two_step(run, DEV)
    assert len(spy.calls) == 2
    nll, grad = outs["nll"].cpu().double(), outs["grad"].cpu().double()
    atol = 2e-5 + 1.5e-6 * float(want_nll.abs().max())
    r_nll = float(((nll - want_nll).abs() / (2e-4 + 2e-5 * want_nll.abs())).max())
    r_g = float(((grad - want_g).abs() / (atol + 1e-4 * want_g.abs())).max())
    WORST[0], WORST[1] = max(WORST[0], r_nll), max(WORST[1], r_g)
    print(f"ctc_loss b {b} T {t} V {v} S {s} blank {blank} il {il.tolist()} tl {tl.tolist()} "
          f"{'per class' if by_class(v, s) else 'list walk'}: nll err / allowance {r_nll:.3f}, gradient err / allowance {r_g:.3f} "
          f"(max|nll| {float(want_nll.abs().max()):.1f}); worst so far {WORST[0]:.3f} / {WORST[1]:.3f}")
    torch.testing.assert_close(nll, want_nll, rtol=2e-5, atol=2e-4)
    torch.testing.assert_close(grad, want_g, rtol=1e-4, atol=atol)
    for i, kind in enumerate(verdict):
        tail = outs["grad"][i, int(il[i]):]
        assert torch.equal(tail, torch.zeros_like(tail)), f"utterance {i}: the gradient past its {int(il[i])} frames is not exactly 0"
        if kind == "infeasible":
            assert float(outs["nll"][i]) == 0.0 and torch.equal(outs["grad"][i], torch.zeros_like(outs["grad"][i]))
    return outs


# V = 31, S = 12: 434 > 36, the list walk; V = 5, S = 30: 70 <= 90, the per-class kernel (tests/test_ctc_native.py's pair)
@pytest.mark.parametrize("v,s,side", [(31, 12, "list walk"), (5, 30, "per class")])
@pytest.mark.parametrize("where", ["zero", "last", "middle"])
def test_blank_index(where, v, s, side, monkeypatch):
    blank = {"zero": 0, "last": v - 1, "middle": v // 2}[where]
    t = 50 if v == 31 else 70                                        # 30 labels of 3 classes: about 10 repeats, 70 frames hold them
    case = _case(3, t, v, s, [t, t - 7, t - 3], [s, s - 5, 0], blank=blank, seed=1)
    _check(case, ["feasible", "feasible", "empty"], monkeypatch, side=side)


@pytest.mark.parametrize("s,side", [(72, "list walk"), (73, "per class")])
def test_gradient_kernel_switch(s, side, monkeypatch):
    """V = 31: 14 V = 434; S = 72: 3 x 72 x 2 = 432 < 434; S = 73: 3 x 73 x 2 = 438 >= 434 (by_class: the host code of cm_ctc_loss)."""
    assert (3 * s * 2 < 434) == (side == "list walk")
    _check(_case(2, 80, 31, s, [80, 78], [s, s - 9], seed=2, repeats=False), ["feasible", "feasible"], monkeypatch, side=side)


@pytest.mark.parametrize("v", [8, 31])
@pytest.mark.parametrize("s", [1, 63, 64, 65])
def test_target_length_edges(s, v, monkeypatch):
    """63, 64, 65 labels: the last lane of a wave's first pass over the labels, a full pass, one label in the second.  V = 8 takes the
    per-class kernel from S = 63 on, V = 31 the list walk throughout."""
    assert by_class(v, s) == (v == 8 and s >= 63)
    _check(_case(2, 80, v, s, [80, 77], [s, max(s - 2, 1)], seed=3, repeats=False), ["feasible", "feasible"], monkeypatch)


def test_no_labels_in_the_whole_batch(monkeypatch):
    """targets (b, 0): an empty tensor has no address, the library takes NULL exactly when S == 0.  The loss is the blank path's."""
    outs = _check(_case(2, 5, 4, 0, [5, 3], [0, 0], seed=4), ["empty", "empty"], monkeypatch)
    assert bool((outs["nll"] > 0).all())


def test_no_labels_in_one_utterance(monkeypatch):
    _check(_case(3, 20, 6, 4, [20, 20, 11], [4, 0, 3], seed=5), ["feasible", "empty", "feasible"], monkeypatch)


def test_511_labels_fill_the_alpha_beta_workgroup(monkeypatch):
    """S = 511: 1023 extended labels on 1024 threads, 8 labels in every lane of the gradient kernel."""
    assert by_class(8, 511)
    _check(_case(1, 1030, 8, 511, [1030], [511], seed=6, repeats=False), ["feasible"], monkeypatch)


def test_512_labels_are_refused_without_a_launch(monkeypatch):
    """ops.ctc_supported is false, sb_compat.ctc_loss takes torch's kernel, and the C entry returns CM_EUNSUPPORTED (-2) before it
    launches anything: the sentinel-filled outputs and the NaN workspace stay as they were."""
    from mamba_asr_amd import ops, sb_compat as sb
    spy = _Spy(monkeypatch)
    b, t, v, s = 1, 1030, 8, 512
    lp, tg, il, tl, _, _ = _case(b, t, v, s, [t], [s], seed=7, repeats=False)
    assert not ops.ctc_supported(lp.to(DEV), tg.to(DEV)) and ops.ctc_supported(lp.to(DEV), tg[:, :511].to(DEV))
    x = lp.to(DEV).requires_grad_(True)
    loss = sb.ctc_loss(x, tg.to(DEV), torch.ones(1, device=DEV), torch.ones(1, device=DEV), 0, reduction="batchmean")
    (gr,) = torch.autograd.grad(loss, x)
    assert not spy.calls                                             # torch's kernel, not ours
    want_nll, want_g = TN._ref(lp, tg, il, tl)
    torch.testing.assert_close(loss.detach().cpu().double(), want_nll.sum(), rtol=2e-5, atol=2e-4)
    torch.testing.assert_close(gr.cpu().double(), want_g, rtol=1e-4, atol=2e-5 + 1.5e-6 * float(want_nll.abs().max()))
    g = G.Guards(DEV)
    bufs = {"nll": g.out("nll", (b,), F32), "grad": g.out("grad", (b, t, v), F32, contiguous=True, rows=4, align=4),
            "workspace": g.scratch("workspace", 2 * b * t * (2 * s + 1), F32)}
    with pytest.raises(RuntimeError, match=r"cm_ctc_loss failed \(code -2\)"):
        ops.ctc_loss_grad(lp.to(DEV), tg.to(DEV), il.to(DEV), tl.to(DEV), bufs=bufs)
    torch.cuda.synchronize()
    for name, (buf, view, outside) in g.items.items():
        G.assert_untouched(buf, outside, name)
        assert bool(torch.isnan(view).all()) if name == "workspace" else bool((view == G.SENTINEL).all()), f"{name} was written"


@pytest.mark.parametrize("t", [1, 8, 9, 10, 17])
def test_frame_count_edges(t, monkeypatch):
    """The alpha / beta loop starts at step 1 and runs in groups of 8 with the next 8 steps' log-probabilities in flight: T = 1 has no
    step, 8 ends inside the first group, 9 fills it, 10 and 17 begin the second and the third.  The second utterance is one frame
    shorter: its own T is what its workgroups count to."""
    s = min(3, t)
    short = max(t - 1, 1)
    case = _case(2, t, 6, s, [t, short], [s, min(s, 1) if t == 1 else s - 1], seed=8, repeats=False)
    _check(case, ["feasible", "feasible"], monkeypatch)


def test_input_length_zero(monkeypatch):
    """An utterance without a frame: labels cannot be emitted (loss 0, gradient exactly 0); no labels either: the empty alignment."""
    _check(_case(3, 12, 6, 3, [12, 0, 0], [3, 2, 0], seed=9), ["feasible", "infeasible", "empty"], monkeypatch)


def test_input_length_one(monkeypatch):
    _check(_case(3, 5, 6, 2, [1, 1, 1], [0, 1, 2], seed=10), ["empty", "feasible", "infeasible"], monkeypatch)


def test_feasibility_boundary_of_repeated_labels(monkeypatch):
    """[1, 1, 2, 2, 1] needs 5 labels + 2 blanks between the repeats: finite at 7 frames, no alignment at 6."""
    tg = [[1, 1, 2, 2, 1]] * 2
    outs = _check(_case(2, 7, 5, 5, [7, 6], [5, 5], seed=11, targets=tg), ["feasible", "infeasible"], monkeypatch)
    assert float(outs["nll"][0]) > 0.0
    # and with one label less for the same 6 frames: [1, 1, 2, 2] needs 6
    _check(_case(2, 7, 5, 5, [6, 5], [4, 4], seed=12, targets=tg), ["feasible", "infeasible"], monkeypatch)


@pytest.mark.parametrize("v", [2, 64, 65])
def test_vocabulary_edges(v, monkeypatch):
    """V = 2: blank and one label, so every neighbour repeats (3 labels need 5 frames: the second utterance has 4); 64 and 65: the
    last lane of the gradient row's first pass, and one class in its second."""
    if v == 2:
        _check(_case(2, 9, 2, 3, [9, 4], [3, 3], seed=13), ["feasible", "infeasible"], monkeypatch)
    else:
        _check(_case(2, 12, v, 5, [12, 9], [5, 4], blank=v - 1, seed=14), ["feasible", "feasible"], monkeypatch)


@pytest.mark.parametrize("s", [6, 0], ids=["labels", "all_empty"])
def test_sb_wrapper_with_the_last_class_as_blank(s, monkeypatch):
    """sb_compat.ctc_loss(blank_index=V - 1, reduction="batchmean") on the native kernel against the fp64 reference, value and
    gradient; the batch whose targets are all empty too.  The file's tolerances, the gradient's divided by the batch as the loss is."""
    from mamba_asr_amd import sb_compat as sb
    assert sb.USE_NATIVE_CTC
    spy = _Spy(monkeypatch)
    b, t, v = 3, 20, 7
    lp, tg, _, _, blank, _ = _case(b, t, v, s, [t] * b, [s] * b, blank=v - 1, seed=15, repeats=False)
    il_rel, tl_rel = torch.tensor([1.0, 0.75, 0.5]), torch.tensor([1.0, 0.5, 0.0])
    x = lp.to(DEV).requires_grad_(True)
    loss = sb.ctc_loss(x, tg.to(DEV), il_rel.to(DEV), tl_rel.to(DEV), blank, reduction="batchmean")
    (gr,) = torch.autograd.grad(loss, x)
    assert [name for name, _ in spy.calls] == ["cm_ctc_loss"]
    il, tl = torch.round(il_rel * t).int(), torch.round(tl_rel * s).int()
    want_nll, want_g = TN._ref(lp, tg, il, tl, blank)
    assert bool(torch.isfinite(want_nll).all()) and bool((want_nll > 0).all())
    torch.testing.assert_close(loss.detach().cpu().double(), want_nll.sum() / b, rtol=2e-5, atol=2e-4)
    torch.testing.assert_close(gr.cpu().double(), want_g / b, rtol=1e-4, atol=(2e-5 + 1.5e-6 * float(want_nll.abs().max())) / b)
    for i in range(b):
        assert not bool(gr[i, int(il[i]):].any())
