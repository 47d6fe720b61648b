"""The folded scan (GPU): cm_scan_cl_fwd_fold / cm_scan_cl_fwd_fold_lens write out = (p_f + p_b) * SiLU(z) into ONE tensor,
as two launches with the pre-gate value of whichever direction reaches a row first stored in between as two bf16 pieces (the rounded
value in the output tensor, what the rounding dropped in the workspace), so that the result has one bf16 rounding.

Kernel level, batch 3, dim 64 / 200 (a partial channel group) / 512, seqlen across one block, odd and even block counts, a ragged last
block and mid = 0; lens = LENS_A of tests/test_ragged_encoder_gpu.py, zeros included:
  * against fp64 -- the oracle's pre-gate scans of both directions on the bf16-rounded inputs and the bf16-rounded dt_proj weight
    (test_scan_rows_two_directions' recipe), every element, at a DERIVED bound:
    |got - ref| <= 2^-8 (|p_f| + |p_b|) |SiLU(z)| + the fp32-recurrence term.  It is what the two bf16 roundings of the two-tensor
    route allow (y_f and y_b each rounded once, 2^-8 relative).  A p stored as ONE bf16 value misses it (round-to-nearest errs by up
    to 2^-8 per rounding, so p's rounding and the result's add up to 2^-8 (|p_first| + |p_f + p_b|) |SiLU(z)|: measured 1.66 x the
    bound); with the remainder carried the only bf16 rounding left is the result's, 2^-8 |p_f + p_b| |SiLU(z)|, and the measured
    worst error / bound is 0.94.  The fp32 term is the tolerance the fp32-I/O row-group kernel is held to against this oracle (test_scan_rows_two_directions /
    SCAN_TOL[F32] of tests/test_forward_guards_gpu.py: rtol 2e-4, atol 5e-5) once per direction:
    2 * 5e-5 + 2e-4 (|p_f| + |p_b|) |SiLU(z)|;
  * guard bands in the same launches: sentinels around the output and the workspace (NaN inside the workspace), NaN around u, z and
    xdbl, under lens also at and past lens[b], output rows past lens[b] untouched;
  * bit for bit: a ragged batch under lens against each utterance alone, a permuted batch, two runs, a captured graph's replay.
Encoder level, 2 layers, d_model 256 (golden g4_large): fold on against the reference golden at test_seqpar.py's bound (rtol 3e-2,
atol 5e-2), against fold off (difference printed), the launch log equal to today's names; CM_SCAN_FOLD=0 bit for bit against the
two-tensor route spelled out launch by launch."""
import ctypes
import functools
import importlib.util
import os
import sys

import pytest
import torch
import torch.nn as nn

from oracle import conmamba_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402
from test_ragged_encoder_gpu import LENS_A  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NAN = float("nan")
COLS = dict(rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
RANK, P, RW = 9, 16, 48
RTOL32, ATOL32 = 2e-4, 5e-5                # the fp32-I/O row-group scan against this oracle (test_scan_rows_two_directions)
FILL = 7.0                                 # what the output holds before a launch under lens: rows past lens[b] keep it
SEQLENS = [1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 70]
DIMS = [64, 200, 512]
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
LAYER = ["cm_ffn_fused", "cm_conv_xproj", "cm_scan_cl_fwd", "cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu", "cm_ffn_fused"]


def dev(t):
    return t.to(DEV)


@functools.lru_cache(maxsize=None)
def _case(b, l, e):
    """test_scan_rows_two_directions' recipe: x_dbl rows [dt 16 | B | C] per direction, everything the kernel reads rounded to bf16."""
    from mamba_asr_amd import ops
    gen = torch.Generator().manual_seed(l * 11 + e + RANK + b)
    xz = torch.randn(b, l, 2 * e, generator=gen).to(BF16)
    ucat = torch.randn(b, l, 2 * e, generator=gen).to(BF16)
    xcat = torch.randn(b, l, 2 * RW, generator=gen)
    par = []
    for i, rev in enumerate((False, True)):
        xcat[:, :, RW * i + RANK:RW * i + P] = 0.0
        A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
        Wdt = torch.randn(e, RANK, generator=gen) * 0.3
        D, bias = torch.randn(e, generator=gen), torch.randn(e, generator=gen) - 1
        par.append(dict(A=dev(A), D=dev(D), bias=dev(bias), W=ops.pad_dt_weight(dev(Wdt)), rev=rev, host=(A, Wdt, D, bias)))
    xq = xcat.to(BF16)
    return dict(b=b, l=l, e=e, host=(xz, ucat, xq), xz=dev(xz), ucat=dev(ucat), xcat=dev(xq), par=par)


def _reference(c, b, n):
    return _reference_of(c["b"], c["l"], c["e"], b, n)


@functools.lru_cache(maxsize=None)
def _reference_of(nb, l, e, b, n):
    """fp64, utterance b of _case(nb, l, e) alone on its first n rows -> (p_f, p_b, SiLU(z)), each (n, e): the oracle's scan without z
    is the pre-gate value sum_n C h + D u.  Computed once, shared, left unchanged."""
    c = _case(nb, l, e)
    xz, ucat, xq = c["host"]
    e = c["e"]
    tr = lambda t: t.double().transpose(1, 2)
    ps = []
    for i, p in enumerate(c["par"]):
        A, Wdt, D, bias = p["host"]
        xd = xq[b:b + 1, :n, RW * i:RW * (i + 1)].double()
        delta = torch.einsum("er,blr->bel", Wdt.to(BF16).double(), xd[:, :, :RANK])
        f = (lambda t: t.flip(-1)) if p["rev"] else (lambda t: t)
        ref = O.selective_scan(f(tr(ucat[b:b + 1, :n, e * i:e * (i + 1)])), f(delta), A, f(xd[:, :, P:P + 16].transpose(1, 2)),
                               f(xd[:, :, P + 16:].transpose(1, 2)), D, None, bias, True, work_dtype=torch.float64)
        ps.append(f(ref).transpose(1, 2)[0])
    z = xz[b, :n, e:].double()
    return ps[0], ps[1], z * torch.sigmoid(z)


def _within_bound(got, c, b, n, what):
    """Every element of got (n, e) against fp64 at the bound of the module docstring."""
    pf, pb, s = _reference(c, b, n)
    mag = (pf.abs() + pb.abs()) * s.abs()
    bound = 2.0 ** -8 * mag + (2 * ATOL32 + RTOL32 * mag)
    err = (got.detach().double().cpu() - (pf + pb) * s).abs()
    worst = float((err / bound).max())
    print(f"{what}: max |got - ref| {float(err.max()):.3e}, worst error / bound {worst:.3f}")
    assert bool(torch.isfinite(err).all()) and bool((err <= bound).all()), \
        f"{what}: {int((~(err <= bound)).sum())} of {err.numel()} element(s) over the bound, worst error / bound {worst:.3f}"


def _dirs(c, ucat, xcat, out, vec=lambda t: t):
    e = c["e"]
    dirs = [dict(u=ucat[:, :, e * i:e * (i + 1)], xdbl=xcat[:, :, RW * i:RW * (i + 1)], A=vec(p["A"]), D=vec(p["D"]), delta_bias=vec(p["bias"]),
                 dt_weight=vec(p["W"]), reverse=p["rev"]) for i, p in enumerate(c["par"])]
    dirs[0]["out"] = out
    return dirs


def _fold(c, idx=None, n=None, lens=None):
    """The fold on plain tensors: utterances ``idx`` (all), their first ``n`` rows (all), under ``lens`` (none).  -> (batch, n, e) bf16."""
    from mamba_asr_amd import ops
    e, n = c["e"], c["l"] if n is None else n
    pick = (lambda t: t[:, :n]) if idx is None else (lambda t: t[idx][:, :n])
    xz, ucat, xcat = pick(c["xz"]), pick(c["ucat"]), pick(c["xcat"])
    out = torch.full((xz.shape[0], n, e), FILL, dtype=BF16, device=DEV)
    ret = ops.scan_cl_fwd(_dirs(c, ucat, xcat, out), z=xz[:, :, e:], delta_softplus=True, time_chunks=1, lens=lens, whole=lens is not None, fold=True)
    assert len(ret) == 1 and ret[0].data_ptr() == out.data_ptr()
    return out


def _fold_guarded(c, lens=None):
    """Plain launch, then the guarded one (guard_bands.two_step): NaN around u, z, xdbl and the small vectors, x half of [x | z] NaN,
    sentinels around the output and the workspace, NaN inside the workspace; under ``lens`` (a list) NaN at and past lens[b] in u, z
    and xdbl in BOTH launches, the output FILL before the launch.  -> the plain launch's output."""
    from mamba_asr_amd import ops
    b, l, e = c["b"], c["l"], c["e"]
    lens_t = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=DEV)

    def run(L):
        xz, ucat, xcat = L.cols(c["xz"], dead=(0, e)), L.cols(c["ucat"]), L.cols(c["xcat"])
        for i, n in enumerate(lens or []):
            xz[i, n:], ucat[i, n:], xcat[i, n:] = NAN, NAN, NAN
        out = L.out("y", (b, l, e), BF16, fill=FILL if lens is not None else None, **COLS)
        ws = L.scratch("ws", 2 * b * e * 16 + b * l * e // 2)     # fp32 elements: the states, then the bf16 remainder plane
        ret = ops.scan_cl_fwd(_dirs(c, ucat, xcat, out, L.vec), z=xz[:, :, e:], delta_softplus=True, time_chunks=1, lens=lens_t,
                              whole=lens is not None, fold=True, workspace=ws)
        assert len(ret) == 1 and ret[0].data_ptr() == out.data_ptr()
    return G.two_step(run, DEV)["y"]


@functools.lru_cache(maxsize=None)
def _plain(b, l, e):
    return _fold(_case(b, l, e))


@pytest.mark.parametrize("l", SEQLENS)
@pytest.mark.parametrize("e", DIMS)
def test_fold_guard_bands(e, l):
    from mamba_asr_amd import _native as N
    a = N.ScanClArgs()
    a.batch, a.seqlen, a.dim = 3, l, e
    assert N.lib().cm_scan_cl_fwd_fold_workspace_bytes(ctypes.byref(a)) == 2 * 3 * e * 16 * 4 + 3 * l * e * 2
    assert torch.equal(_fold_guarded(_case(3, l, e)), _plain(3, l, e))


@pytest.mark.parametrize("l", SEQLENS)
@pytest.mark.parametrize("e", DIMS)
def test_fold_against_fp64(e, l):
    """The bound of the module docstring: 2^-8 (|p_f| + |p_b|) |SiLU(z)| + the fp32 term, every element."""
    c, y = _case(3, l, e), _plain(3, l, e)
    for b in range(3):
        _within_bound(y[b], c, b, l, f"dim {e}, seqlen {l}, utterance {b}")


@functools.lru_cache(maxsize=None)
def _under_lens(e):
    c = _case(len(LENS_A), max(LENS_A), e)
    return c, _fold_guarded(c, LENS_A)


@pytest.mark.parametrize("e", DIMS)
def test_fold_under_lens(e):
    """LENS_A in one batch of 70 rows: guard bands with NaN at and past lens[b]; rows past lens[b] untouched; every utterance
    bit-equal to the fold on that utterance alone with seqlen = lens[b]."""
    c, y = _under_lens(e)
    for b, n in enumerate(LENS_A):
        assert bool((y[b, n:] == FILL).all()), f"utterance {b}: rows at and past {n} were written"
        if n:
            alone = _fold(c, idx=[b], n=n)
            assert torch.equal(y[b, :n], alone[0]), f"utterance {b} ({n} rows) under lens differs from the fold on it alone"


@pytest.mark.parametrize("e", DIMS)
def test_fold_under_lens_against_fp64(e):
    c, y = _under_lens(e)
    for b, n in enumerate(LENS_A):
        if n:
            _within_bound(y[b, :n], c, b, n, f"dim {e}, lens {n}")


def test_bits_do_not_depend_on_batch_order_run_or_graph():
    c = _case(3, 49, 200)
    base = _fold(c)
    assert torch.equal(_fold(c), base), "two runs of one build differ"
    perm = [2, 0, 1]
    assert torch.equal(_fold(c, idx=perm), base[perm]), "a permuted batch differs from the permuted output"
    lens = torch.tensor([49, 17, 0], dtype=torch.int32, device=DEV)
    under = _fold(c, lens=lens)
    assert torch.equal(_fold(c, idx=perm, lens=lens[perm].contiguous()), under[perm]), "a permuted ragged batch differs"
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _fold(c)
        out_l = _fold(c, lens=lens)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, base), "a captured graph's replay differs from eager"
    assert torch.equal(out_l, under), "a captured graph's replay under lens differs from eager"


# ------------------------------------------------------------------------------------------------------------------------ encoder
@pytest.fixture(scope="module")
def enc_case():
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(os.path.dirname(__file__), "golden", "synth.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    enc = ConmambaEncoder(num_layers=2, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True, dropout=0.0,
                          causal=False, mamba_config=dict(CFG))
    enc.load_state_dict(S.synth_like(enc, 256), strict=True)
    return enc.to(DEV).eval(), S.synth_input("g4_large.x", (16, 100, 256), 256).to(DEV)


def _logged(enc, x, monkeypatch, fold):
    """encoder_forward with the switch at ``fold`` -> (output, launch names and units, the fold arguments the scans were called with)."""
    from mamba_asr_amd import fused, ops
    monkeypatch.setattr(fused, "USE_SCAN_FOLD", fold)
    real, seen = ops.scan_cl_fwd, []

    def spy(*a, **k):
        seen.append(bool(k.get("fold", False)))
        return real(*a, **k)

    monkeypatch.setattr(ops, "scan_cl_fwd", spy)
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            out = fused.encoder_forward(enc, x, dtype=BF16, streams=1)
        torch.cuda.synchronize()
        log = [(e[0], e[3]) for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
        monkeypatch.setattr(ops, "scan_cl_fwd", real)
    return out, log, seen


def test_encoder_with_the_fold_against_the_reference_golden(enc_case, golden, monkeypatch):
    enc, x = enc_case
    rows = x.shape[0] * x.shape[1]
    on, log_on, seen_on = _logged(enc, x, monkeypatch, True)
    off, log_off, seen_off = _logged(enc, x, monkeypatch, False)
    assert seen_on == [True, True] and seen_off == [False, False]
    torch.testing.assert_close(on.cpu(), golden("g4_large")["y_enc"], rtol=3e-2, atol=5e-2)
    err = (on - off).abs()
    print(f"fold on against fold off: max |diff| {float(err.max()):.3e}, mean {float(err.mean()):.3e}")
    assert log_on == log_off == [(n, rows * (2 if n == "cm_scan_cl_fwd" else 1)) for n in LAYER * 2], log_on


def test_switch_off_is_the_two_tensor_route_bit_for_bit(enc_case, monkeypatch):
    """CM_SCAN_FOLD=0 against the route of before the fold, launch by launch: [y_fwd | y_bwd] from one cm_scan_cl_fwd, out_proj over
    K = 2E in the mixer's tail."""
    from mamba_asr_amd import fused, ops
    enc, x = enc_case
    off, _, seen = _logged(enc, x, monkeypatch, False)
    assert seen == [False, False]
    batch, seqlen, _ = x.shape
    caches = [fused._cache(layer, BF16) for layer in enc.layers]
    E, fin = caches[0].d_inner, fused._final_norm(enc)
    with torch.no_grad(), torch.autocast("cuda", enabled=False):
        r = fused._residual_rows(x)
        xz, ucat, ycat = (torch.empty((batch, seqlen, 2 * E), dtype=BF16, device=DEV) for _ in range(3))
        xdbl = torch.empty((batch, seqlen, 2 * caches[0].row_width), dtype=BF16, device=DEV)
        for li, c in enumerate(caches):
            fused._head(c, r, xz, ucat, xdbl)
            ops.scan_cl_fwd(fused._scan_dirs(c, ucat, ycat, batch, seqlen, xdbl), z=xz[:, :, E:], delta_softplus=True)
            want = fused._tail(c, r, ycat.view(batch * seqlen, 2 * E), batch, seqlen, fin if li == len(caches) - 1 else None)
    assert torch.equal(off, want.view(batch, seqlen, -1))
