"""The mixer's tail as one kernel: cm_ln_pw_glu with out_proj in front (cm_ln_pw_glu_mix, ops.ln_pw_glu(..., ycat=, out_w=)).

  * against fp64 torch on the CPU of the same formula (no rounding of y), beside the two-launch route it replaces
    (torch.mm + ops.ln_pw_glu): both round y to bf16 at the same point and differ only in the fp32 summation order of one
    GEMM, so the new kernel must stay within 1.5 x the two-launch route's max abs error (the factor covers the fluctuation
    of a maximum over elements);
  * bit-for-bit: a token's outputs depend neither on its position nor on the launch's row count; x_out may alias x; repeats
    give the same bits;
  * the encoder route: no library GEMM between the scan and cm_ln_pw_glu; CM_MIXER_TAIL=0 restores it;
  * the entry point refuses what the kernel does not take, without a launch (CPU).
"""
import ctypes as C
import importlib.util
import os

import pytest
import torch
import torch.nn as nn

DEV = "cuda"
D, K = 256, 1024
ROWS = (1, 63, 64, 65, 200)


def _case(rows, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(rows, D), ycat=r(rows, K).bfloat16(), wo=(r(D, K) * 0.05).bfloat16(), w=(r(2 * D, D) * 0.05).bfloat16(),
                bias=r(2 * D) * 0.1, ln_g=1.0 + 0.1 * r(D), ln_b=0.1 * r(D), eps=1e-5)


def _reference(c):
    """fp64, y not rounded: x_out = x + ycat @ Wo^T; g = GLU(LN(x_out) @ W^T + b)."""
    y = c["ycat"].double() @ c["wo"].double().t()
    xo = c["x"].double() + y
    h = torch.nn.functional.layer_norm(xo, (D,), c["ln_g"].double(), c["ln_b"].double(), c["eps"])
    pw = h @ c["w"].double().t() + c["bias"].double()
    return xo, pw[:, :D] * torch.sigmoid(pw[:, D:])


class _Dev:
    def __init__(self, c):
        from mamba_asr_amd import ops
        self.x, self.ycat, self.wo = c["x"].to(DEV), c["ycat"].to(DEV), c["wo"].to(DEV)
        self.ln = (c["ln_g"].to(DEV), c["ln_b"].to(DEV), c["eps"])
        self.wp, self.wop, self.bias = ops.PackedWeight(c["w"].to(DEV)), ops.PackedWeight(self.wo), c["bias"].to(DEV)

    def mix(self, x=None, ycat=None, x_out="new"):
        from mamba_asr_amd import ops
        x = self.x if x is None else x
        xo = torch.empty_like(x) if isinstance(x_out, str) else x_out
        g = ops.ln_pw_glu(x, None, 1.0, self.ln, self.wp, self.bias, x_out=xo, ycat=self.ycat if ycat is None else ycat, out_w=self.wop)
        return xo, g

    def pair(self):
        from mamba_asr_amd import ops
        xo = torch.empty_like(self.x)
        g = ops.ln_pw_glu(self.x, torch.mm(self.ycat, self.wo.t()), 1.0, self.ln, self.wp, self.bias, x_out=xo)
        return xo, g


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
def test_mix_kernel_vs_fp64_beside_the_two_launch_route(rows):
    """Max abs error against fp64 measured on MI355X, two launches (torch.mm + cm_ln_pw_glu) / one kernel -- identical to the digits
    printed, the bf16 rounding of y dominates both:
        rows   1: x_out 1.001e-02 / 1.001e-02, gated 4.043e-03 / 4.043e-03
        rows  63: x_out 1.548e-02 / 1.548e-02, gated 7.448e-03 / 7.448e-03
        rows  64: x_out 1.562e-02 / 1.562e-02, gated 8.047e-03 / 8.047e-03
        rows  65: x_out 1.562e-02 / 1.562e-02, gated 8.173e-03 / 8.173e-03
        rows 200: x_out 1.560e-02 / 1.560e-02, gated 8.302e-03 / 8.302e-03"""
    c = _case(rows)
    want_x, want_g = _reference(c)
    d = _Dev(c)
    err = {}
    for name, fn in (("pair", d.pair), ("mix", d.mix)):
        xo, g = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(xo).all() and torch.isfinite(g.float()).all()
        err[name] = ((xo.cpu().double() - want_x).abs().max().item(), (g.cpu().double() - want_g).abs().max().item())
    print(f"rows {rows}: max|err| vs fp64  x_out: two launches {err['pair'][0]:.3e}, one kernel {err['mix'][0]:.3e};  "
          f"gated: two launches {err['pair'][1]:.3e}, one kernel {err['mix'][1]:.3e}")
    assert err["mix"][0] <= 1.5 * err["pair"][0]
    assert err["mix"][1] <= 1.5 * err["pair"][1]


@pytest.mark.gpu
def test_token_outputs_do_not_depend_on_position_or_row_count():
    c = _case(200, seed=1)
    d = _Dev(c)
    xo, g = d.mix()
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(5)).to(DEV)
    xo_p, g_p = d.mix(x=d.x[perm].contiguous(), ycat=d.ycat[perm].contiguous())
    assert torch.equal(xo_p, xo[perm]) and torch.equal(g_p, g[perm])
    for n in (1, 63, 65):                                            # another launch size, another tile position for most rows
        xo_n, g_n = d.mix(x=d.x[200 - n:].contiguous(), ycat=d.ycat[200 - n:].contiguous())
        assert torch.equal(xo_n, xo[200 - n:]) and torch.equal(g_n, g[200 - n:])


@pytest.mark.gpu
def test_x_out_may_alias_x():
    d = _Dev(_case(200, seed=2))
    xo, g = d.mix()
    x2 = d.x.clone()
    xo2, g2 = d.mix(x=x2, x_out=x2)
    assert xo2.data_ptr() == x2.data_ptr() and torch.equal(xo2, xo) and torch.equal(g2, g)


@pytest.mark.gpu
def test_repeats_give_the_same_bits_at_32000_rows():
    g_ = torch.Generator(device=DEV).manual_seed(3)
    c = _case(1, seed=3)
    d = _Dev(c)
    x = torch.randn(32000, D, device=DEV, generator=g_)
    ycat = torch.randn(32000, K, device=DEV, generator=g_).bfloat16()
    first = d.mix(x=x, ycat=ycat)
    for _ in range(5):
        again = d.mix(x=x, ycat=ycat)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    # and the tiles agree with a small launch of the same rows
    tail = d.mix(x=x[31936:].contiguous(), ycat=ycat[31936:].contiguous())
    assert torch.equal(tail[0], first[0][31936:]) and torch.equal(tail[1], first[1][31936:])


# ---- the encoder route -------------------------------------------------------------------------------------------------
_spec = importlib.util.spec_from_file_location("golden_synth", os.path.join(os.path.dirname(__file__), "golden", "synth.py"))
S = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(S)
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
LAYER = ["cm_ffn_fused", "cm_conv_xproj", "cm_scan_cl_fwd", "cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu", "cm_ffn_fused"]


def _large_encoder():
    """The 2-layer d_model-256 encoder of test_hip_parity_r2 (reference golden g4_large)."""
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    enc = ConmambaEncoder(num_layers=2, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True, dropout=0.0,
                          causal=False, mamba_config=dict(CFG))
    enc.load_state_dict(S.synth_like(enc, 256), strict=True)
    return enc.to(DEV).eval(), S.synth_input("g4_large.x", (16, 100, 256), 256).to(DEV)


def _run_logged(enc, x, monkeypatch):
    """-> (output, native launches in order, number of library out_proj GEMMs)."""
    from mamba_asr_amd import fused, ops
    gemms = []
    real = fused._out_proj
    monkeypatch.setattr(fused, "_out_proj", lambda c, ycat: (gemms.append(1), real(c, ycat))[1])
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            out = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=1)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    return out, names, len(gemms)


@pytest.mark.gpu
def test_encoder_layer_has_no_library_gemm_and_the_switch_restores_it(golden, monkeypatch):
    from mamba_asr_amd import fused
    g = golden("g4_large")
    enc, x = _large_encoder()
    monkeypatch.setattr(fused, "USE_MIXER_TAIL", True)
    out, names, gemms = _run_logged(enc, x, monkeypatch)
    assert names == LAYER * 2, names                                 # six native launches per layer, nothing else
    assert gemms == 0, "a library out_proj GEMM ran between the scan and cm_ln_pw_glu"
    torch.testing.assert_close(out.float().cpu(), g["y_enc"], rtol=3e-2, atol=5e-2)
    assert (out.float().cpu() - g["y_enc"]).abs().mean() < 6e-3
    monkeypatch.setattr(fused, "USE_MIXER_TAIL", False)              # CM_MIXER_TAIL=0
    out0, names0, gemms0 = _run_logged(enc, x, monkeypatch)
    assert names0 == LAYER * 2 and gemms0 == 2
    torch.testing.assert_close(out0.float().cpu(), g["y_enc"], rtol=3e-2, atol=5e-2)
    assert (out0.float().cpu() - g["y_enc"]).abs().mean() < 6e-3


# ---- argument refusal: no GPU, no launch -------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_launch():
    import mamba_asr_amd._native as N
    lib = N.lib()
    assert lib.cm_ln_pw_glu_mix(None) == -1

    def args(**over):
        a = N.LnPwGluMixArgs()
        a.rows, a.dim, a.proj_k, a.alpha, a.eps = 64, 256, 1024, 1.0, 1e-5
        # distinct, 16-byte aligned, far apart; never dereferenced: every case below is refused before a launch
        for i, k in enumerate(("x", "ln_g", "ln_b", "w", "bias", "x_out", "out", "ycat", "proj_w")):
            setattr(a, k, C.cast(C.c_void_p(0x10000000 * (i + 1)), dict(N.LnPwGluMixArgs._fields_)[k]))
        for k, v in over.items():
            if isinstance(v, int) and k not in ("rows", "dim", "proj_k"):
                v = C.cast(C.c_void_p(v), dict(N.LnPwGluMixArgs._fields_)[k]) if v else None
            setattr(a, k, v)
        return a

    for bad in (dict(ycat=0), dict(proj_w=0), dict(x=0), dict(out=0), dict(rows=0)):
        assert lib.cm_ln_pw_glu_mix(C.byref(args(**bad))) == -1, bad                     # CM_EINVAL
    for bad in (dict(dim=128), dict(proj_k=96), dict(proj_k=1056), dict(proj_k=0), dict(proj_k=16384)):
        assert lib.cm_ln_pw_glu_mix(C.byref(args(**bad))) == -2, bad                     # CM_EUNSUPPORTED
    for bad in (dict(ycat=0x80000008), dict(proj_w=0x90000004), dict(x=0x10000004), dict(out=0x70000002)):
        assert lib.cm_ln_pw_glu_mix(C.byref(args(**bad))) == -3, bad                     # CM_EALIGN: misaligned
    for bad in (dict(out=0x80000000), dict(out=0x10000000), dict(x_out=0x80000100), dict(x_out=0x10000400), dict(out=0x60000000)):
        assert lib.cm_ln_pw_glu_mix(C.byref(args(**bad))) == -3, bad                     # CM_EALIGN: output overlaps an input
    assert b"ln_pw_glu_mix" in lib.cm_last_error()
