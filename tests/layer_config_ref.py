"""fp64 restatement of a ConMamba encoder under every constructor argument, and the table of layer-configuration gates.

Helper of test_layer_config_gates_cpu.py / test_layer_config_gates_gpu.py; no tests in it.

``encoder`` restates ConmambaEncoder.forward from a state_dict on oracle.conmamba_oracle's pieces (mamba_inner_no_out_proj,
conv_module, ffn_module, _ln), with the mixer taking what the constructor takes: in_proj / out_proj bias, a missing conv bias,
if_devide_out, gamma (init_layer_scale), one direction (the causal layer, whose convolution module pads in front), any d_state,
d_conv, dt_rank, expand and kernel_size.  Which of these a layer has is read from the state_dict's keys and shapes; only
if_devide_out, kernel_size and causal leave no trace there and are arguments.  Everything is differentiable through torch autograd.

``CASES``: every entry is the smallest encoder on one side of one gate, every other argument at its default.  ``gate`` names the
condition by its predicate; the file:line beside it is a hint, as of the commit that added this table, ``flip`` the native launch whose presence in the INFERENCE
forward the gate decides, ``bf16`` / ``fp32`` whether it is present in that dtype.  They are derived from the conditions as written
in fused.py and modules/*_rows.py, not from a run.  ``train_kernels`` does the same for the backward launches of the autograd route.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import conmamba_oracle as O

DEFAULT_MAMBA = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}

# the project's bounds for an encoder output against the oracle (test_hip_modules.py::test_fused_frontend_and_encoder_match_unfused_and_oracle)
INFER_TOL = {torch.float32: dict(rtol=5e-3, atol=1e-3), torch.bfloat16: dict(rtol=3e-2, atol=5e-2)}


# ------------------------------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------------------------------
def mixer(p, hidden, prefix="", if_devide_out=True, work_dtype=torch.float64):
    """The layer's Mamba mixer, hidden (b, l, d) -> (b, l, d).  Two directions when the state_dict has ``A_b_log`` (bimamba.Mamba,
    v2), else one (UniMamba).  ``work_dtype`` None: the inner op in fp32 with fp32 A / D / dt bias, as oracle.bimamba_v2 leaves it
    (that is what agrees with the oracle to the last bit); torch.float64: everything in fp64."""
    has = lambda k: (prefix + k) in p
    hs = hidden
    w = lambda k: p[prefix + k].to(hs.dtype)
    small = (lambda t: t.to(work_dtype)) if work_dtype is not None else (lambda t: t.float())
    scan = O.selective_scan if work_dtype is None else functools.partial(O.selective_scan, work_dtype=work_dtype)
    b, l, d = hs.shape
    # (b, 2e, l), by the oracle's own expression: the fp32 inner op rounds xz, and another summation order would round it elsewhere
    xz = (w("in_proj.weight") @ hs.reshape(b * l, d).t()).reshape(-1, b, l).permute(1, 0, 2)
    if has("in_proj.bias"):
        xz = xz + w("in_proj.bias")[None, :, None]

    def direction(sfx, xz_):
        A = -torch.exp(small(p[prefix + ("A_b_log" if sfx else "A_log")]))
        return O.mamba_inner_no_out_proj(xz_, p[prefix + f"conv1d{sfx}.weight"],
                                         p[prefix + f"conv1d{sfx}.bias"] if has(f"conv1d{sfx}.bias") else None,
                                         p[prefix + f"x_proj{sfx}.weight"], p[prefix + f"dt_proj{sfx}.weight"], A,
                                         small(p[prefix + ("D_b" if sfx else "D")]), small(p[prefix + f"dt_proj{sfx}.bias"]),
                                         scan, work_dtype)

    mix = direction("", xz)
    if has("A_b_log"):
        bwd = direction("_b", xz.flip(-1)).flip(-1)
        mix = 0.5 * mix + 0.5 * bwd if if_devide_out else mix + bwd
    y = F.linear(mix.permute(0, 2, 1).to(hs.dtype), w("out_proj.weight"), w("out_proj.bias") if has("out_proj.bias") else None)
    return y * w("gamma") if has("gamma") else y


def conv_module(p, x, prefix="", kernel_size=31, causal=False):
    """ConvolutionModule.forward: O.conv_module for the 'same'-padded module; the causal one pads kernel_size - 1 rows in front
    (the module's pad-then-chomp)."""
    if not causal:
        return O.conv_module(p, x, prefix, kernel_size)
    g = lambda k: p[prefix + k].to(x.dtype)
    out = O._ln(x, g("layer_norm.weight"), g("layer_norm.bias"), 1e-5).transpose(1, 2)
    out = F.glu(F.conv1d(out, g("bottleneck.0.weight"), g("bottleneck.0.bias")), dim=1)
    out = F.conv1d(F.pad(out, (kernel_size - 1, 0)), g("conv.weight"), g("conv.bias"), groups=out.shape[1]).transpose(1, 2)
    out = F.gelu(O._ln(out, g("after_conv.0.weight"), g("after_conv.0.bias"), 1e-5))
    return F.linear(out, g("after_conv.2.weight"), g("after_conv.2.bias"))


def encoder_layer(p, x, prefix="", kernel_size=31, causal=False, if_devide_out=True, work_dtype=torch.float64):
    g = lambda k: p[prefix + k].to(x.dtype)
    x = x + 0.5 * O.ffn_module(p, x, prefix + "ffn_module1.")
    h = O._ln(x, g("norm1.norm.weight"), g("norm1.norm.bias"), 1e-5)
    x = mixer(p, h, prefix + "mamba.", if_devide_out, work_dtype) + x
    x = x + conv_module(p, x, prefix + "convolution_module.", kernel_size, causal)
    y = x + 0.5 * O.ffn_module(p, x, prefix + "ffn_module2.")
    return O._ln(y, g("norm2.norm.weight"), g("norm2.norm.bias"), 1e-5)


def encoder(p, x, num_layers, prefix="", kernel_size=31, causal=False, if_devide_out=True, work_dtype=torch.float64):
    for i in range(num_layers):
        x = encoder_layer(p, x, f"{prefix}layers.{i}.", kernel_size, causal, if_devide_out, work_dtype)
    return O._ln(x, p[prefix + "norm.norm.weight"].to(x.dtype), p[prefix + "norm.norm.bias"].to(x.dtype), 1e-6)


# ------------------------------------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    gate: str                               # the condition: predicate (file:line as a hint)
    flip: str                               # the native launch of the inference forward whose presence the gate decides
    bf16: bool                              # present in the bf16 inference forward
    fp32: bool                              # present in the fp32 inference forward
    d_model: int = 256
    d_ffn: int = 256
    layers: int = 2
    shape: Tuple[int, int] = (3, 37)        # 111 rows: no multiple of 16, 32 or 64, more than one 64-token tile
    kernel_size: int = 31
    causal: bool = False
    mamba: Dict = field(default_factory=dict)

    def mamba_config(self):
        return {**DEFAULT_MAMBA, **self.mamba}

    @property
    def d_inner(self):
        return int(self.mamba_config()["expand"] * self.d_model)

    @property
    def dt_rank(self):
        return self.mamba.get("dt_rank", math.ceil(self.d_model / 16))

    @property
    def supports(self):
        """fused.supports (fused.py:165-173) on this layer: the encoder's inference forward is fused.encoder_forward."""
        c = self.mamba_config()
        return self.kernel_size == 31 and c["d_state"] == 16 and c["d_conv"] == 4 and self.d_model % 4 == 0 and self.d_model <= 1024

    @property
    def if_devide_out(self):
        return self.mamba.get("if_devide_out", True)


BIG = dict(layers=1, shape=(2, 19), mamba={"expand": 1})       # d_model 1024 / 1032: one layer, 38 rows, E = d_model
OPTIONS = {"bias": {"bias": True}, "no_conv_bias": {"conv_bias": False}, "no_devide": {"if_devide_out": False},
           "layer_scale": {"init_layer_scale": 0.5}}
ALL_OPTIONS = {k: v for o in OPTIONS.values() for k, v in o.items()}

CASES: Dict[str, Case] = {
    # 1. expand.  E = expand * d_model.  cm_conv_xproj needs wx_packed: bf16, E % 32 == 0, E <= 2048 (fused.py:108); the fp32 forward
    # and E = 300 take cm_conv_cl_fwd.  expand 8: 2E = 4096 is the last width inside in_packed (fused.py:70, <= 4096) and
    # out_packed (fused.py:119-120, 2E % 128 == 0 and <= 8192).
    "expand1": Case("_LayerCache.wx_packed (fused.py:108) (E 256)", "cm_conv_xproj", True, False, mamba={"expand": 1}),
    "expand2": Case("_LayerCache.wx_packed (fused.py:108) (E 512, the default layer)", "cm_conv_xproj", True, False),
    "expand4": Case("_LayerCache.wx_packed (fused.py:108) (E 1024)", "cm_conv_xproj", True, False, mamba={"expand": 4}),
    "expand8": Case("_LayerCache.wx_packed (fused.py:108) E <= 2048; _LayerCache.in_packed (fused.py:70) 2E <= 4096; _LayerCache.out_packed (fused.py:119) 2E <= 8192 (all at their last value)",
                    "cm_conv_xproj", True, False, mamba={"expand": 8}),
    "expand8_dt_rank24": Case("ops.conv_xproj_supported: 64-wide rows stop at E 1248 (conv_xproj.hip:364) -> _LayerCache.wx_packed, mixer_rows._Derived.xr_packed", "cm_conv_xproj",
                              False, False, mamba={"expand": 8, "dt_rank": 24}),
    "expand4_dt_rank24": Case("ops.conv_xproj_supported: E 1024 <= 1248 with 64-wide rows", "cm_conv_xproj", True, False,
                              mamba={"expand": 4, "dt_rank": 24}),
    "expand1p5_d200": Case("_LayerCache.rows_mode (fused.py:100) E % 8 == 0; mixer_rows.py:39 (E 300: outside both)", "cm_conv_xproj", False, False,
                           d_model=200, mamba={"expand": 1.5}),
    # 2. dt_rank.  The fold (one E-wide scan output, out_proj at K = E) needs R <= 16 (fused.py:125); 17..32 keep rows_mode in bf16
    # only (fused.py:100) and so cm_conv_xproj; above 32 there is no rows mode and delta is a library GEMM (fused.py:244).
    "dt_rank5": Case("_LayerCache.rows_mode (fused.py:100) R <= 16", "cm_conv_xproj", True, False, mamba={"dt_rank": 5}),
    "dt_rank16": Case("_LayerCache.out_fold_packed (fused.py:125) R <= 16 (last value with the fold)", "cm_conv_xproj", True, False, mamba={"dt_rank": 16}),
    "dt_rank17": Case("_LayerCache.rows_mode (fused.py:100) 16 < R <= 32: bf16 only (64-wide rows)", "cm_conv_xproj", True, False, mamba={"dt_rank": 17}),
    "dt_rank24": Case("_LayerCache.rows_mode (fused.py:100) 16 < R <= 32: bf16 only", "cm_conv_xproj", True, False, mamba={"dt_rank": 24}),
    "dt_rank32": Case("_LayerCache.rows_mode (fused.py:100) R <= 32 (last value)", "cm_conv_xproj", True, False, mamba={"dt_rank": 32}),
    "dt_rank33": Case("_LayerCache.rows_mode (fused.py:100) R <= 32 (first value outside)", "cm_conv_xproj", False, False, mamba={"dt_rank": 33}),
    "dt_rank40": Case("_LayerCache.rows_mode (fused.py:100) R <= 32 (outside); _scan_dirs' library delta (fused.py:244)", "cm_conv_xproj", False, False, mamba={"dt_rank": 40}),
    # 3. d_model.  cm_ffn_fused streams d_model 256 and 144 only (fused.py:56, ops.py:2009); every other width takes layer_forward's
    # cm_add_layernorm seams, which the kernel serves up to 1024 columns (elementwise_cl.hip: cm_add_layernorm).  1032 is refused by
    # it: fused.supports (fused.py:172-173) mirrors that limit, and the 1032-wide encoder runs the module path.
    "d144": Case("_LayerCache.ffn_native: d144 (fused.py:55) (d_ffn 256)", "cm_ffn_fused", True, False, d_model=144),
    "d192": Case("_LayerCache.ffn_native: wide or d144 (fused.py:56)", "cm_ffn_fused", False, False, d_model=192),
    "d256": Case("_LayerCache.ffn_native: wide (fused.py:56)", "cm_ffn_fused", True, False),
    "d264": Case("_LayerCache.ffn_native: wide or d144 (fused.py:56) (a multiple of 8, not 256)", "cm_ffn_fused", False, False, d_model=264),
    "d1024": Case("ops.add_layernorm dim <= 1024; ffn_rows.py:45, convmod_rows.py:31, mixer_rows.py:256 d <= 1024 (last value)",
                  "cm_add_layernorm", True, True, d_model=1024, **BIG),
    "d1032": Case("fused.supports (fused.py:173) d_model <= 1024 = cm_add_layernorm's limit (first value outside)", "cm_add_layernorm", False, False,
                  d_model=1032, **BIG),
    # 4. d_ffn at d_model 256.  ops.ffn_supported: hidden >= 256 and % 256 == 0 (ops.py:2009).  Training: ffn_rows.supported f % 8 == 0 and
    # f <= 2048 (ffn_rows.py:45), _fused_ok F <= 2048 (ffn_rows.py:36).
    "ffn256": Case("ops.ffn_supported (ops.py:2009) hidden % 256 == 0 (smallest)", "cm_ffn_fused", True, False),
    "ffn264": Case("ops.ffn_supported (ops.py:2009) hidden % 256 == 0 (outside)", "cm_ffn_fused", False, False, d_ffn=264),
    "ffn2048": Case("ffn_rows.py:36/45 F <= 2048 (last value)", "cm_ffn_fused", True, False, d_ffn=2048),
    "ffn2304": Case("ops.ffn_supported (ops.py:2009) hidden <= 2048 = cm_ffn_fused's limit (first multiple of 256 outside)", "cm_ffn_fused", False, False,
                    d_ffn=2304),
    "ffn2056": Case("ffn_rows.py:45 f <= 2048 (outside); ops.py:2009", "cm_ffn_fused", False, False, d_ffn=2056),
    # 5. kernel_size.  fused.supports needs 31 (fused.py:172); convmod_rows and the native depthwise conv take <= 32
    # (convmod_rows.py:31, Conmamba.py:56).  An even kernel_size cannot be evaluated on the non-causal module at all: 'same' padding
    # (k - 1) // 2 on both sides gives T - 1 rows and the residual add fails, so 32 runs on the causal layer only.
    "k31": Case("fused.supports (fused.py:172) kernel_size == 31", "cm_glu_dwconv_ln_gelu", True, True),
    "k15": Case("fused.supports (fused.py:172) kernel_size == 31 (outside: module path)", "cm_glu_dwconv_ln_gelu", False, False, kernel_size=15),
    "k32_causal": Case("convmod_rows.py:31 kernel_size <= 32 (last value; causal: the non-causal module cannot add T - 1 rows to T)",
                       "cm_dwconv_cl_fwd", True, True, kernel_size=32, causal=True),
    "k33": Case("convmod_rows.py:31, Conmamba.py:56 kernel_size <= 32 (outside)", "cm_dwconv_cl_fwd", False, False, kernel_size=33),
    # 6. d_state, d_conv: outside fused.supports (fused.py:173) and mixer_rows.supported (mixer_rows.py:39)
    "d_state8": Case("fused.supports (fused.py:173) d_state == 16; mixer_rows.py:39", "cm_scan_cl_fwd", False, False, mamba={"d_state": 8}),
    "d_conv3": Case("fused.supports (fused.py:173) d_conv == 4; mixer_rows.py:39", "cm_scan_cl_fwd", False, False, mamba={"d_conv": 3}),
    # 7. options.  in_packed needs no in_proj bias (fused.py:70); out_packed no out_proj bias and no gamma (fused.py:120).  The launch names
    # stay what they are (the projection rides inside cm_ffn_fused / cm_ln_pw_glu), so ``flip`` names the kernel that carries it and the
    # GPU test counts library GEMMs: see ``library_gemms``.
    "opt_bias": Case("_LayerCache.in_packed (fused.py:70) in_proj.bias is None; _LayerCache.out_packed (fused.py:120) out_bias is None", "cm_ln_pw_glu", True, False,
                     mamba=OPTIONS["bias"]),
    "opt_no_conv_bias": Case("_LayerCache.dirs conv_b None (fused.py:89) -> cm_conv_xproj bias_f NULL (conv_xproj.hip:190); mixer_rows.py:41", "cm_conv_xproj", True, False,
                             mamba=OPTIONS["no_conv_bias"]),
    "opt_no_devide": Case("_LayerCache half = 1.0 (fused.py:81)", "cm_ln_pw_glu", True, False, mamba=OPTIONS["no_devide"]),
    "opt_layer_scale": Case("_LayerCache.out_packed (fused.py:120) gamma is None; mixer_rows.py:40", "cm_ln_pw_glu", True, False, mamba=OPTIONS["layer_scale"]),
    "opt_all": Case("_LayerCache.in_packed, half, conv_b, out_packed together (fused.py:70, 81, 89, 120)", "cm_ln_pw_glu", True, False, mamba=ALL_OPTIONS),
    # 8. the causal layer (UniMamba, front-padded convolution module): cm_conv_xproj_uni under the same wx_packed / rows_mode conditions
    "causal_expand1": Case("fused._conv, uni + wx_packed (fused.py:295) (E 256)", "cm_conv_xproj_uni", True, False, causal=True, mamba={"expand": 1}),
    "causal_expand4": Case("fused._conv, uni + wx_packed (fused.py:295) (E 1024)", "cm_conv_xproj_uni", True, False, causal=True, mamba={"expand": 4}),
    "causal_dt_rank5": Case("_LayerCache.rows_mode (fused.py:100) R <= 16, uni", "cm_conv_xproj_uni", True, False, causal=True, mamba={"dt_rank": 5}),
    "causal_dt_rank24": Case("_LayerCache.rows_mode (fused.py:100) 16 < R <= 32 bf16 only, uni", "cm_conv_xproj_uni", True, False, causal=True, mamba={"dt_rank": 24}),
    "causal_dt_rank40": Case("_LayerCache.rows_mode (fused.py:100) R <= 32 (outside), uni", "cm_conv_xproj_uni", False, False, causal=True, mamba={"dt_rank": 40}),
}


def library_gemms(case: Case, dtype) -> Optional[int]:
    """Library GEMMs (aten mm / addmm / _addmm_activation / bmm) of one layer of fused.encoder_forward(streams=1) on the all-native
    bf16 route, from the gates: None where the layer is not on that route (fp32, d_model other than 256 / 144, d_ffn off the
    256 grid, layers outside fused.supports).  in_proj: 0 inside cm_ffn_fused (in_packed: 2E % 256 (64 at d_model 144) == 0, 2E <= 4096,
    no bias), else 1.  x_proj: 0 inside cm_conv_xproj (rows_mode, E % 32 == 0, E <= 2048, and E <= 1248 for both directions' 64-wide rows), else 1, plus 1 for delta when dt_rank > 16
    without rows_mode.  out_proj: 0 inside cm_ln_pw_glu_mix (d_model 256, K % 128 == 0, K <= 8192, no bias, no gamma), else 1.  The
    convolution module's closing Linear: 0 inside cm_glu_dwconv_ln_gelu at d_model 256, else 1."""
    c = case.mamba_config()
    if dtype != torch.bfloat16 or not case.supports or case.d_model not in (256, 144) or case.d_ffn % 256 or not 256 <= case.d_ffn <= 2048:
        return None
    E, R, wide = case.d_inner, case.dt_rank, case.d_model == 256
    ndir = 1 if case.causal else 2
    rows_mode = R <= 32 and E % 8 == 0
    n = 0
    n += not ((2 * E) % (256 if wide else 64) == 0 and 2 * E <= 4096 and not c.get("bias", False))
    if not (rows_mode and E % 32 == 0 and E <= 2048 and (R <= 16 or ndir == 1 or E <= 1248)):
        n += 1 + (ndir if R > 16 and not rows_mode else 0)
    K = ndir * E
    n += not (wide and K % 128 == 0 and K <= 8192 and not c.get("bias", False) and c.get("init_layer_scale") is None)
    n += not wide
    return n


BWD_KERNELS = ("cm_ffn_bwd_fused", "cm_wgrad_bf16", "cm_scan_cl_bwd", "cm_conv_cl_bwd", "cm_dwconv_cl_bwd")


def train_kernels(case: Case, dtype) -> Dict[str, bool]:
    """Which of BWD_KERNELS the backward of the autograd route (eval mode, grad enabled; bf16 = autocast) launches, from the gates:
      cm_scan_cl_bwd, cm_conv_cl_bwd  the mixer is MixerRowsFn: mixer_rows.supported (mixer_rows.py:39-41)
      cm_dwconv_cl_bwd                convmod_rows.supported (convmod_rows.py:30-32), or the module's own native depthwise conv
                                      (Conmamba.py:56: kernel_size <= 32)
      cm_ffn_bwd_fused                ffn_rows._fused_ok (ffn_rows.py:36): bf16, d_model 256, d_ffn % 256 == 0, <= 2048 -- inside
                                      ffn_rows.supported (ffn_rows.py:45)
      cm_wgrad_bf16                   ops.wgrad: bf16 operands and a weight whose two sides are multiples of 128, 4096 at the most
                                      (cm_wgrad_supported).  The weights that go through it: the feed-forward node's (d_model, d_ffn) pair,
                                      the convolution-module node's (d_model, d_model) and (2 d_model, d_model), the mixer node's
                                      (d_model, ndir E) and (2E, d_model).  Never in fp32; in bf16 when any node that runs has such a weight."""
    c = case.mamba_config()
    bf = dtype == torch.bfloat16
    E, R, D, Fh = case.d_inner, case.dt_rank, case.d_model, case.d_ffn
    ndir = 1 if case.causal else 2
    mix = (c["d_state"] == 16 and c["d_conv"] == 4 and E % 8 == 0 and not c.get("bias", False) and c.get("init_layer_scale") is None
           and (R <= 16 or (R <= 32 and bf)) and c.get("conv_bias", True))
    ffn_rows = D % 8 == 0 and Fh % 8 == 0 and Fh <= 2048 and D <= 1024
    ffn_fused = ffn_rows and bf and D == 256 and Fh % 256 == 0 and Fh >= 256
    convmod = case.kernel_size <= 32 and D % 8 == 0 and D <= 1024
    side = lambda n: n % 128 == 0 and n <= 4096
    wgrad = bf and side(D) and ((ffn_rows and side(Fh)) or convmod or (mix and (side(ndir * E) or side(2 * E))))
    return {"cm_scan_cl_bwd": mix, "cm_conv_cl_bwd": mix, "cm_dwconv_cl_bwd": case.kernel_size <= 32,
            "cm_ffn_bwd_fused": ffn_fused, "cm_wgrad_bf16": wgrad}


# ------------------------------------------------------------------------------------------------------------------------
# building a case
# ------------------------------------------------------------------------------------------------------------------------
# dt_proj's weight is drawn N(0, DT_STD^2 / dt_rank): with the constructor's draw (std dt_rank^-0.5 against a bias of -7 .. -2) the
# low-rank dt features move delta by a few percent and a kernel that dropped some of them would pass; this draw is the one the CPU
# file's sensitivity test holds to its 25 % cap
DT_STD = 4.0
DT_HIGH_GAIN = 4.0      # x_proj's dt rows past the 16th (dt_rank 17: one row) weigh as much as the first sixteen together
OUT_GAIN = 2.0          # out_proj over its xavier draw: the mixer's share of the residual stream is what every option case changes


def build(case: Case, seed: int = 0):
    """-> (encoder on the CPU in eval mode, input (batch, frames, d_model) fp32), everything drawn from one seeded CPU generator:
    weight matrices xavier-normal as the module tests draw them (A_log keeps its S4D init), the mixer's biases N(0, 0.5), gamma
    0.5 * (1 + 0.3 randn), LayerNorm weights and biases perturbed by 10 %."""
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2000 + seed)                          # the constructors' own draws (dt_proj bias, uniform inits)
        enc = ConmambaEncoder(num_layers=case.layers, d_model=case.d_model, d_ffn=case.d_ffn, kernel_size=case.kernel_size,
                              activation=nn.GELU, bias=True, dropout=0.0, causal=case.causal, mamba_config=case.mamba_config()).eval()
    rn = lambda t, std=1.0: torch.randn(t.shape, generator=g) * std
    with torch.no_grad():
        for name, p in enc.named_parameters():
            leaf = name.split(".")[-1]
            if "A_log" in name or "A_b_log" in name:
                continue
            if isinstance(_owner(enc, name), nn.LayerNorm):
                p.copy_((1.0 + 0.1 * rn(p)) if leaf == "weight" else 0.1 * rn(p))
            elif leaf == "gamma":
                p.copy_(0.5 * (1.0 + 0.3 * rn(p)))
            elif ".mamba." in name and leaf == "bias" and "dt_proj" not in name:
                p.copy_(rn(p, 0.5))                             # in_proj / out_proj / conv1d / conv1d_b
            elif "dt_proj" in name and leaf == "weight":
                p.copy_(rn(p, DT_STD * p.shape[1] ** -0.5))     # every dt column moves delta: see DT_STD
            elif p.dim() == 2 or (p.dim() == 3 and p.shape[1] > 1):
                p.copy_(rn(p, math.sqrt(2.0 / (p.shape[0] + p.shape[1]))))      # Linear and pointwise conv; depthwise taps keep their init
                if ".mamba.out_proj" in name:
                    p.mul_(OUT_GAIN)
                if ".mamba.x_proj" in name:
                    p[16:p.shape[0] - 2 * case.mamba_config()["d_state"]].mul_(DT_HIGH_GAIN)     # the dt rows past the 16th, if any
    b, t = case.shape
    return enc, torch.randn(b, t, case.d_model, generator=g)


def _owner(root, name):
    m = root
    for part in name.split(".")[:-1]:
        m = getattr(m, part)
    return m


def params64(enc, requires_grad=False):
    return {k: v.detach().cpu().double().requires_grad_(requires_grad and v.is_floating_point()) for k, v in enc.state_dict().items()}


def reference(case: Case, p, x, work_dtype=torch.float64):
    """The fp64 encoder output of ``case`` from the state_dict ``p`` (fp64 tensors) and the input x."""
    return encoder(p, x.double(), case.layers, "", case.kernel_size, case.causal, case.if_devide_out, work_dtype)
