"""Fused MI355X forward of the ConMamba encoder (inference / no-grad path).

Same numbers as ConmambaEncoder.forward (reference modules/Conmamba.py:631-650, :716-727 and
modules/mamba/bimamba.py:192-253), but laid out for the hardware instead of mirroring the reference's op
sequence:
  * activations stay channels-last (rows = batch*time, channel axis contiguous) end to end: no transposes,
    no .flip() copies, no .contiguous() round trips;
  * the residual stream is fp32 (as under the reference's bf16 autocast, where LayerNorm outputs fp32), every
    GEMM operand is the compute dtype, and each residual-add + LayerNorm seam is ONE kernel (cm_add_layernorm);
  * both BiMamba directions share one conv launch (cm_conv_cl_fwd) and one scan launch (cm_scan_cl_fwd); the
    0.5*(fwd+bwd) average is folded into out_proj by K-concatenation: [y_f | y_b] @ (0.5*[W_out | W_out])^T;
  * GLU -> depthwise conv k=31 -> LayerNorm -> GELU of the convolution module is one kernel.
The causal layer (UniMamba mixer, front-padded depthwise conv) takes the same sequence with one scan direction
(cm_conv_xproj_uni, cm_glu_dwconv_ln_gelu_causal); those kernels and the scan carry state from one chunk of frames to the next,
which is how forward_streaming (at the end of this file) streams a causal encoder.

A layer's launches are written down once, in three pieces cut where the routes differ -- in front of the selective scan
and behind it:
  _head  FFN1 + norm1 + in_proj (cm_ffn_fused), both causal convs + x_proj (cm_conv_xproj)       rows of whole utterances
  _scan  cm_scan_cl_fwd, both directions                                                          any batch of utterances
  _tail  out_proj + LN + pointwise conv + GLU (cm_ln_pw_glu), cm_glu_dwconv_ln_gelu (+ Linear),
         FFN2 + norm2 (+ the encoder's final norm) (cm_ffn_fused)                                 rows of whole utterances
_encoder_forward_joined composes them for one part (head, scan, tail on the whole batch) or several (head per part on
its own stream, one scan, tail per part).  Each piece falls back to the library GEMM / seam kernel where a switch is off or
a kernel does not cover the layer; layer_forward (library feed-forward GEMMs) and layer_forward_native (cm_gemm_bf16) are
different sequences around the same conv + scan block.  Those GEMMs go to the vendor library through torch
(hipBLASLt/rocBLAS): plain library GEMMs, not the product.
"""
from __future__ import annotations

import os
from typing import Optional

import torch
import torch.nn.functional as F

from . import ops, weight_cache


class _LayerCache:
    """Per-layer GEMM weights in the compute dtype and small fp32 vectors, rebuilt when parameters change."""

    def __init__(self, layer, dtype):
        self.dtype = dtype
        c = lambda t: t.detach().to(dtype).contiguous()
        f = lambda t: None if t is None else t.detach().float().contiguous()
        ffn = lambda m: dict(ln=(f(m[0].weight), f(m[0].bias), m[0].eps), w1=c(m[1].ffn[0].weight), b1=c(m[1].ffn[0].bias),
                             w2=c(m[1].ffn[3].weight), b2=c(m[1].ffn[3].bias), b1f=f(m[1].ffn[0].bias),
                             b2f=f(m[1].ffn[3].bias))
        self.ffn1, self.ffn2 = ffn(layer.ffn_module1), ffn(layer.ffn_module2)
        D = self.ffn1["w1"].shape[1]
        # d_model 144 (csrc/fused_d144.hip): images padded to 160 columns / rows, 16x16x32 kernels only; CM_FUSED_D144=0 builds none
        wide = D == 256
        kp = ops._kpad(D)
        d144 = D == 144 and USE_FUSED_D144 and ops.FFN_LAYOUT == 16
        if ops.ffn_supported(D, self.ffn1["w1"].shape[0], dtype) and self.ffn1["w1"].is_cuda and (wide or d144):
            for q in (self.ffn1, self.ffn2):                       # cm_ffn_fused's fragment-tiled weight images
                q["w1p"] = ops.PackedWeight(q["w1"], ops.FFN_LAYOUT, pad=(q["w1"].shape[0], kp))
                q["w2p"] = ops.PackedWeight(q["w2"], ops.FFN_LAYOUT, pad=(kp, q["w2"].shape[1]))
                # the 32 x 16 tile image for small launches (32-token workgroups exist on the 32x32x16 kernel only)
                if ops.SMALL_FFN_ROWS > 0 and wide:
                    q["w1s"], q["w2s"] = (q["w1p"], q["w2p"]) if ops.FFN_LAYOUT == 32 else (ops.PackedWeight(q["w1"], 32), ops.PackedWeight(q["w2"], 32))
        self.norm1 = (f(layer.norm1.norm.weight), f(layer.norm1.norm.bias), layer.norm1.norm.eps)
        self.norm2 = (f(layer.norm2.norm.weight), f(layer.norm2.norm.bias), layer.norm2.norm.eps)
        m = layer.mamba
        self.d_inner, self.dt_rank, self.d_state = m.d_inner, m.dt_rank, m.d_state
        self.in_proj = c(m.in_proj.weight)
        self.in_packed = None                                     # in_proj inside cm_ffn_fused (bf16, d_model 256 / 144, no bias)
        if (USE_FFN_INPROJ and dtype == torch.bfloat16 and self.in_proj.is_cuda and self.in_proj.shape[1] == D and (wide or d144)
                and self.in_proj.shape[0] % (256 if wide else 64) == 0 and self.in_proj.shape[0] <= 4096 and m.in_proj.bias is None):
            # streamed by cm_ffn_fused's projection epilogue only
            self.in_packed = ops.PackedWeight(self.in_proj, ops.FFN_LAYOUT, pad=(self.in_proj.shape[0], kp))
            if ops.SMALL_FFN_ROWS > 0 and wide:
                self.in_packed_s = self.in_packed if ops.FFN_LAYOUT == 32 else ops.PackedWeight(self.in_proj, 32)
        self.in_bias = None if m.in_proj.bias is None else c(m.in_proj.bias)
        self.uni = not hasattr(m, "conv1d_b")                     # UniMamba (the causal layer): one direction, nothing to average
        sfxs = ("",) if self.uni else ("", "_b")
        if self.uni:
            self.out_cat = c(m.out_proj.weight)                                                    # (D, E)
        else:
            half = 0.5 if m.if_devide_out else 1.0
            self.out_cat = c(torch.cat([m.out_proj.weight, m.out_proj.weight], dim=1) * half)      # (D, 2E)
        self.out_bias = None if m.out_proj.bias is None else c(m.out_proj.bias)
        self.gamma = None if getattr(m, "init_layer_scale", None) is None else f(m.gamma)
        self.dirs = []
        for sfx in sfxs:
            conv, xp, dtp = getattr(m, "conv1d" + sfx), getattr(m, "x_proj" + sfx), getattr(m, "dt_proj" + sfx)
            A_log = getattr(m, "A_b_log" if sfx else "A_log")
            self.dirs.append(dict(conv_w=f(conv.weight).reshape(m.d_inner, -1), conv_b=f(conv.bias), x_proj=c(xp.weight),
                                  dt_proj=c(dtp.weight), dt_proj_f32=c(dtp.weight).float().contiguous(), dt_bias=f(dtp.bias), A=(-torch.exp(A_log.detach().float())).contiguous(),
                                  D=f(getattr(m, "D_b" if sfx else "D"))))
        cm = layer.convolution_module
        # both directions' x_proj as ONE GEMM over [u_fwd | u_bwd]: block-diagonal (2*(R+2N), 2E) weight
        xps = [getattr(m, "x_proj" + sfx) for sfx in sfxs]
        self.x_proj_bd = torch.block_diag(*[xp.weight.detach().to(dtype) for xp in xps])
        # row-major variant for cm_scan_cl_fwd's xdbl mode: output columns per direction are
        # [dt (zero padded to 16, or to 32 in bf16 when 16 < dt_rank <= 32) | B (16) | C (16)], so the scan reads the
        # GEMM's rows as written
        R, N = self.dt_rank, self.d_state
        self.rows_mode = (R <= 16 or (R <= 32 and dtype == torch.bfloat16)) and N == 16 and m.d_inner % 8 == 0
        if self.rows_mode:
            pad = ops.rows_dt_pad(R)
            self.row_width = pad + 32
            rows = [ops.xproj_rows(xp.weight, R, pad, dtype) for xp in xps]
            self.x_proj_rows = torch.block_diag(*rows)            # (2 RW, 2 E)
            # per-direction (RW, E) images for cm_conv_xproj (conv + x_proj in one kernel, bf16)
            self.wx_packed = None
            if dtype == torch.bfloat16 and ops.conv_xproj_supported(m.d_inner, pad, m.d_conv, len(sfxs)) and rows[0].is_cuda:
                self.wx_packed = [ops.PackedWeight(r) for r in rows]
            for d_, dtp in zip(self.dirs, [getattr(m, "dt_proj" + sfx) for sfx in sfxs]):
                d_["dt_w16"] = ops.pad_dt_weight(dtp.weight.detach().to(dtype))      # dtype-rounded like the reference's GEMM operand
        self.cm_ln = (f(cm.layer_norm.weight), f(cm.layer_norm.bias), cm.layer_norm.eps)
        self.pw_w, self.pw_b = c(cm.bottleneck[0].weight.squeeze(-1)), c(cm.bottleneck[0].bias)
        self.pw_bf, self.lin_bf = f(cm.bottleneck[0].bias), f(cm.after_conv[2].bias)
        self.pw_packed = None                                     # cm_ln_pw_glu's fragment-tiled pointwise-conv weight
        if dtype == torch.bfloat16 and self.pw_w.is_cuda and tuple(self.pw_w.shape) == (2 * D, D) and (wide or d144) and self.pw_bf is not None:
            self.pw_packed = ops.PackedWeight(self.pw_w, pad=(2 * D, kp))
        self.out_packed = None                                    # out_proj inside cm_ln_pw_glu (mixer_tail): no bias, no layer scale
        if (self.pw_packed is not None and self.out_cat.is_cuda and self.out_cat.shape[0] == 256 and self.out_cat.shape[1] % 128 == 0
                and self.out_cat.shape[1] <= 8192 and self.out_bias is None and self.gamma is None):
            self.out_packed = ops.PackedWeight(self.out_cat)
        # the same projection for the folded scan output (ycat = the gated sum of both directions, E wide): half * out_proj.weight,
        # (256, E); if_devide_out's 0.5 is a power of two, so the scaling is exact
        self.out_fold_packed = None
        if self.out_packed is not None and not self.uni and self.rows_mode and R <= 16 and dtype == torch.bfloat16:
            self.out_fold_packed = ops.PackedWeight(c(m.out_proj.weight * half))
        self.in_bias_f = None if m.in_proj.bias is None else f(m.in_proj.bias)
        self.out_bias_f = None if m.out_proj.bias is None else f(m.out_proj.bias)
        self.dw_w, self.dw_b = f(cm.conv.weight), f(cm.conv.bias)
        self.dw_wt = self.dw_w.reshape(self.dw_w.shape[0], -1).t().contiguous()              # (k, D) taps, coalesced reads
        self.cm_ln2 = (f(cm.after_conv[0].weight), f(cm.after_conv[0].bias), cm.after_conv[0].eps)
        self.lin_w, self.lin_b = c(cm.after_conv[2].weight), c(cm.after_conv[2].bias)
        self.lin_packed = None                                    # the same Linear inside cm_glu_dwconv_ln_gelu (bf16, d_model 256)
        if USE_DWCONV_LIN and dtype == torch.bfloat16 and self.lin_w.is_cuda and tuple(self.lin_w.shape) == (256, 256) and self.lin_bf is not None:
            self.lin_packed = ops.PackedWeight(self.lin_w)
        self.kernel_size, self.causal = cm.kernel_size, bool(cm.causal)

    @property
    def ffn_native(self) -> bool:
        """Both feed-forward modules run on cm_ffn_fused (bf16, d_model 256, or 144 with CM_FUSED_D144 on; one hidden width)."""
        return "w1p" in self.ffn1 and self.ffn2["w1"].shape[0] == self.ffn1["w1"].shape[0]     # the images exist: __init__ decided

    @property
    def all_native(self) -> bool:
        """The all-native bf16 route covers the layer: six launches and, with every switch on, no library GEMM."""
        return (self.ffn_native and self.rows_mode and self.wx_packed is not None and self.pw_packed is not None
                and self.in_bias is None and self.out_bias is None and self.gamma is None)


def _params_key(dtype, *modules):
    # (version, storage) per parameter: see ops.cast_cached / weight_cache.invalidate_caches
    return (dtype,) + tuple((p._version, p.data_ptr()) for m in modules for p in m.parameters())


# inference bundles: no captured training graph reads them
_LAYER = weight_cache.Kind("_cm_fused_cache", graphs_read=False, build=_LayerCache)


def _cache(layer, dtype) -> _LayerCache:
    return _LAYER.lookup(layer, _params_key(dtype, layer), dtype)


def supports(layer) -> bool:
    """The fused path covers the two layers the ASR recipes build: non-causal with the bidirectional (BiMamba v2) mixer, and causal
    (ConmambaEncoderLayer(causal=True)) with the unidirectional mixer and the front-padded convolution module."""
    from .modules.mamba.bimamba import Mamba as BiMamba, UniMamba
    cm = layer.convolution_module
    act_ok = isinstance(cm.after_conv[1], torch.nn.GELU) and isinstance(layer.ffn_module1[1].ffn[1], torch.nn.GELU)
    mixer_ok = isinstance(layer.mamba, UniMamba) if cm.causal else isinstance(layer.mamba, BiMamba)
    # every route off cm_ffn_fused (d_model 256 / 144) joins its stages with cm_add_layernorm: rows of whole float4s, 1024 columns at most
    d = layer.mamba.d_model
    return (mixer_ok and cm.kernel_size == 31 and cm.dilation == 1 and act_ok
            and layer.mamba.d_state == 16 and layer.mamba.d_conv == 4 and d % 4 == 0 and d <= 1024)


def _ffn(x, y_in, p, dtype):
    """y_in = LN(x) already computed (compute dtype) -> Linear -> GELU -> Linear (bias folded by addmm)."""
    if dtype == torch.bfloat16:
        # library epilogue (bias + GELU fused into the GEMM); its GELU differs from erf-GELU by < 1 bf16 ulp
        h = torch._addmm_activation(p["b1"], y_in, p["w1"].t(), use_gelu=True)
    else:
        h = F.gelu(torch.addmm(p["b1"], y_in, p["w1"].t()))
    return torch.addmm(p["b2"], h, p["w2"].t())


# cm_ffn_fused and cm_ln_pw_glu at d_model 144 (the ConMamba-small recipes; csrc/fused_d144.hip); CM_FUSED_D144=0 = no 144-wide images
# are built and those layers take layer_forward (library feed-forward GEMMs + cm_add_layernorm seams)
USE_FUSED_D144 = os.environ.get("CM_FUSED_D144", "1") == "1"


# BiMamba in_proj inside the first cm_ffn_fused of a layer; CM_FFN_INPROJ=0 = library GEMM after the kernel
USE_FFN_INPROJ = os.environ.get("CM_FFN_INPROJ", "1") == "1"


# the convolution module's closing Linear inside cm_glu_dwconv_ln_gelu; CM_DWCONV_LIN=0 = library GEMM after the kernel
USE_DWCONV_LIN = os.environ.get("CM_DWCONV_LIN", "1") == "1"


# cm_scan_cl_fwd's xdbl mode (row-group scan kernel, csrc/scan_rows_fwd.hip); CM_SCAN_ROWS=0 keeps the state-split kernel
USE_SCAN_ROWS = os.environ.get("CM_SCAN_ROWS", "1") == "1"


# cm_conv_xproj: conv (both directions) + x_proj GEMMs in one kernel (bf16); CM_CONV_XPROJ=0 = conv kernel + library GEMM
USE_CONV_XPROJ = os.environ.get("CM_CONV_XPROJ", "1") == "1"


# both directions' gated outputs summed by the scan into one E-wide tensor (cm_scan_cl_fwd_fold), out_proj at K = E in the mixer's
# tail; CM_SCAN_FOLD=0 = [y_fwd | y_bwd] and K = 2E
USE_SCAN_FOLD = os.environ.get("CM_SCAN_FOLD", "1") == "1"


def _layer_folds(c: _LayerCache) -> bool:
    """The layer's scan folds its directions: a function of the layer cache and the switches (the caller adds the chunk policy --
    time-chunked launches stay on the two-tensor route)."""
    return (USE_SCAN_FOLD and USE_SCAN_ROWS and USE_MIXER_TAIL and USE_LN_PW_GLU and c.out_fold_packed is not None
            and _conv_forms_xdbl(c))


def _scan_dirs(c: _LayerCache, ucat, ycat, batch, seqlen, xdbl=None, fold=False):
    """x_proj for both directions (one library GEMM, time-contiguous output rows), fp32 feature buffer, and the two
    direction descriptors of cm_scan_cl_fwd (one of each for the unidirectional mixer: ucat / ycat are E wide then).
    ``xdbl``: x_proj's rows when cm_conv_xproj has formed them already (only the row-group kernel reads them)."""
    E, R, N, nd = c.d_inner, c.dt_rank, c.d_state, len(c.dirs)
    rows, P = batch * seqlen, c.dt_rank + 2 * c.d_state
    if c.rows_mode and (USE_SCAN_ROWS or xdbl is not None):
        if xdbl is None:
            xdbl = (ucat.view(rows, nd * E) @ c.x_proj_rows.t()).view(batch, seqlen, nd * c.row_width)  # one library GEMM, rows as the scan reads them
        RW = c.row_width
        return [dict(u=ucat[:, :, i * E:(i + 1) * E], A=d["A"], D=d["D"], delta_bias=d["dt_bias"], dt_weight=d["dt_w16"],
                     xdbl=xdbl[:, :, RW * i:RW * (i + 1)], out=ycat if fold else ycat[:, :, i * E:(i + 1) * E], reverse=bool(i))
                for i, d in enumerate(c.dirs)]
    assert not fold
    xdblT = c.x_proj_bd @ ucat.view(rows, nd * E).t()                     # (2P, rows): [dt | B | C] fwd, then bwd
    feat = ops.alloc_bc(nd * P, batch, seqlen, ucat.device)
    feat.view(nd * P, rows).copy_(xdblT)                                  # one bf16 -> fp32 conversion
    dirs = []
    for i, d in enumerate(c.dirs):
        f = feat[i * P:(i + 1) * P]
        dd = dict(u=ucat[:, :, i * E:(i + 1) * E], A=d["A"], B=f[R:R + N], C=f[R + N:], D=d["D"],
                  delta_bias=d["dt_bias"], out=ycat[:, :, i * E:(i + 1) * E], reverse=bool(i))
        if R <= 16:                                                       # dt_proj folded into the scan kernel
            dd.update(dt_low=f[:R], dt_weight=d["dt_proj_f32"])
        else:
            dd["delta"] = (xdblT[i * P:i * P + R].t() @ d["dt_proj"].t()).view(batch, seqlen, E)   # (rows, E), pre-bias
        dirs.append(dd)
    return dirs


# the mixer's out_proj inside cm_ln_pw_glu (cm_ln_pw_glu_mix); CM_MIXER_TAIL=0 = library GEMM + cm_ln_pw_glu
USE_MIXER_TAIL = os.environ.get("CM_MIXER_TAIL", "1") == "1"


def _out_proj(c: _LayerCache, ycat):
    """Both directions' gated scan outputs (rows, 2E) -> mixer output (rows, D): 0.5*(y_f + y_b) @ W_out^T, one library GEMM."""
    y = ycat @ c.out_cat.t()
    if c.out_bias is not None:
        y = y + c.out_bias
    if c.gamma is not None:
        y = y * c.gamma.to(y.dtype)
    return y


def mixer_tail(c: _LayerCache, x, ycat):
    """The mixer's tail on the residual stream: x += out_proj(ycat); conv-module LN; pointwise conv; GLU.  x (rows, D) fp32, updated in
    place; ycat (rows, 2E) bf16 contiguous, or (rows, E): the folded scan output.  One kernel (cm_ln_pw_glu with the projection in front) when out_proj has neither bias nor
    layer scale, else the library GEMM and cm_ln_pw_glu.  Returns the gated (rows, D) bf16 tensor."""
    if ycat.shape[1] == c.d_inner and not c.uni:
        return ops.ln_pw_glu(x, None, 1.0, c.cm_ln, c.pw_packed, c.pw_bf, ycat=ycat, out_w=c.out_fold_packed)
    if USE_MIXER_TAIL and c.out_packed is not None:
        return ops.ln_pw_glu(x, None, 1.0, c.cm_ln, c.pw_packed, c.pw_bf, ycat=ycat, out_w=c.out_packed)
    return ops.ln_pw_glu(x, _out_proj(c, ycat), 1.0, c.cm_ln, c.pw_packed, c.pw_bf)


def _in_proj(c: _LayerCache, h, out=None):
    """h (rows, D) -> xz (rows, 2E) = [x | z], channels-last: one library GEMM (into ``out`` when given)."""
    xz = torch.mm(h, c.in_proj.t(), out=out)
    return xz if c.in_bias is None else xz.add_(c.in_bias)


def _conv_forms_xdbl(c: _LayerCache) -> bool:
    return USE_CONV_XPROJ and USE_SCAN_ROWS and c.rows_mode and c.wx_packed is not None and c.dtype == torch.bfloat16


def _conv(c: _LayerCache, xz, ucat, xdbl=None, xproj=True, hist=None, lens=None):
    """Both directions' causal conv + SiLU of xz's x half (batch, seqlen, 2E views) into ucat = [u_fwd | u_bwd].  With
    cm_conv_xproj the same kernel forms x_proj's rows (into ``xdbl`` when given) and they are returned, else None.
    The unidirectional mixer: one direction into ucat (E wide); ``hist`` = (x_hist, x_hist_out) of cm_conv_xproj_uni, the
    native streaming route's carry, ``lens`` its per-slot row counts (cm_conv_xproj_uni_slots).  ``lens`` with the bidirectional mixer:
    the utterances' own row counts (cm_conv_xproj_lens; the ragged whole-utterance route)."""
    E = c.d_inner
    if c.uni:
        w0 = (c.dirs[0]["conv_w"], c.dirs[0]["conv_b"])
        if xproj and _conv_forms_xdbl(c):
            x_hist, x_hist_out = hist or (None, None)
            return ops.conv_xproj_uni(xz[:, :, :E], *w0, c.wx_packed[0], out=ucat, xdbl=xdbl, x_hist=x_hist, x_hist_out=x_hist_out, lens=lens)
        assert hist is None and lens is None
        ops.conv_cl_fwd(xz[:, :, :E], *w0, silu=True, out_f=ucat)
        return None
    w = (c.dirs[0]["conv_w"], c.dirs[0]["conv_b"], c.dirs[1]["conv_w"], c.dirs[1]["conv_b"])
    if xproj and _conv_forms_xdbl(c):
        return ops.conv_xproj(xz[:, :, :E], *w, c.wx_packed[0], c.wx_packed[1], out_f=ucat[:, :, :E], out_b=ucat[:, :, E:], xdbl=xdbl, lens=lens)
    assert lens is None
    ops.conv_cl_fwd(xz[:, :, :E], *w, True, out_f=ucat[:, :, :E], out_b=ucat[:, :, E:])
    return None


def _scan(c: _LayerCache, xz, ucat, ycat, xdbl, batch, seqlen, state=None, lens=None, fold=False):
    """Both directions' selective scan of ucat, gated by xz's z half, into ycat (all (batch, seqlen, 2E)): one launch.
    ``fold``: ycat is (batch, seqlen, E) and receives the gated sum of both directions (cm_scan_cl_fwd_fold).
    ``state`` (batch, E, 16) fp32, streaming: the unidirectional scan starts from it and leaves its last state there (each workgroup
    reads its channels' entry state before it writes them), unchunked -- the recurrence then visits the same values in the same
    order as over the whole sequence.  ``lens`` (with ``state``): per-slot step counts (cm_scan_cl_fwd_slots).  ``lens`` without
    ``state``: the utterances' own step counts, every direction, unchunked (cm_scan_cl_fwd_lens; the ragged whole-utterance route)."""
    dirs = _scan_dirs(c, ucat, ycat, batch, seqlen, xdbl, fold)
    if state is None and lens is not None:
        ops.scan_cl_fwd(dirs, z=xz[:, :, c.d_inner:], delta_softplus=True, time_chunks=1, lens=lens, whole=True, fold=fold)
        return
    if state is None:
        ops.scan_cl_fwd(dirs, z=xz[:, :, c.d_inner:], delta_softplus=True, fold=fold)
        return
    assert not fold
    if len(dirs) != 1 or "xdbl" not in dirs[0]:
        raise NotImplementedError("streaming needs the row-group scan (dt_rank <= 16, or <= 32 in bf16) of a unidirectional mixer")
    ops.scan_cl_fwd([dict(dirs[0], h0=state, h_last=state)], z=xz[:, :, c.d_inner:], delta_softplus=True, time_chunks=1, lens=lens)


def bimamba_fused(c: _LayerCache, h, batch, seqlen):
    """h: LN'd input (rows, D) in the compute dtype -> mixer output (rows, D) (reference bimamba.py:192-253)."""
    xz = _in_proj(c, h).view(batch, seqlen, -1)
    ucat = torch.empty((batch, seqlen, len(c.dirs) * c.d_inner), dtype=xz.dtype, device=xz.device)
    ycat = torch.empty_like(ucat)
    _scan(c, xz, ucat, ycat, _conv(c, xz, ucat), batch, seqlen)
    return _out_proj(c, ycat.view(batch * seqlen, -1))


# cm_ffn_fused: the whole feed-forward module (LayerNorm, both Linears, GELU, scaled residual, the next LayerNorm) in
# one kernel with the hidden activations kept in LDS.  bf16 compute, d_model 256.  CM_FUSED_FFN=0 falls back to the
# library GEMMs + cm_add_layernorm seams.
USE_FUSED_FFN = os.environ.get("CM_FUSED_FFN", "1") == "1"


# cm_ln_pw_glu: residual add + LayerNorm + pointwise conv + GLU in one kernel; CM_LN_PW_GLU=0 = seam kernel + library GEMM
USE_LN_PW_GLU = os.environ.get("CM_LN_PW_GLU", "1") == "1"


def _ffn_call(x, f, **kw):
    """cm_ffn_fused on the residual rows x with the cached feed-forward module f (c.ffn1 / c.ffn2), at the layer's alpha = 0.5."""
    return ops.ffn_fused(x, f["ln"], f["w1p"], f["b1f"], f["w2p"], f["b2f"], alpha=0.5, **kw)


def _ffn_images(c: _LayerCache, small: bool):
    """(ffn1, ffn2, in_packed) as cm_ffn_fused streams them.  ``small``: a launch of at most CM_FFN_SMALL_ROWS rows leaves CUs
    idle at 64 tokens per workgroup, so it takes the 32 x 16 tile images (the 32-token form of the 32x32x16 kernel)."""
    if not (small and "w1s" in c.ffn1):
        return c.ffn1, c.ffn2, c.in_packed
    return (dict(c.ffn1, w1p=c.ffn1["w1s"], w2p=c.ffn1["w2s"]), dict(c.ffn2, w1p=c.ffn2["w1s"], w2p=c.ffn2["w2s"]),
            getattr(c, "in_packed_s", None))


def _head(c: _LayerCache, x, xz, ucat, xdbl=None, small=False, hist=None, lens=None):
    """A layer in front of the scan, on the rows of whole utterances: x (rows, D) fp32 += 0.5 ffn1(x); norm1; in_proj -> xz;
    both causal convs -> ucat; x_proj -> xdbl.  xz / ucat (batch, seqlen, 2E) and xdbl (batch, seqlen, 2 RW) or None are
    these rows' slices of the forward's buffers.  Returns x_proj's rows when cm_conv_xproj formed them, else None."""
    f1, _, inp = _ffn_images(c, small)
    if c.in_packed is not None:
        _ffn_call(x, f1, norm2=c.norm1, proj_w=inp, proj_out=xz.view(x.shape[0], -1))
    else:
        _in_proj(c, _ffn_call(x, f1, norm2=c.norm1)[1], out=xz.view(x.shape[0], -1))
    return _conv(c, xz, ucat, xdbl, hist=hist, lens=lens)


def _ffn2(c: _LayerCache, x, addend, final_ln=None, f2=None):
    """A layer's closing step: x = norm2(x + addend + 0.5 ffn2(x + addend)) in place, one kernel.  On the last layer the
    encoder's final norm rides along and its fp32 output rows are returned."""
    return _ffn_call(x, f2 or c.ffn2, addend=addend, norm1=c.norm2, norm2=final_ln, want_h=final_ln is not None,
                     h_dtype=torch.float32)[1]


def _tail(c: _LayerCache, x, ycat, batch, seqlen, final_ln=None, small=False, hist=None, lens=None):
    """A layer behind the scan, on the rows of whole utterances: x (rows, D) fp32 += out_proj(ycat (rows, 2E, or E folded)); the
    convolution module; FFN2 + norm2 (-> _ffn2).  ``hist`` = (hist, hist_out) of cm_glu_dwconv_ln_gelu_causal, the native
    streaming route's carry, ``lens`` its per-slot row counts (cm_glu_dwconv_ln_gelu_causal_slots).  ``lens`` without ``hist``: the
    utterances' own row counts under the 'same' padding (cm_glu_dwconv_ln_gelu_lens; the ragged whole-utterance route)."""
    D = x.shape[-1]
    dw = (c.dw_w, c.dw_b, c.cm_ln2[0], c.cm_ln2[1], c.cm_ln2[2])
    kw = dict(causal=True, hist=hist[0], hist_out=hist[1], lens=lens) if hist is not None else dict(causal=c.causal, lens=lens)
    if USE_LN_PW_GLU and c.pw_packed is not None:
        # x += mamba ; conv-module LN ; pointwise conv ; GLU -- one kernel, the 2D-wide tensor never exists
        gl = mixer_tail(c, x, ycat)
        g = ops.glu_dwconv_ln_gelu(gl.view(batch, seqlen, D), *dw, weight_t=c.dw_wt, glu_done=True, lin_w=c.lin_packed, lin_b=c.lin_bf, **kw)
    else:
        assert hist is None                                      # the carried rows are the gated ones
        _, h = ops.add_layernorm(x, _out_proj(c, ycat), 1.0, x_out=x, norm2=c.cm_ln, out_dtype=c.dtype)   # x += mamba ; conv-module LN
        pw = torch.addmm(c.pw_b, h, c.pw_w.t()).view(batch, seqlen, 2 * D)
        g = ops.glu_dwconv_ln_gelu(pw, *dw, weight_t=c.dw_wt, lin_w=c.lin_packed, lin_b=c.lin_bf, **kw)
    y = g.view(-1, D) if c.lin_packed is not None else torch.addmm(c.lin_b, g.view(-1, D), c.lin_w.t())
    return _ffn2(c, x, y, final_ln, _ffn_images(c, small)[1])


def layer_forward(layer, x, batch, seqlen, dtype, final_ln=None):
    """One ConmambaEncoderLayer with its feed-forward GEMMs in the library (fp32, or cm_ffn_fused off / not covering it), on
    the fp32 residual stream x (rows, D), in place.  Returns x, or the encoder's final norm of it under ``final_ln``."""
    c = _cache(layer, dtype)
    D = x.shape[-1]
    _, h = ops.add_layernorm(x, None, norm2=c.ffn1["ln"], out_dtype=dtype)                   # LN of ffn_module1
    y = _ffn(x, h, c.ffn1, dtype)
    _, h = ops.add_layernorm(x, y, 0.5, x_out=x, norm2=c.norm1, out_dtype=dtype)              # x += 0.5 ffn1 ; norm1
    y = bimamba_fused(c, h, batch, seqlen)
    _, h = ops.add_layernorm(x, y, 1.0, x_out=x, norm2=c.cm_ln, out_dtype=dtype)              # x += mamba ; conv-module LN
    pw = torch.addmm(c.pw_b, h, c.pw_w.t()).view(batch, seqlen, 2 * D)                       # pointwise conv D -> 2D
    g = ops.glu_dwconv_ln_gelu(pw, c.dw_w, c.dw_b, c.cm_ln2[0], c.cm_ln2[1], c.cm_ln2[2], weight_t=c.dw_wt, causal=c.causal)
    y = torch.addmm(c.lin_b, g.view(-1, D), c.lin_w.t())
    _, h = ops.add_layernorm(x, y, 1.0, x_out=x, norm2=c.ffn2["ln"], out_dtype=dtype)         # x += conv ; LN of ffn_module2
    y = _ffn(x, h, c.ffn2, dtype)
    ops.add_layernorm(x, y, 0.5, x_out=x, norm1=c.norm2, want_out=False)                      # x = norm2(x + 0.5 ffn2)
    if final_ln is None:
        return x
    return ops.add_layernorm(x, None, norm2=final_ln, out_dtype=torch.float32)[1]             # the encoder's final norm


# cm_gemm_bf16 (hand-written MFMA GEMM with fused bias/GELU/residual+LayerNorm epilogues) is correct but, in round 1,
# 2-3x slower than the vendor library on these shapes (profiles/r01/bench_ops_gemm.log): opt-in until it is tuned.
USE_NATIVE_GEMM = os.environ.get("CM_NATIVE_GEMM", "0") == "1"


def _native_gemms_ok(c: _LayerCache, D: int, dtype) -> bool:
    """cm_gemm_bf16 covers the layer when d_model == 256 (one workgroup owns whole residual rows) in bf16."""
    F_ = c.ffn1["w1"].shape[0]
    return (USE_NATIVE_GEMM and dtype == torch.bfloat16 and D == 256 and F_ % 256 == 0 and F_ % 64 == 0 and (2 * c.d_inner) % 256 == 0
            and c.gamma is None and not c.uni)


def layer_forward_native(layer, x, h, batch, seqlen, next_ln):
    """ConmambaEncoderLayer with every projection on cm_gemm_bf16: bias/GELU and all four residual + LayerNorm seams
    are GEMM epilogues.  x: fp32 residual (rows, 256), updated in place; h = LN_ffn1(x) in bf16.
    Returns the bf16 LayerNorm of the layer output under ``next_ln`` (next layer's first LN) or None."""
    c = _cache(layer, torch.bfloat16)
    D, E, rows = x.shape[-1], c.d_inner, batch * seqlen
    g = ops.gemm_bf16
    u1 = g(h, c.ffn1["w1"], c.ffn1["b1f"], epilogue=1)                                        # Linear + GELU
    h = g(u1, c.ffn1["w2"], c.ffn1["b2f"], epilogue=2, x=x, alpha=0.5, norm2=c.norm1)        # x += 0.5 ffn1 ; norm1
    xz = g(h, c.in_proj, c.in_bias_f, epilogue=0)                                            # (rows, 2E) = [x | z]
    xz = xz.view(batch, seqlen, 2 * E)
    ucat, ycat = torch.empty_like(xz), torch.empty_like(xz)
    _conv(c, xz, ucat, xproj=False)                                                          # conv kernel; x_proj in the library
    _scan(c, xz, ucat, ycat, None, batch, seqlen)
    h = g(ycat.view(rows, 2 * E), c.out_cat, c.out_bias_f, epilogue=2, x=x, alpha=1.0, norm2=c.cm_ln)   # x += mixer
    pw = g(h, c.pw_w, c.pw_bf, epilogue=0).view(batch, seqlen, 2 * D)
    gl = ops.glu_dwconv_ln_gelu(pw, c.dw_w, c.dw_b, c.cm_ln2[0], c.cm_ln2[1], c.cm_ln2[2], weight_t=c.dw_wt)
    h = g(gl.view(rows, D), c.lin_w, c.lin_bf, epilogue=2, x=x, alpha=1.0, norm2=c.ffn2["ln"])           # x += conv
    u2 = g(h, c.ffn2["w1"], c.ffn2["b1f"], epilogue=1)
    return g(u2, c.ffn2["w2"], c.ffn2["b2f"], epilogue=2, x=x, alpha=0.5, norm1=c.norm2, norm2=next_ln,
             want_out=next_ln is not None)                                                   # x = norm2(x + 0.5 ffn2)


# Utterances are independent through the whole encoder, so the batch can run as N parts on N HIP streams (captured into
# the hipGraph): kernels of different parts then overlap each other's launch tails and their load / compute / store
# phases.  Two modes (CM_STREAM_MODE):
#   "join" (default): every kernel but the selective scan runs per part on its own stream; the scan runs once per layer
#           on the whole batch between a join and a fork, so the dominant kernel keeps the chip to itself and its launch
#           duration is its own.  Measured over one stream at 64 utterances: 2 parts +2.5 %, 3 parts +3.5 %, 4 parts +6.5 %,
#           6 parts -4 %.
#   "free": the parts are fully independent.  +7.7-8.6 %, most of it from the VALU-bound scan running beside
#           memory-bound kernels of the other parts -- but every kernel's duration then includes the time it shares the
#           chip (the scan's measured roofline fraction halves), so it is not the default.
# CM_STREAMS=1 disables.
N_STREAMS = int(os.environ.get("CM_STREAMS", "2"))
STREAM_MODE = os.environ.get("CM_STREAM_MODE", "join")
_side_streams = {}


def _side_pool(dev, n):
    """``n`` side streams of the device's pool, which grows on demand."""
    pool = _side_streams.setdefault(dev.index, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=dev))
    return pool[:n]


def _final_norm(encoder):
    """The encoder's closing LayerNorm as the kernels take one: (weight, bias, eps), fp32."""
    ln = encoder.norm.norm
    return ln.weight.detach().float(), ln.bias.detach().float(), ln.eps


def _residual_rows(src):
    """src (batch, seqlen, D) -> the fp32 residual stream (rows, D), a private copy: the layers update it in place."""
    x = src.detach().float().reshape(-1, src.shape[-1]).contiguous()
    return x.clone() if x.data_ptr() == src.data_ptr() else x


def _ragged_native(caches, dtype) -> bool:
    """The ragged whole-utterance route runs on the kernels that take lengths: bf16, every layer bidirectional and all_native with
    cm_conv_xproj forming x_proj's rows (d_model 256, and 144 with its library GEMMs in the row-local places)."""
    return (USE_FUSED_FFN and USE_LN_PW_GLU and dtype == torch.bfloat16 and bool(caches)
            and all(c.all_native and _conv_forms_xdbl(c) and not c.uni and not c.causal and c.kernel_size == 31 for c in caches))


def _encoder_forward_joined(encoder, src, dtype, ns, paired=False, lens=None):
    """The encoder with both feed-forward modules on cm_ffn_fused, every layer as _head, _scan, _tail, the batch as ``ns``
    parts.  One part: the three pieces on the whole batch.  Several: the parts run on ``ns`` HIP streams for everything
    EXCEPT the selective scan, which runs once per layer on the whole batch between a join and a fork: the kernels whose
    load / compute / store phases run in lock step (FFN, seam, conv, GEMMs) overlap across parts, while the dominant kernel
    keeps the chip to itself (its launch duration is then its own, and its grid is the full batch).  Returns None when
    cm_ffn_fused does not cover a layer or, with several parts, a layer is not covered by the all-native bf16 path.

    ``paired`` (CM_STREAM_MODE=pair): the scan runs PER PART, and a part's scan waits for the end of the scan launched before
    it -- at most one scan is on the chip at any time, always beside the other parts' feed-forward / row kernels (VERDICT r2
    item 4: the vector-issue-bound scan leaves 80 % of HBM and the matrix pipe idle).

    ``lens`` (device int32 (batch,)): utterance b has lens[b] rows.  The three kernels of a layer that mix time take each
    part's slice of it, the joined scan the whole tensor, unchunked; None is returned unless _ragged_native holds."""
    batch, seqlen, D = src.shape
    caches = [_cache(layer, dtype) for layer in encoder.layers]
    if not (USE_FUSED_FFN and caches and all(c.ffn_native for c in caches)):
        return None
    if lens is not None and not _ragged_native(caches, dtype):
        return None
    if ns > 1 and not (USE_CONV_XPROJ and USE_SCAN_ROWS and USE_LN_PW_GLU and all(c.all_native and not c.uni for c in caches)):
        return None
    dev = src.device
    cur = torch.cuda.current_stream(dev)
    edges = [int(round(i * batch / ns)) for i in range(ns + 1)]
    parts = [(edges[i], edges[i + 1]) for i in range(ns) if edges[i + 1] > edges[i]]
    streams = [cur] + _side_pool(dev, len(parts) - 1)
    # CM_FFN_SMALL_ROWS is about the unsplit launch: parts share the chip with each other's kernels
    small = len(parts) == 1 and 0 < batch * seqlen <= ops.SMALL_FFN_ROWS
    fin = _final_norm(encoder)
    # lens is checked once per tensor a launch takes: the whole one (the joined scan) and each part's slice
    sl = None if lens is None else ops.slot_lens(lens, batch, dev, "encoder_forward")
    psl = [None if lens is None else (sl if (b0, b1) == (0, batch) else ops.slot_lens(lens[b0:b1], b1 - b0, dev, "encoder_forward"))
           for b0, b1 in parts]
    with torch.autocast("cuda", enabled=False):
        x = _residual_rows(src)
        nd = len(caches[0].dirs)
        xz = torch.empty((batch, seqlen, 2 * caches[0].d_inner), dtype=dtype, device=dev)
        ucat = torch.empty((batch, seqlen, nd * caches[0].d_inner), dtype=dtype, device=dev)
        # a layer folds both directions into an E-wide ycat unless its scan launches are time-chunked (small batches without lens)
        E = caches[0].d_inner
        unchunked = all(ops.scan_chunks_policy(nb, seqlen, E, nd, lens) == 1
                        for nb in ([b1 - b0 for b0, b1 in parts] if paired else [batch]))
        folds = [unchunked and _layer_folds(c) for c in caches]
        ycat = None if all(folds) else torch.empty_like(ucat)
        yfold = torch.empty((batch, seqlen, E), dtype=dtype, device=dev) if any(folds) else None
        xdbl = torch.empty((batch, seqlen, nd * caches[0].row_width), dtype=dtype, device=dev) if _conv_forms_xdbl(caches[0]) else None
        x3 = x.view(batch, seqlen, D)
        rows = lambda t, b0, b1: t[b0:b1].view((b1 - b0) * seqlen, -1)      # a part's utterances of a (batch, seqlen, .) buffer as rows
        outs = [None] * len(parts)

        def fork():
            for st in streams[1:]:
                st.wait_stream(cur)

        def join():
            for st in streams[1:]:
                cur.wait_stream(st)

        fork()
        gate = None                                                                 # pair mode: end of the scan launched last
        for li, c in enumerate(caches):
            fold = folds[li]
            yc = yfold if fold else ycat
            for st, (b0, b1), pl in zip(streams, parts, psl):
                with torch.cuda.stream(st):
                    _head(c, rows(x3, b0, b1), xz[b0:b1], ucat[b0:b1], None if xdbl is None else xdbl[b0:b1], small, lens=pl)
            if paired:
                for st, (b0, b1), pl in zip(streams, parts, psl):
                    with torch.cuda.stream(st):
                        if gate is not None:
                            st.wait_event(gate)
                        _scan(c, xz[b0:b1], ucat[b0:b1], yc[b0:b1], xdbl[b0:b1], b1 - b0, seqlen, lens=pl, fold=fold)
                        gate = torch.cuda.Event()
                        gate.record(st)
            else:
                join()
                _scan(c, xz, ucat, yc, xdbl, batch, seqlen, lens=sl, fold=fold)
                fork()
            for pi, (st, (b0, b1)) in enumerate(zip(streams, parts)):
                with torch.cuda.stream(st):
                    outs[pi] = _tail(c, rows(x3, b0, b1), rows(yc, b0, b1), b1 - b0, seqlen,
                                     fin if li == len(caches) - 1 else None, small, lens=psl[pi])
        join()
        for o in outs[1:]:
            o.record_stream(cur)
        return (outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)).view(batch, seqlen, D)


def _encoder_forward_ragged(encoder, src, dtype, streams, lens):
    """encoder_forward with per-utterance row counts: the joined native route with ``lens`` in its three time-mixing kernels, or each
    utterance alone on its own rows."""
    batch, seqlen, D = src.shape
    ops.slot_lens(lens, batch, src.device, "encoder_forward")
    ns = min(N_STREAMS, max(1, batch // 16)) if streams is None else streams
    if not (ns > 1 and batch >= 2 * 8):
        ns = 1
    caches = [_cache(layer, dtype) for layer in encoder.layers]
    if _ragged_native(caches, dtype):
        # several parts: the joined route, or the per-part scans of "pair"; "free" falls out of slicing -- independent parts are one part each
        if ns > 1 and STREAM_MODE not in ("join", "pair"):
            ns = 1
        out = _encoder_forward_joined(encoder, src, dtype, ns, paired=ns > 1 and STREAM_MODE == "pair", lens=lens)
        if out is not None:
            return out
    out = torch.zeros((batch, seqlen, D), dtype=torch.float32, device=src.device)
    for b, n in enumerate(lens.clamp(0, seqlen).tolist()):       # the one host read of the fallback
        if n > 0:
            out[b, :n] = encoder_forward(encoder, src[b:b + 1, :n], dtype, streams=1)[0]
    return out


@torch.no_grad()
def encoder_forward(encoder, src, dtype: Optional[torch.dtype] = None, streams: Optional[int] = None, lens=None):
    """ConmambaEncoder.forward (eval, no grad) through the fused path: src (B, T, D) -> (B, T, D) fp32.

    ``lens``: an int32 (B,) tensor on src's device, utterance b has lens[b] rows (clamped to [0, T] on the device).  Its
    output rows [0, lens[b]) are those of this function on src[b:b+1, :lens[b]] alone; rows at and past lens[b] are unspecified, and
    what src holds there (NaN included) reaches no valid row of any utterance.  On the native route (bf16, every layer bidirectional
    and all_native with cm_conv_xproj: d_model 256, and 144) the lengths are read on the device only, so a fixed (B, T) call can be
    captured in a hipGraph and replayed with other lengths; the selective scan is unchunked under ``lens``, as in the per-slot
    streaming route (bit-equal to a solo run whose scan is unchunked too: CM_SCAN_CHUNKS=1).  Any other configuration (fp32,
    CM_*=0 switches, other layers) reads ``lens`` on the host, encodes each utterance alone on its own rows and scatters the results:
    the same semantics, slowly.  ``lens=None`` is the call without lengths, launch for launch."""
    if dtype is None:
        dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
    if lens is not None:
        return _encoder_forward_ragged(encoder, src, dtype, streams, lens)
    # parts of at least 16 utterances (measured, join mode: 16 utterances 12.1 M frames/s as one part vs 10.6 M as four;
    # 32: 15.1 / 15.3 / 15.2 M with 1 / 2 / 4; 64: 16.6 / 17.0 / 17.7 M); an explicit ``streams`` argument is taken as is
    ns = min(N_STREAMS, max(1, src.shape[0] // 16)) if streams is None else streams
    if any(layer.convolution_module.causal for layer in encoder.layers):
        ns = 1                                                   # the multi-stream modes are built around the two-direction scan
    if ns > 1 and src.shape[0] >= 2 * 8:                       # split only batches large enough to keep each half busy
        if STREAM_MODE in ("join", "pair"):
            out = _encoder_forward_joined(encoder, src, dtype, ns, paired=STREAM_MODE == "pair")
            if out is not None:
                return out
        cur = torch.cuda.current_stream(src.device)            # "free", or a layer the joined route does not cover
        chunks = list(torch.chunk(src, ns, dim=0))
        pool = _side_pool(src.device, len(chunks) - 1)
        outs = [None] * len(chunks)
        for i in range(1, len(chunks)):
            pool[i - 1].wait_stream(cur)
            with torch.cuda.stream(pool[i - 1]):
                outs[i] = encoder_forward(encoder, chunks[i], dtype, streams=1)
        outs[0] = encoder_forward(encoder, chunks[0], dtype, streams=1)
        for i in range(1, len(chunks)):
            cur.wait_stream(pool[i - 1])
            outs[i].record_stream(cur)
        return torch.cat(outs, dim=0)
    batch, seqlen, D = src.shape
    caches = [_cache(layer, dtype) for layer in encoder.layers]
    n = len(caches)
    native = all(_native_gemms_ok(c, D, dtype) for c in caches)
    out = None if native else _encoder_forward_joined(encoder, src, dtype, 1)
    if out is not None:
        return out
    with torch.autocast("cuda", enabled=False):
        out = x = _residual_rows(src)
        fin = _final_norm(encoder)
        if native:
            _, h = ops.add_layernorm(x, None, norm2=caches[0].ffn1["ln"], out_dtype=dtype)      # first LN of layer 0
            for i, layer in enumerate(encoder.layers):
                h = layer_forward_native(layer, x, h, batch, seqlen, caches[i + 1].ffn1["ln"] if i + 1 < n else None)
            _, out = ops.add_layernorm(x, None, norm2=fin, out_dtype=torch.float32)             # encoder's final norm
        else:
            for i, layer in enumerate(encoder.layers):
                out = layer_forward(layer, x, batch, seqlen, dtype, final_ln=fin if i == n - 1 else None)
        return out.view(batch, seqlen, D)


# ------------------------------------------------------------------------------------------------
# streaming: the causal encoder one chunk of frames at a time (ConmambaEncoder.forward_streaming)
# ------------------------------------------------------------------------------------------------
# Per layer and stream the context carries what the three time-mixing steps have seen: the scan's state (E, 16) fp32, the last
# 3 inputs of the mixer's width-4 conv, the last 30 gated rows in front of the k = 31 depthwise conv.  Everything else is row-local.
# Native route (bf16, d_model 256, every layer all_native): a layer is the six launches of the whole-utterance route --
#   cm_ffn_fused (FFN1 + norm1 + in_proj), cm_conv_xproj_uni (reads / writes the conv rows), cm_scan_cl_fwd (h0 = h_last = the state),
#   cm_ln_pw_glu_mix, cm_glu_dwconv_ln_gelu_causal (+ Linear; reads / writes the gated rows), cm_ffn_fused (FFN2 + norm2 [+ final norm])
# -- no library GEMM, no copy of history rows.  The two row histories are double-buffered (a launch may not write the rows its
# other workgroups still read) and swapped after each layer.  CM_STREAM_NATIVE=0 = the generic route for A/B runs.
# Generic route (fp32, other widths): layer_forward's sequence, the history rows prepended in torch and their outputs dropped.
USE_STREAM_NATIVE = os.environ.get("CM_STREAM_NATIVE", "1") == "1"


def _rows_behind(rows, first, n):
    """rows (B, R, W), first (B,) int64 -> (B, n, W): rows [first[b], first[b] + n) of slot b, gathered on the device."""
    idx = first[:, None] + torch.arange(n, device=rows.device)
    return torch.gather(rows, 1, idx[:, :, None].expand(-1, -1, rows.shape[2]))


def _stream_layer_generic(c: _LayerCache, st, x, batch, t, dtype, final_ln=None, lens=None):
    """layer_forward for one chunk: the convs run on [history | chunk] rows, the scan from the carried state.  ``lens`` (B,) int32,
    already clamped to [0, t]: slot b's new histories are the rows behind its row lens[b] - 1 and its scan stops there; both convs
    are causal and everything else is row-local, so rows at and past lens[b] reach no valid row."""
    D, E = x.shape[-1], c.d_inner
    first = None if lens is None else lens.long()
    _, h = ops.add_layernorm(x, None, norm2=c.ffn1["ln"], out_dtype=dtype)
    y = _ffn(x, h, c.ffn1, dtype)
    _, h = ops.add_layernorm(x, y, 0.5, x_out=x, norm2=c.norm1, out_dtype=dtype)
    xz = _in_proj(c, h).view(batch, t, 2 * E)
    xe = torch.cat([st.conv_state, xz[:, :, :E]], dim=1)                                    # (batch, 3 + t, E)
    st.conv_state.copy_(xe[:, t:] if first is None else _rows_behind(xe, first, 3))
    ue = torch.empty_like(xe)
    ops.conv_cl_fwd(xe, c.dirs[0]["conv_w"], c.dirs[0]["conv_b"], silu=True, out_f=ue)
    u = ue[:, 3:].contiguous()
    ycat = torch.empty_like(u)
    _scan(c, xz, u, ycat, None, batch, t, state=st.ssm_state, lens=lens)
    _, h = ops.add_layernorm(x, _out_proj(c, ycat.view(batch * t, E)), 1.0, x_out=x, norm2=c.cm_ln, out_dtype=dtype)
    gl = F.glu(torch.addmm(c.pw_b, h, c.pw_w.t()), dim=-1).view(batch, t, D)
    ge = torch.cat([st.dw_state, gl], dim=1)                                                # (batch, 30 + t, D)
    st.dw_state.copy_(ge[:, t:] if first is None else _rows_behind(ge, first, c.kernel_size - 1))
    g = ops.glu_dwconv_ln_gelu(ge, c.dw_w, c.dw_b, c.cm_ln2[0], c.cm_ln2[1], c.cm_ln2[2], weight_t=c.dw_wt, glu_done=True,
                               causal=True)[:, c.kernel_size - 1:]
    y = torch.addmm(c.lin_b, g.reshape(-1, D), c.lin_w.t())
    _, h = ops.add_layernorm(x, y, 1.0, x_out=x, norm2=c.ffn2["ln"], out_dtype=dtype)
    y = _ffn(x, h, c.ffn2, dtype)
    ops.add_layernorm(x, y, 0.5, x_out=x, norm1=c.norm2, want_out=False)
    if final_ln is None:
        return x
    return ops.add_layernorm(x, None, norm2=final_ln, out_dtype=torch.float32)[1]


@torch.no_grad()
def forward_streaming(encoder, src, context, lens=None):
    """ConmambaEncoder.forward_streaming: src (B, t, D), any t >= 1, continues the B streams whose state ``context`` holds ->
    (B, t, D) fp32; the context is updated in place.  The outputs over the chunks of an utterance, concatenated, are the causal
    whole-utterance forward.  The compute dtype is the context's.  No host synchronisation and no data-dependent allocation: a
    fixed (B, t) step can be captured in a hipGraph.

    ``lens``: a device int32 (B,) tensor, 0 <= lens[b] <= t (larger values are clamped on the device; it is never
    read on the host).  Slot b consumes rows [0, lens[b]) of src[b]: its output rows there and its state after the call are, bit for
    bit, those of a lock-step call on that slot alone with t = lens[b]; lens[b] == 0 leaves its state as it was.  Output rows at
    and past lens[b] are unspecified, and what src holds there (NaN included) reaches no valid row and no state of any slot."""
    batch, t, D = src.shape
    sl = None if lens is None else ops.slot_lens(lens, batch, src.device, "forward_streaming")    # the one check of lens, for every launch of the call
    dtype = context.layers[0].conv_state.dtype
    caches = [_cache(layer, dtype) for layer in encoder.layers]
    if not all(c.uni and c.causal and c.rows_mode and c.kernel_size == 31 for c in caches):
        raise NotImplementedError("forward_streaming: a layer is outside the streamed routes (causal layer, dt_rank <= 16, or <= 32 in bf16)")
    native = (USE_STREAM_NATIVE and USE_FUSED_FFN and USE_LN_PW_GLU and dtype == torch.bfloat16 and D == 256
              and all(c.all_native and _conv_forms_xdbl(c) for c in caches))
    fin = _final_norm(encoder)
    n = len(caches)
    with torch.autocast("cuda", enabled=False):
        out = x = _residual_rows(src)
        if not native:
            clamped = None if lens is None else lens.clamp(0, t)
            for i, (c, st) in enumerate(zip(caches, context.layers)):
                out = _stream_layer_generic(c, st, x, batch, t, dtype, fin if i == n - 1 else None, clamped)
            return out.view(batch, t, D)
        E, dev = caches[0].d_inner, src.device
        xz = torch.empty((batch, t, 2 * E), dtype=dtype, device=dev)
        ucat = torch.empty((batch, t, E), dtype=dtype, device=dev)
        ycat = torch.empty_like(ucat)
        xdbl = torch.empty((batch, t, caches[0].row_width), dtype=dtype, device=dev)
        small = 0 < batch * t <= ops.SMALL_FFN_ROWS
        for i, (c, st) in enumerate(zip(caches, context.layers)):
            _head(c, x, xz, ucat, xdbl, small, hist=(st.conv_state, st.conv_spare), lens=sl)
            _scan(c, xz, ucat, ycat, xdbl, batch, t, state=st.ssm_state, lens=sl)
            out = _tail(c, x, ycat.view(batch * t, E), batch, t, fin if i == n - 1 else None, small, hist=(st.dw_state, st.dw_spare), lens=sl)
            st.swap()
        return out.view(batch, t, D)


# ------------------------------------------------------------------------------------------------
# front end + encoder: the whole path the headline metric times (reference train_CTC.py:285-298)
# ------------------------------------------------------------------------------------------------
# cm_cnn_front: both CNN blocks in one kernel; CM_CNN_FRONT=0 = cm_cnn_block1 + cm_cnn_block2
USE_CNN_FRONT = os.environ.get("CM_CNN_FRONT", "1") == "1"


def _frontend_bundle(model, dtype):
    b0, b1 = model.CNN.blocks
    lin = model.Transformer.custom_src_module.layers[0].w
    return dict(w2=b1.conv.weight.detach().to(dtype).contiguous(memory_format=torch.channels_last),
                b2=b1.conv.bias.detach().to(dtype), b2f=b1.conv.bias.detach().float().contiguous(),
                w2_ohwi=b1.conv.weight.detach().to(dtype).permute(0, 2, 3, 1).contiguous(),
                ln2=(b1.norm.norm.weight.detach().float().reshape(-1).contiguous(),
                     b1.norm.norm.bias.detach().float().reshape(-1).contiguous(), b1.norm.norm.eps),
                lin_w=lin.weight.detach().to(dtype).contiguous(), lin_b=lin.bias.detach().to(dtype))


_FRONTEND = weight_cache.Kind("_cm_frontend_cache", graphs_read=False, build=_frontend_bundle)


def _frontend_cache(model, dtype):
    return _FRONTEND.lookup(model, _params_key(dtype, model.CNN, model.Transformer.custom_src_module), dtype)


def _cnn_args(model, c):
    """What ops.cnn_front and ops.cnn_front_stream take for the two CNN blocks: block 1 from the module (fp32), block 2 from the
    front-end cache ``c``, and the LeakyReLU slope."""
    b0 = model.CNN.blocks[0]
    n0 = b0.norm.norm
    return b0.conv.weight, b0.conv.bias, n0.weight, n0.bias, n0.eps, c["w2_ohwi"], c["b2f"], c["ln2"][0], c["ln2"][1], c["ln2"][2], 0.01


def _recipes_front(model) -> bool:
    """The recipes' Fbank and CNN, which the native front-end routes are built for: n_fft 512, 80 bins, channels (64, 32)."""
    fb, b0 = model.compute_features, model.CNN.blocks[0]
    return (ops.fbank_wav_supported(fb.n_fft, fb.hop, fb.n_mels) and fb.n_mels == 80 and tuple(b0.conv.weight.shape) == (64, 1, 3, 3)
            and b0.norm.norm.weight.numel() == 40 * 64 and tuple(model.CNN.blocks[1].conv.weight.shape) == (32, 64, 3, 3))


def ragged_sample_counts(wav_lens, n_total: int, hop: int):
    """Per-utterance sample counts of a padded (B, n_total) batch, on the host: relative lengths (a floating tensor, speechbrain's
    wav_lens) become round(rel * n_total), absolute counts (an integer tensor or a sequence of ints) are taken as they are; one
    .tolist().  An utterance outside [0, n_total] or under the front end's minimum of 5 frames (4 * hop samples) raises ValueError."""
    if isinstance(wav_lens, torch.Tensor):
        vals = wav_lens.detach().tolist()
        counts = [int(round(v * n_total)) for v in vals] if wav_lens.is_floating_point() else [int(v) for v in vals]
    else:
        counts = [int(v) for v in wav_lens]
    for b, n in enumerate(counts):
        if not 0 <= n <= n_total:
            raise ValueError(f"ragged batch: utterance {b} has {n} samples, outside [0, {n_total}]")
        if 1 + n // hop < 5:
            raise ValueError(f"ragged batch: utterance {b} has {n} samples = {1 + n // hop} frames; the front end needs at least 5 "
                             f"frames ({4 * hop} samples)")
    return counts


def frontend_ragged_native(model, wavs, dtype) -> bool:
    """The ragged front end runs on cm_fbank_wav_lens / cm_fbank_finish_lens / cm_cnn_front_lens: GPU, bf16, n_fft 512, the recipes' CNN."""
    from . import sb_compat
    return wavs.is_cuda and dtype == torch.bfloat16 and USE_CNN_FRONT and sb_compat.USE_FBANK_WAV and _recipes_front(model)


@torch.no_grad()
def frontend_ragged(model, wavs, n_samples, dtype=torch.bfloat16):
    """The whole-utterance front end on a padded batch whose utterance b has n_samples[b] samples (host ints, checked by
    ragged_sample_counts): -> (rows (B, T2_max, 640) bf16, row_lens, frames) with row_lens a RowLens of frontend_rows_total(n_samples[b],
    hop) and frames the device int32 (B,) frame counts.  Rows [0, row_lens[b]) are those of the front end on wavs[b:b+1, :n_samples[b]]
    alone; rows past them are unspecified.  Three device arrays (samples, frames, rows) are built once; the kernels read them."""
    fb, hop = model.compute_features, model.compute_features.hop
    frames = [1 + n // hop for n in n_samples]
    rows = [frontend_rows_total(n, hop) for n in n_samples]
    counts = torch.tensor([list(n_samples), frames, rows], dtype=torch.int32).to(wavs.device)
    with torch.autocast("cuda", enabled=False):
        feats = ops.fbank_from_wav(wavs, fb.window, fb.n_fft, hop, fb.fbank, fb.amin, fb.top_db, model.normalize.glob_mean,
                                   model.normalize.glob_std, lens=counts[0])
        src = ops.cnn_front(feats, *_cnn_args(model, _frontend_cache(model, dtype)), lens=counts[1])
    return src, RowLens(rows, counts[2]), counts[1]


def _asr_encode_ragged(model, wavs, n_samples, dtype):
    """asr_encode on a padded batch with per-utterance sample counts -> (enc (B, T2_max, d_model) fp32, row_lens)."""
    batch = wavs.shape[0]
    if frontend_ragged_native(model, wavs, dtype):
        src, row_lens, _ = frontend_ragged(model, wavs, n_samples, dtype)
        c = _frontend_cache(model, dtype)
        t2 = src.shape[1]
        with torch.autocast("cuda", enabled=False):
            x = torch.addmm(c["lin_b"], src.view(batch * t2, -1), c["lin_w"].t())           # row-local: a row past an utterance's own stays there
        return encoder_forward(model.Transformer.encoder, x.view(batch, t2, -1), dtype, lens=row_lens.dev), row_lens
    # any other configuration: each utterance alone through the route without lengths, scattered
    hop = model.compute_features.hop
    rows = [frontend_rows_total(n, hop) for n in n_samples]
    out = None
    for b, n in enumerate(n_samples):
        e = asr_encode(model, wavs[b:b + 1, :n], None, dtype)
        if out is None:
            out = torch.zeros((batch, max(rows), e.shape[-1]), dtype=e.dtype, device=e.device)
        out[b, :rows[b]] = e[0]
    return out, RowLens(rows, torch.tensor(rows, dtype=torch.int32).to(wavs.device))


@torch.no_grad()
def asr_encode(model, wavs, wav_lens, dtype: Optional[torch.dtype] = None, n_samples=None):
    """ConMambaASR.encode in eval mode through native kernels: Fbank (torch.stft/rocFFT + mel GEMM) -> global
    normalisation -> the two CNN blocks -> src Linear -> fused encoder.  The CNN blocks (conv + LayerNorm + LeakyReLU
    each) run as cm_cnn_front, both in one kernel (bf16, the recipes' shapes); else cm_cnn_block1 (the next block's
    reflect border included) + cm_cnn_block2 (bf16); else cm_cnn_block1 + library conv (64->32, 3x3, stride 2,
    channels-last, unpadded) + cm_add_layernorm (LN + LeakyReLU).  Returns (batch, ceil(T/4), d_model) fp32.

    ``n_samples``: per-utterance sample counts as host ints (ragged_sample_counts) -> (enc, row_lens): utterance b's rows
    [0, row_lens[b]) are those of this function on wavs[b:b+1, :n_samples[b]] alone, row_lens a RowLens.  ``wav_lens`` itself is not
    read on either path (the reference computes a padding mask from it and discards it)."""
    if dtype is None:
        dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled("cuda") else torch.float32
    if n_samples is not None:
        return _asr_encode_ragged(model, wavs, list(n_samples), dtype)
    with torch.autocast("cuda", enabled=False):
        # Fbank back end + frozen global normalisation in the native kernels (cm_fbank_mel_db / cm_fbank_finish)
        feats = model.compute_features(wavs, norm=(model.normalize.glob_mean, model.normalize.glob_std))
        c = _frontend_cache(model, dtype)
        b0 = model.CNN.blocks[0]
        n0 = b0.norm.norm
        if (USE_CNN_FRONT and dtype == torch.bfloat16 and ops.cnn_front_supported(feats, b0.conv.weight, c["w2_ohwi"])
                and n0.weight.numel() == 40 * 64):
            # both CNN blocks in one kernel: the (B, T/2 + 2, 42, 64) intermediate never reaches memory
            src = ops.cnn_front(feats, *_cnn_args(model, c))                            # (B, T2, 640)
        else:
            y1 = ops.cnn_block1(feats, b0.conv.weight, b0.conv.bias, n0.weight, n0.bias, n0.eps, 0.01, out_dtype=dtype,
                                pad_out=1)                                              # (B, T1+2, F1+2, 64) NHWC
            if dtype == torch.bfloat16 and tuple(c["w2_ohwi"].shape) == (32, 3, 3, 64):
                src = ops.cnn_block2(y1, c["w2_ohwi"], c["b2f"], c["ln2"][0], c["ln2"][1], c["ln2"][2], 0.01)   # (B, T2, 640)
            else:
                y2 = F.conv2d(y1.permute(0, 3, 1, 2), c["w2"], c["b2"], stride=2)       # channels_last in / out
                y2 = y2.permute(0, 2, 3, 1).contiguous()                                # (B, T2, F2, 32)
                _, src = ops.add_layernorm(None, y2.flatten(2), norm2=c["ln2"], out_dtype=dtype, out_act=1)
        batch, t2 = src.shape[:2]
        x = torch.addmm(c["lin_b"], src.view(batch * t2, -1), c["lin_w"].t())           # (rows, D)
        return encoder_forward(model.Transformer.encoder, x.view(batch, t2, -1), dtype)


# ------------------------------------------------------------------------------------------------
# the front end as a stream: waveform chunks -> the CNN's rows
# ------------------------------------------------------------------------------------------------
# Encoder row r reads feature frames 4r - 3 .. 4r + 3 and frame f the samples [hop f - n_fft/2, hop f + n_fft/2): mid-stream the
# front end has a finite look-ahead, and what a call returns is host arithmetic on the sample count.  The reflect borders of the
# CNN blocks and the STFT's zero padding are applied at the two ends of the utterance only (reset / last=True).  The top_db clamp
# is the causal one (floor of frame f = max dB of frames 0..f - top_db; sb_compat.Fbank(causal_top_db=True) is its whole-utterance
# form).  Native route (GPU, bf16, n_fft 512, the recipes' CNN): cm_fbank_wav_stream, cm_fbank_finish_stream, cm_cnn_front_stream
# -- three launches, no torch.cat, no torch.stft; the sample and feature histories are double-buffered and swapped.
# CM_STREAM_FRONT_NATIVE=0 = the generic torch route (also: fp32, n_fft 400, CPU tensors).
USE_STREAM_FRONT_NATIVE = os.environ.get("CM_STREAM_FRONT_NATIVE", "1") == "1"


def frontend_frames_ready(n_samples: int, n_fft: int, hop: int) -> int:
    """Feature frames that are final after ``n_samples`` samples of an unfinished utterance."""
    return 0 if n_samples < n_fft // 2 else (n_samples - n_fft // 2) // hop + 1


def frontend_rows_ready(n_samples: int, n_fft: int, hop: int) -> int:
    """CNN front-end rows that are final after ``n_samples`` samples of an unfinished utterance (row r needs frame 4r + 3)."""
    f = frontend_frames_ready(n_samples, n_fft, hop)
    return 0 if f < 4 else (f - 4) // 4 + 1


def frontend_rows_total(n_samples: int, hop: int) -> int:
    """Rows of a finished utterance of ``n_samples`` samples: T = 1 + S // hop frames, T1 = ceil(T / 2), T2 = ceil(T1 / 2)."""
    t1 = (1 + n_samples // hop + 1) // 2
    return (t1 + 1) // 2


class FrontEndStreamingContext:
    """What the streamed front end carries from one call to the next for ``batch_size`` streams in lock step: the last 512 samples
    and the last 8 feature rows (each with the spare the native kernels write the new history into), the running dB maximum of
    the causal top_db clamp, and the host counters samples / frames / rows.  About 9 KB per stream.  The generic route keeps its
    own (shorter) sample and feature tails in ``tail``.  ``dtype`` is the dtype of the rows that come out."""

    def __init__(self, batch_size, device, dtype):
        self.batch_size, self.device, self.dtype = int(batch_size), torch.device(device), dtype
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.samp_hist, self.samp_spare = z(batch_size, ops.FRONT_HIST_SAMPLES), z(batch_size, ops.FRONT_HIST_SAMPLES)
        self.feat_hist, self.feat_spare = z(batch_size, ops.FRONT_HIST_FRAMES, 80), z(batch_size, ops.FRONT_HIST_FRAMES, 80)
        self.umax = torch.full((batch_size,), float("-inf"), dtype=torch.float32, device=self.device)
        self.reset()

    def reset(self, rows=None):
        """The start of a new utterance on every stream.  Per-slot resets are not offered: streams that end at different samples
        would yield different row counts per call, and the encoder behind takes one row count for all slots."""
        if rows is not None:
            raise NotImplementedError("FrontEndStreamingContext.reset(rows=...): the streams of a front-end context advance in lock step "
                                      "(one sample count, one row count per call); reset all of them, or keep one context per stream")
        for t in (self.samp_hist, self.samp_spare, self.feat_hist, self.feat_spare):
            t.zero_()
        self.umax.fill_(float("-inf"))
        self.samples = self.frames = self.rows = 0
        self.finished = False
        self.tail = None


class ASRStreamingContext:
    """ConMambaASR.make_streaming_context: ``frontend`` (FrontEndStreamingContext) and ``encoder`` (what
    Transformer.make_streaming_context returns); ``reset`` starts a new utterance on every stream of both."""

    def __init__(self, frontend, encoder):
        self.frontend, self.encoder = frontend, encoder

    def reset(self):
        self.frontend.reset()
        self.encoder.encoder_context.reset()


def _front_plan(model, ctx, wav_chunk, last):
    """Host arithmetic of one call: (n_fft, hop, first frame, frames, first row, rows, T or -1)."""
    fb = model.compute_features
    if wav_chunk.dim() != 2 or wav_chunk.shape[0] != ctx.batch_size:
        raise ValueError(f"frontend_streaming: wav_chunk must be (batch, n) with batch = {ctx.batch_size}, the context's; got {tuple(wav_chunk.shape)}")
    if ctx.finished:
        raise RuntimeError("frontend_streaming: the utterance was finished (last=True); reset() the context before the next one")
    total = ctx.samples + wav_chunk.shape[1]
    if last:
        T = 1 + total // fb.hop
        if T < 5:
            raise RuntimeError(f"frontend_streaming: the finished utterance has {T} feature frames; the CNN front end needs at least 5 frames")
        f1, r1 = T, frontend_rows_total(total, fb.hop)
    else:
        T, f1, r1 = -1, frontend_frames_ready(total, fb.n_fft, fb.hop), frontend_rows_ready(total, fb.n_fft, fb.hop)
    return fb.n_fft, fb.hop, ctx.frames, f1 - ctx.frames, ctx.rows, r1 - ctx.rows, T


def _front_norm(model, n_mels, device):
    """The frozen global statistics as (n_mels,) fp32 vectors; uncalibrated ones are (1,)-shaped and broadcast."""
    mean, std = model.normalize.glob_mean, model.normalize.glob_std
    return (mean.detach().float().to(device).expand(n_mels).contiguous(), std.detach().float().to(device).expand(n_mels).contiguous())


def _reflect(i, n):
    return -i if i < 0 else (2 * n - 2 - i if 0 <= n <= i else i)


def _conv_block_rows(blk, x):
    """One ConvolutionFrontEnd block on rows whose time border is already in place: x (B, L, F, C) -> (B, (L - 3) // 2 + 1, F', C')."""
    y = F.pad(x.permute(0, 3, 1, 2), (1, 1, 0, 0), mode="reflect")                   # the frequency border only
    return blk.act(blk.norm(blk.conv(y).permute(0, 2, 3, 1)))


def _front_generic(model, wav_chunk, ctx, last, plan):
    n_fft, hop, f0, nf, r0, nr, T = plan
    fb, dev, half = model.compute_features, wav_chunk.device, n_fft // 2
    B = ctx.batch_size
    if ctx.tail is None:       # samples from index s0 on (the zeros in front of the utterance included), features from frame g0 on
        ctx.tail = dict(s0=-half, samp=torch.zeros(B, half, dtype=torch.float32, device=dev), g0=0,
                        feat=torch.zeros(B, 0, fb.n_mels, dtype=torch.float32, device=dev))
    tl = ctx.tail
    parts = [tl["samp"], wav_chunk.float()] + ([torch.zeros(B, half, dtype=torch.float32, device=dev)] if last else [])
    samp = torch.cat(parts, dim=1)
    feat = tl["feat"]
    if nf > 0:
        seg = samp[:, hop * f0 - half - tl["s0"]: hop * (f0 + nf - 1) + half - tl["s0"]]
        spec = torch.stft(seg, n_fft, hop, fb.win, fb.window.to(dev), center=False, normalized=False, onesided=True, return_complex=True)
        power = (spec.real ** 2 + spec.imag ** 2).transpose(1, 2)
        db = 10.0 * torch.log10(torch.clamp(power @ fb.fbank.to(dev), min=fb.amin))                     # (B, nf, n_mels)
        run = torch.maximum(db.amax(dim=-1).cummax(dim=1).values, ctx.umax.to(dev)[:, None])       # prefix maximum, seeded with the carried one
        ctx.umax = run[:, -1].contiguous()
        mean, std = _front_norm(model, fb.n_mels, dev)
        feat = torch.cat([feat, (torch.maximum(db, run[..., None] - fb.top_db) - mean) / std], dim=1)
        keep = hop * (f0 + nf) - half - tl["s0"]
        tl["samp"], tl["s0"] = samp[:, keep:].clone(), tl["s0"] + keep
    else:
        tl["samp"] = samp
    out = torch.zeros(B, 0, 640, dtype=ctx.dtype, device=dev)
    if nr > 0:
        b0, b1 = model.CNN.blocks
        T1 = (T + 1) // 2 if T >= 0 else -1
        t1s = [_reflect(t, T1) for t in range(2 * r0 - 1, 2 * (r0 + nr))]             # block-1 rows under block 2's taps
        lo, hi = min(t1s), max(t1s)
        frames = [_reflect(f, T) - tl["g0"] for f in range(2 * lo - 1, 2 * hi + 2)]   # feature frames under block 1's taps
        # block 1 in fp32 and its rows rounded once to the compute dtype, block 2's conv in that dtype: cm_cnn_front's precision
        y1 = _conv_block_rows(b0, feat[:, frames, :, None]).to(ctx.dtype)              # rows lo .. hi
        with torch.autocast(dev.type, dtype=ctx.dtype, enabled=ctx.dtype != torch.float32):
            out = _conv_block_rows(b1, y1[:, [t - lo for t in t1s]])
        out = out.flatten(2).to(ctx.dtype)
        keep = max(4 * (r0 + nr) - 3, 0) - tl["g0"]
        feat, tl["g0"] = feat[:, keep:].clone(), tl["g0"] + keep
    tl["feat"] = feat
    return out


def _front_native(model, wav_chunk, ctx, last=False, plan=None, slots=None):
    """The native route of one call -> out.  Lock step: ``plan`` is _front_plan's; no host-to-device copy and no pinned allocation, so
    the call stays capturable.  Per slot: ``slots``, _slot_plan's table, stands in place of ``last`` and ``plan``; the kernels read it from
    the device, the counts handed to them are the maxima over the slots, and -> (out, lens_dev)."""
    fb, B, dev = model.compute_features, ctx.batch_size, wav_chunk.device
    if slots is None:
        n_fft, hop, f0, nf, r0, nr, T = plan
        n, consumed, table, alloc = wav_chunk.shape[1], ctx.samples, None, torch.empty
        total = consumed + n if last else -1
    else:
        n_fft, hop, f0, r0, T, consumed, total = fb.n_fft, fb.hop, 0, 0, -1, 0, -1
        n, nf, nr = (max(p[k] for p in slots) for k in (0, 4, 6))
        host = torch.tensor(slots, dtype=torch.int32).pin_memory()
        table = (host, host.to(dev, non_blocking=True))
        lens_dev = table[1][:, 6].contiguous()
        alloc = torch.zeros                                # rows past a slot's own count stay zero
    if n == 0 and nf == 0:                                 # nothing arrived and no utterance ends: no launch
        out = alloc((B, 0, 640), dtype=torch.bfloat16, device=dev)
        return out if slots is None else (out, lens_dev)
    if wav_chunk.dtype != torch.float32 or (wav_chunk.shape[1] and wav_chunk.stride(1) != 1):
        wav_chunk = wav_chunk.float().contiguous()
    db, fmax = ops.fbank_wav_stream(wav_chunk, ctx.samp_hist, ctx.samp_spare, consumed, f0, nf, fb.window, n_fft, hop, fb.fbank, fb.amin,
                                    total=total, plan=table)
    ctx.samp_hist, ctx.samp_spare = ctx.samp_spare, ctx.samp_hist
    out = alloc((B, max(nr, 0), 640), dtype=torch.bfloat16, device=dev)
    if nf == 0:
        return out if slots is None else (out, lens_dev)
    mean, std = _front_norm(model, fb.n_mels, dev)
    ops.fbank_finish_stream(db, fmax, ctx.umax, f0, fb.top_db, mean, std, ctx.feat_hist, ctx.feat_spare, n_fft=n_fft, plan=table)
    if nr > 0:
        ops.cnn_front_stream(db, ctx.feat_hist, f0, r0, nr, *_cnn_args(model, _frontend_cache(model, torch.bfloat16)), t_total=T, out=out,
                             plan=table)
    ctx.feat_hist, ctx.feat_spare = ctx.feat_spare, ctx.feat_hist
    return out if slots is None else (out, lens_dev)


def frontend_streaming_native(model, ctx) -> bool:
    """Whether frontend_streaming takes the native route for this model and context."""
    return USE_STREAM_FRONT_NATIVE and ctx.device.type == "cuda" and ctx.dtype == torch.bfloat16 and _recipes_front(model)


@torch.no_grad()
def frontend_streaming(model, wav_chunk, ctx: FrontEndStreamingContext, last: bool = False):
    """The next ``n`` samples (B, n), any n >= 0, of the B streams whose state ``ctx`` holds -> the CNN front end's rows that became
    final, (B, t, 640) in the context's dtype (t may be 0): rows frontend_rows_ready(before) .. frontend_rows_ready(after) - 1, and
    with ``last`` every remaining row of the utterance, with the end-of-utterance zero padding and reflections.  Concatenated over
    the calls of an utterance the rows do not depend on the chunking.  No host synchronisation, no data-dependent shape."""
    plan = _front_plan(model, ctx, wav_chunk, last)
    with torch.autocast("cuda", enabled=False):
        if frontend_streaming_native(model, ctx) and wav_chunk.is_cuda:
            out = _front_native(model, wav_chunk, ctx, last, plan)
        else:
            out = _front_generic(model, wav_chunk, ctx, last, plan)
    ctx.samples += wav_chunk.shape[1]
    ctx.frames += plan[3]
    ctx.rows += plan[5]
    ctx.finished = bool(last)
    return out


# ------------------------------------------------------------------------------------------------
# the front end with every slot at its own pace: per-slot sample counts, ends and resets
# ------------------------------------------------------------------------------------------------
class RowLens(list):
    """The rows every slot got from one frontend_streaming_slots call: a host list of ints (what StreamingCTCBeamSearcher.step takes
    as ``lengths``) whose ``dev`` is the same as a device int32 (B,) tensor (what encode_streaming takes as ``lens``)."""

    def __init__(self, values, dev):
        super().__init__(values)
        self.dev = dev


class SlotFrontEndStreamingContext:
    """FrontEndStreamingContext for ``batch_size`` slots that advance independently: the same device state (sample history, feature
    history, each with its spare, and umax), and the host counters samples / frames / rows / finished as lists, one entry per slot.
    ``reset(rows)`` starts a new utterance in the listed slots (default all) with device index_fill_, no synchronisation."""

    def __init__(self, batch_size, device, dtype):
        self.batch_size, self.device, self.dtype = int(batch_size), torch.device(device), dtype
        z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.samp_hist, self.samp_spare = z(batch_size, ops.FRONT_HIST_SAMPLES), z(batch_size, ops.FRONT_HIST_SAMPLES)
        self.feat_hist, self.feat_spare = z(batch_size, ops.FRONT_HIST_FRAMES, 80), z(batch_size, ops.FRONT_HIST_FRAMES, 80)
        self.umax = torch.full((batch_size,), float("-inf"), dtype=torch.float32, device=self.device)
        self.samples, self.frames, self.rows, self.finished = ([0] * self.batch_size for _ in range(4))
        self.subs = None                  # generic route: one lock-step context of one stream per slot
        self.reset()

    def reset(self, rows=None):
        rows = list(range(self.batch_size)) if rows is None else [int(r) for r in rows]
        if any(not 0 <= r < self.batch_size for r in rows):
            raise ValueError(f"SlotFrontEndStreamingContext.reset: rows {rows} outside a context of {self.batch_size} slots")
        if rows:
            idx = torch.as_tensor(rows, dtype=torch.long).to(self.device, non_blocking=True)
            self.samp_hist.index_fill_(0, idx, 0.0)
            self.feat_hist.index_fill_(0, idx, 0.0)
            self.umax.index_fill_(0, idx, float("-inf"))
        for r in rows:
            self.samples[r] = self.frames[r] = self.rows[r] = 0
            self.finished[r] = False
            if self.subs is not None:
                self.subs[r].reset()


class SlotASRStreamingContext:
    """ConMambaASR.make_streaming_context(per_slot=True): ``frontend`` (SlotFrontEndStreamingContext) and ``encoder``; ``reset(rows)``
    starts a new utterance in the listed slots (default all) of both."""

    def __init__(self, frontend, encoder):
        self.frontend, self.encoder = frontend, encoder

    def reset(self, rows=None):
        self.frontend.reset(rows)
        self.encoder.encoder_context.reset(rows)


def _slot_plan(model, ctx, wav_chunk, n_valid, last):
    """Host arithmetic of one per-slot call, nothing changed: -> (rows of the plan table {n, consumed, total, f0, nf, r0, nr, T}, ends).
    Every refusal is raised here, before anything is launched or any counter moves."""
    fb, B = model.compute_features, ctx.batch_size
    if wav_chunk.dim() != 2 or wav_chunk.shape[0] != B:
        raise ValueError(f"frontend_streaming_slots: wav_chunk must be (batch, n_max) with batch = {B}, the context's; got {tuple(wav_chunk.shape)}")
    n_max = wav_chunk.shape[1]
    n_valid = [int(n) for n in n_valid]
    ends = [bool(last)] * B if isinstance(last, (bool, int)) else [bool(x) for x in last]
    if len(n_valid) != B or len(ends) != B:
        raise ValueError(f"frontend_streaming_slots: n_valid and last must have {B} entries (got {len(n_valid)} and {len(ends)})")
    plan = []
    for b, n in enumerate(n_valid):
        if not 0 <= n <= n_max:
            raise ValueError(f"frontend_streaming_slots: n_valid[{b}] = {n} outside [0, {n_max}]")
        if ctx.finished[b]:
            if n != 0:
                raise ValueError(f"frontend_streaming_slots: slot {b} has finished its utterance and takes no samples until it is reset (got {n})")
            ends[b] = False
            plan.append([0, ctx.samples[b], -1, ctx.frames[b], 0, ctx.rows[b], 0, -1])
            continue
        total = ctx.samples[b] + n
        if ends[b]:
            T = 1 + total // fb.hop
            if T < 5:
                raise RuntimeError(f"frontend_streaming_slots: slot {b} ends its utterance with {T} feature frames; the CNN front end needs at least 5 frames")
            f1, r1 = T, frontend_rows_total(total, fb.hop)
        else:
            T, f1, r1 = -1, frontend_frames_ready(total, fb.n_fft, fb.hop), frontend_rows_ready(total, fb.n_fft, fb.hop)
        plan.append([n, ctx.samples[b], total if ends[b] else -1, ctx.frames[b], f1 - ctx.frames[b], ctx.rows[b], r1 - ctx.rows[b], T])
    return plan, ends


def _front_generic_slots(model, wav_chunk, ctx, plan, ends):
    """The lock-step generic route per slot, on one single-stream context each; the rows padded with zeros to the widest slot."""
    B, dev = ctx.batch_size, wav_chunk.device
    if ctx.subs is None:
        ctx.subs = [FrontEndStreamingContext(1, ctx.device, ctx.dtype) for _ in range(B)]
    nr_max = max(p[6] for p in plan)
    out = torch.zeros((B, nr_max, 640), dtype=ctx.dtype, device=dev)
    for b, p in enumerate(plan):
        if p[0] == 0 and not ends[b]:
            continue
        sub = ctx.subs[b]
        lock = _front_plan(model, sub, wav_chunk[b:b + 1, :p[0]], ends[b])
        rows = _front_generic(model, wav_chunk[b:b + 1, :p[0]], sub, ends[b], lock)
        sub.samples, sub.frames, sub.rows, sub.finished = sub.samples + p[0], sub.frames + lock[3], sub.rows + lock[5], ends[b]
        assert rows.shape[1] == p[6], (b, rows.shape, p)
        out[b, :p[6]] = rows[0]
    return out, torch.tensor([p[6] for p in plan], dtype=torch.int32).to(dev, non_blocking=True)


@torch.no_grad()
def frontend_streaming_slots(model, wav_chunk, n_valid, ctx: SlotFrontEndStreamingContext, last=False):
    """The next samples of B slots that advance independently: wav_chunk (B, n_max), of which slot b hands over its first n_valid[b]
    (a host sequence of ints, 0 allowed; samples at and past it are never read by the native route); ``last`` a bool or a sequence of
    B bools, last[b] ending slot b's utterance at samples[b] + n_valid[b] with the whole-utterance treatment of the end.  ->
    (rows (B, t_max, 640), row_lens): row_lens[b] is what frontend_streaming gives that slot alone (a RowLens: host list, ``.dev`` the
    device int32 tensor), t_max its maximum, rows at and past row_lens[b] zeros.  A finished slot takes only n_valid[b] = 0 until it
    is reset (ValueError names it); a slot that ends under 5 frames raises; both before anything is launched or any counter moves.
    Native route: three launches, two when no slot has a row, one when none has a frame, none when nothing arrived and no slot ends."""
    plan, ends = _slot_plan(model, ctx, wav_chunk, n_valid, last)
    with torch.autocast("cuda", enabled=False):
        if frontend_streaming_native(model, ctx) and wav_chunk.is_cuda:
            out, lens_dev = _front_native(model, wav_chunk, ctx, slots=plan)
        else:
            out, lens_dev = _front_generic_slots(model, wav_chunk, ctx, plan, ends)
    for b, p in enumerate(plan):
        ctx.samples[b] += p[0]
        ctx.frames[b] += p[4]
        ctx.rows[b] += p[6]
        ctx.finished[b] = ctx.finished[b] or ends[b]
    return out, RowLens([p[6] for p in plan], lens_dev)


class GraphedEncode:
    """hipGraph capture of ConMambaASR.encode for fixed-shape, device-resident inputs.

    A ConMamba-large forward is ~450 short kernels; launched eagerly from Python the host needs ~9.5 ms per step,
    more than the GPU does.  Capturing the launch sequence once and replaying it removes that bound (MI355X:
    8.5 ms replay vs 9.5 ms eager at the round-1 kernel set).  Inputs are copied into static buffers; the returned
    tensor is the graph's static output (valid until the next replay)."""

    def __init__(self, model, wavs, wav_lens, dtype=torch.bfloat16, warmup: int = 2):
        self.model, self.dtype = model, dtype
        self.wavs, self.lens = wavs.clone(), wav_lens.clone()
        side = torch.cuda.Stream(device=wavs.device)
        side.wait_stream(torch.cuda.current_stream(wavs.device))
        with torch.cuda.stream(side):                      # warm-up outside capture: caches, library handles, LDS attributes
            for _ in range(warmup):
                self._run()
        torch.cuda.current_stream(wavs.device).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._run()

    def _run(self):
        with torch.no_grad(), torch.autocast("cuda", dtype=self.dtype, enabled=self.dtype != torch.float32):
            return self.model.encode(self.wavs, self.lens)

    def __call__(self, wavs=None, wav_lens=None):
        if wavs is not None:
            self.wavs.copy_(wavs)
        if wav_lens is not None:
            self.lens.copy_(wav_lens)
        self.graph.replay()
        return self.out
