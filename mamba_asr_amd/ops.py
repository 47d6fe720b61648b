"""Tensor-level wrappers over the C ABI (include/conmamba_hip.h).

These play the role of the reference's binary extension modules
``selective_scan_cuda`` / ``causal_conv1d_cuda`` (reference
modules/mamba/selective_scan_interface.py:15-16): torch tensors in, torch tensors out, all
arithmetic in the HIP library.  PyTorch is used for device memory and the stream only.
"""
from __future__ import annotations

import ctypes as ct
from typing import Optional, Tuple

import math
import os

import torch

from . import _native as N
from . import weight_cache
from .weight_cache import invalidate_caches          # noqa: F401 -- the entry point callers and the load_state_dict hook know

_DT = {torch.float32: N.CM_F32, torch.bfloat16: N.CM_BF16, torch.float16: N.CM_F16}


# Gradient reductions across workgroups (scan backward: dA / dB / dC / dD / ddelta_bias; causal conv backward: dweight /
# dbias) run as per-workgroup partials + a fixed-order second pass: bit-identical gradients from run to run (what
# SURVEY.md §8d config 4's 1-GPU vs 8-GPU comparison needs to be meaningful at fp32).  CM_DETERMINISTIC=0 switches to
# the fp32 atomics the CUDA kernels behind the reference use (no workspace, order-dependent last bits).
DETERMINISTIC = os.environ.get("CM_DETERMINISTIC", "1") == "1"


# When set to a list, every native launch is bracketed by HIP events recorded on the stream the kernel
# is launched on; entries are (kernel_name, start_event, end_event, units).  Used by bench.py's roofline leg.
LAUNCH_LOG: Optional[list] = None


def _launch(name: str, fn, args, units: int = 0):
    log = LAUNCH_LOG
    if log is None:
        N.check(fn(ct.byref(args)), name)
        return
    st = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    N.check(fn(ct.byref(args)), name)
    e1.record(st)
    log.append((name, e0, e1, units))


# The three kinds cached on the parameter they derive from (weight_cache.py holds the protocol); captured training graphs read them all.
_CAST = weight_cache.Kind("_cm_cast", graphs_read=True, key_of=weight_cache.param_key,
                          build=lambda p, dtype: p.detach().to(dtype), refresh_=lambda old, p, dtype: old.copy_(p.detach()),
                          usable=lambda old, p, dtype: old.dtype == dtype and old.device == p.device,
                          reusable=lambda old, p, dtype: old.shape == p.shape)


def _pack_kind(attr, matrix, shape):
    """A PackedWeight of the bf16 matrix ``matrix(p)``, whose shape is ``shape(p)``."""
    return weight_cache.Kind(attr, graphs_read=True, key_of=weight_cache.param_key,
                             build=lambda p: PackedWeight(matrix(p)), refresh_=lambda old, p: old.repack_(matrix(p)),
                             usable=lambda old, p: old.data.device == p.device, reusable=lambda old, p: old.shape == shape(p))


_PACK = _pack_kind("_cm_pack", lambda p: cast_cached(p, torch.bfloat16), lambda p: tuple(p.shape))
_PACK_T = _pack_kind("_cm_pack_t", lambda p: cast_cached(p, torch.bfloat16).t().contiguous(), lambda p: tuple(p.shape)[::-1])


def cast_cached(p: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """p in `dtype`, without autograd, cached on the tensor until it is modified in place (optimizer step, load_state_dict,
    broadcast): the autograd nodes of this package use a weight's bf16 copy in forward AND backward, several times per
    step, and autocast's own cache does not reach into custom Functions."""
    if p.dtype == dtype:
        return p.detach()
    return _CAST.lookup(p, weight_cache.param_key(p), dtype)


def reflect_pad_tf(x, pad, backward=False, shape=None):
    """Reflect padding of the time and frequency axes of a channels-last (batch, time, freq, channels) tensor (cm_reflect_pad_tf).
    backward: x is the padded tensor's gradient and ``shape`` the source's shape -> the gradient folded back."""
    _dev_check(x)
    if x.dim() != 4 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("reflect_pad_tf: expected a contiguous (batch, time, freq, channels) fp32 / bf16 tensor")
    if backward:
        b, t, f, c = shape
        if tuple(x.shape) != (b, t + 2 * pad, f + 2 * pad, c):
            raise RuntimeError("reflect_pad_tf: gradient shape does not match the padded source shape")
        out = torch.empty((b, t, f, c), dtype=x.dtype, device=x.device)
    else:
        b, t, f, c = x.shape
        out = torch.empty((b, t + 2 * pad, f + 2 * pad, c), dtype=x.dtype, device=x.device)
    rc = N.lib().cm_reflect_pad_tf(_ptr(x), _ptr(out), b, t, f, c, int(pad), _DT[x.dtype], int(bool(backward)), _stream())
    N.check(rc, "cm_reflect_pad_tf")
    return out


class ReflectPadTfFn(torch.autograd.Function):
    """autograd node over cm_reflect_pad_tf (torch: F.pad(..., mode='reflect') on the 5-d view, 448 / 851 us at block 2's size)."""

    @staticmethod
    def forward(ctx, x, pad):
        ctx.pad, ctx.shape = pad, tuple(x.shape)
        return reflect_pad_tf(x if x.is_contiguous() else x.contiguous(), pad)

    @staticmethod
    def backward(ctx, dy):
        return reflect_pad_tf(dy if dy.is_contiguous() else dy.contiguous(), ctx.pad, backward=True, shape=ctx.shape), None


def wgrad(a, b, nbatch=None, variant=0, bufs=None):
    """dW (M, N) fp32 = a^T b for a (rows, M), b (rows, N): the weight gradient of a Linear from its output gradient and its input.
    bf16 operands with M, N multiples of 128: cm_wgrad_bf16 (split over row chunks, fixed-order fold).  Otherwise ``nbatch``
    batched GEMMs over equal row chunks folded by cm_sum_leading (fp32 accumulation in a fixed order either way).
    ``bufs``: caller-supplied ``out`` (M, N) and ``workspace`` (cm_wgrad_workspace_floats) of the cm_wgrad_bf16 route."""
    _dev_check(a, b)
    rows, M = a.shape
    Nn = b.shape[1]
    if (a.dtype == torch.bfloat16 and b.dtype == torch.bfloat16 and a.stride(1) == 1 and b.stride(1) == 1 and a.stride(0) % 8 == 0
            and b.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and N.lib().cm_wgrad_supported(rows, M, Nn)):
        args = N.WgradArgs()
        args.rows, args.m, args.n, args.variant = rows, M, Nn, int(variant)   # 0: the library picks; 1 registers, 2 LDS-DMA staging
        args.a, args.b, args.lda, args.ldb = _ptr(a), _ptr(b), a.stride(0), b.stride(0)
        nws = int(N.lib().cm_wgrad_workspace_floats(rows, M, Nn))
        take = _bufs(bufs, ("out", "workspace"), "wgrad")
        ws = take("workspace", (nws,), torch.float32, a.device)
        out = take("out", (M, Nn), torch.float32, a.device)
        args.out, args.workspace, args.workspace_floats, args.stream = _ptr(out), _ptr(ws), nws, _stream()
        _launch("cm_wgrad_bf16", N.lib().cm_wgrad_bf16, args, units=rows)
        return out
    if bufs is not None:
        raise RuntimeError("wgrad: bufs places the buffers of cm_wgrad_bf16, which does not take these operands")
    nb = nbatch if (nbatch and rows % nbatch == 0) else 1
    return sum_leading(torch.bmm(a.view(nb, rows // nb, M).transpose(1, 2), b.view(nb, rows // nb, Nn)))


def pack_cached(p: torch.Tensor) -> "PackedWeight":
    """p (2-D parameter) as a bf16 PackedWeight (cm_ffn_fused's fragment-tiled image), cached like cast_cached."""
    return _PACK.lookup(p, weight_cache.param_key(p))


def pack_cached_t(p: torch.Tensor) -> "PackedWeight":
    """p^T as a bf16 PackedWeight (the "weights" of cm_ffn_bwd_fused's two GEMMs), cached like cast_cached."""
    return _PACK_T.lookup(p, weight_cache.param_key(p))


def ffn_bwd_fused(dout, w2t, w1t, pre, alpha, p1, p2, seed1, seed2, bufs=None):
    """The data-gradient chain of a feed-forward module's backward in one kernel (cm_ffn_bwd_fused), for the forward
    ffn_fused(..., train=(p1, p2, seed1, seed2)) ran.  dout (rows, 256) fp32; w2t / w1t PackedWeight of W2^T (hidden, 256) /
    W1^T (256, hidden); pre (rows, hidden) bf16.  -> (da2, da1, act, dh, db1, db2): bf16 (rows, 256) / (rows, hidden) x 2 /
    (rows, 256), fp32 (hidden) / (256).
    ``bufs``: caller-supplied ``da2`` / ``da1`` / ``act`` / ``dh``, ``db1`` (hidden + 256 floats: [db1 | db2], which the C contract
    wants adjacent) and ``workspace`` (cm_ffn_bwd_workspace_floats)."""
    _dev_check(dout, pre)
    rows, d = dout.shape
    hidden = pre.shape[1]
    if dout.dtype != torch.float32 or not dout.is_contiguous() or pre.dtype != torch.bfloat16 or not pre.is_contiguous() or pre.shape[0] != rows:
        raise RuntimeError("ffn_bwd_fused: dout must be contiguous fp32 (rows, 256), pre contiguous bf16 (rows, hidden)")
    if w2t.shape != (hidden, d) or w1t.shape != (d, hidden):
        raise RuntimeError("ffn_bwd_fused: packed weight shapes do not match")
    dev = dout.device
    take = _bufs(bufs, ("da2", "da1", "act", "dh", "db1", "workspace"), "ffn_bwd_fused")
    da2 = take("da2", (rows, d), torch.bfloat16, dev)
    dh = take("dh", (rows, d), torch.bfloat16, dev)
    da1 = take("da1", (rows, hidden), torch.bfloat16, dev)
    act = take("act", (rows, hidden), torch.bfloat16, dev)
    nws = int(N.lib().cm_ffn_bwd_workspace_floats(rows, hidden))
    if bufs is None:
        ws = torch.empty((nws + hidden + d,), dtype=torch.float32, device=dev)
        db1, db2 = ws[nws:nws + hidden], ws[nws + hidden:]
    else:
        ws, db = take("workspace", (nws,), torch.float32, dev), take("db1", (hidden + d,), torch.float32, dev)
        db1, db2 = db[:hidden], db[hidden:]
    a = N.FfnBwdArgs()
    a.rows, a.dim, a.hidden = rows, d, hidden
    a.dout, a.w2t, a.w1t, a.pre = _ptr(dout), _ptr(w2t.data), _ptr(w1t.data), _ptr(pre)
    a.da2, a.da1, a.act, a.dh, a.db1, a.db2 = _ptr(da2), _ptr(da1), _ptr(act), _ptr(dh), _ptr(db1), _ptr(db2)
    a.alpha, a.p1, a.p2, a.seed1, a.seed2 = float(alpha), float(p1), float(p2), int(seed1), int(seed2)
    a.seed_epoch = _seed_epoch_ptr()
    a.workspace, a.workspace_floats, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_ffn_bwd_fused", N.lib().cm_ffn_bwd_fused, a, units=rows)
    return da2, da1, act, dh, db1, db2


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev_check(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("mamba_asr_amd ops run on the GPU only (got a CPU tensor); there is no CPU fallback")


def _fresh(name, shape, dtype, device, rows3=False):
    return torch.empty(shape, dtype=dtype, device=device)


def _bufs(bufs, names, what):
    """-> take(name, shape, dtype, device): the caller-supplied buffer ``bufs[name]`` (a dict from the C struct's field name to a
    tensor; the guard-band tests place outputs and workspaces with it), validated as _out_rows does, or a fresh one.  None: every
    buffer is fresh.  ``rows3``: a (batch, seqlen, dim) buffer may be any view with the channel axis contiguous."""
    if bufs is None:
        return _fresh
    if not set(bufs) <= set(names):
        raise RuntimeError(f"{what}: bufs has no {sorted(set(bufs) - set(names))}; its names are {sorted(names)}")

    def take(name, shape, dtype, device, rows3=False):
        t = bufs.get(name)
        if t is not None and rows3:
            if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.stride(2) != 1 or t.device != device:
                raise RuntimeError(f"{what}: bufs[{name!r}] must be a {dtype} tensor of shape {tuple(shape)} on {device} with the channel axis contiguous")
            return t
        return _out_rows(t, shape, dtype, device, f"{what}: bufs[{name!r}]")
    return take


def _time_view(t, shape, dtype, device, what):
    """A caller-supplied (batch, dim, seqlen) output of the operator-route kernels: any view with the time axis contiguous (a half of
    xz, (dim, batch, seqlen) storage), or a fresh one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.stride(-1) != 1 or t.device != device:
        raise RuntimeError(f"{what} must be a {dtype} tensor of shape {tuple(shape)} on {device} with the time axis contiguous")
    return t


def _accum(bufs, name, shape, device, what):
    """A caller-placed fp32 reduction output is ACCUMULATED into (the C contract); a fresh one starts at zero."""
    if bufs is None or bufs.get(name) is None:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    return _out_rows(bufs[name], shape, torch.float32, device, f"{what}: bufs[{name!r}]")


def _time_contig(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    # same rule as the reference wrappers (selective_scan_interface.py:24-35): last dim must have stride 1
    if t is None:
        return None
    return t if t.stride(-1) == 1 else t.contiguous()


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.detach().to(torch.float32).contiguous()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    # the raw handle of the current stream: torch.cuda.current_stream() builds a Stream object per call (2.5 us x 220 launches per
    # forward; the training step is host-bound: 44.7 ms to enqueue 47 ms of kernels)
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def num_chunks(seqlen: int) -> int:
    return (seqlen + N.CM_SCAN_CHUNK - 1) // N.CM_SCAN_CHUNK


def _bc4(t: torch.Tensor) -> torch.Tensor:
    if t.dim() == 3:
        t = t.unsqueeze(1)
    if t.dim() != 4 or t.shape[1] != 1:
        raise RuntimeError("B/C must be (batch, dstate, seqlen) or (batch, 1, dstate, seqlen): one group only")
    return _time_contig(t)


def _fill_scan_args(a, u, delta, A, B, C_, D, z, delta_bias, delta_softplus, reverse):
    b, d, l = u.shape
    a.batch, a.dim, a.seqlen, a.dstate = b, d, l, A.shape[1]
    a.io_dtype, a.bc_dtype = _DT[u.dtype], _DT[B.dtype]
    a.delta_softplus, a.reverse_time = int(bool(delta_softplus)), int(bool(reverse))
    a.u, a.delta, a.A, a.B, a.C = _ptr(u), _ptr(delta), _ptr(A), _ptr(B), _ptr(C_)
    a.D, a.z, a.delta_bias = _ptr(D), _ptr(z), _ptr(delta_bias)
    a.u_bs, a.u_ds = u.stride(0), u.stride(1)
    a.delta_bs, a.delta_ds = delta.stride(0), delta.stride(1)
    if z is not None:
        a.z_bs, a.z_ds = z.stride(0), z.stride(1)
    a.B_bs, a.B_ns = B.stride(0), B.stride(2)
    a.C_bs, a.C_ns = C_.stride(0), C_.stride(2)
    a.stream = _stream()


def selective_scan_fwd(u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False,
                       reverse=False, need_out=True, need_x=True, out_z_buf: Optional[torch.Tensor] = None,
                       h0: Optional[torch.Tensor] = None, split: int = 0, bufs=None):
    """-> (out, x, out_z): what selective_scan_cuda.fwd returns (selective_scan_interface.py:42).
    ``out`` is the pre-gate output (None when z is given and need_out is False), ``x`` the
    checkpoint tensor (batch, dim, nchunks, 2*dstate) or None, ``out_z`` the gated output or None.
    ``h0`` (batch, dim, dstate) fp32: state the recurrence starts from (time-split scans, seqpar.py).
    ``split``: tuning, lanes per channel (cm_scan_fwd_args.lanes_per_channel; 0 = the library's choice).
    ``bufs``: caller-supplied ``out`` / ``out_z`` (time-contiguous (batch, dim, seqlen) views of u's dtype; the C contract gives both
    one pair of strides) and ``x`` (contiguous fp32); an output this call does not produce may not be placed."""
    _dev_check(u, delta, A, B, C, D, z, delta_bias)
    u, delta, z = _time_contig(u), _time_contig(delta), _time_contig(z)
    if delta.dtype != u.dtype or (z is not None and z.dtype != u.dtype):
        raise RuntimeError("u, delta and z must share one dtype")
    B, C = _bc4(B), _bc4(C)
    if B.dtype != C.dtype:
        raise RuntimeError("B and C must share one dtype")
    A, D, delta_bias = _f32c(A), _f32c(D), _f32c(delta_bias)
    b, d, l = u.shape
    a = N.ScanFwdArgs()
    _fill_scan_args(a, u, delta, A, B, C, D, z, delta_bias, delta_softplus, reverse)
    want_out = z is None or need_out
    if bufs is not None:
        what = "selective_scan_fwd"
        _bufs(bufs, ("out", "out_z", "x"), what)
        if out_z_buf is not None and bufs.get("out_z") is not None:
            raise RuntimeError(f"{what}: out_z_buf and bufs['out_z'] name the same output")
        for name, made in (("out", want_out), ("out_z", z is not None), ("x", need_x)):
            if bufs.get(name) is not None and not made:
                raise RuntimeError(f"{what}: bufs[{name!r}] places an output this call does not produce")
        out_z_buf = bufs.get("out_z") if out_z_buf is None else out_z_buf
    out = _time_view(None if bufs is None else bufs.get("out"), (b, d, l), u.dtype, u.device, "selective_scan_fwd: bufs['out']") if want_out else None
    out_z = None
    if z is not None:
        # out_z_buf: a pre-allocated time-contiguous (batch, dim, seqlen) view, e.g. of (dim, batch, seqlen) storage
        out_z = out_z_buf if out_z_buf is not None else torch.empty((b, d, l), dtype=u.dtype, device=u.device)
        if out_z.shape != (b, d, l) or out_z.stride(-1) != 1 or out_z.dtype != u.dtype:
            raise RuntimeError("out_z_buf must be a time-contiguous (batch, dim, seqlen) tensor of u's dtype")
    xshape = (b, d, num_chunks(l), 2 * A.shape[1])
    x = _out_rows(None if bufs is None else bufs.get("x"), xshape, torch.float32, u.device, "selective_scan_fwd: bufs['x']") if need_x else None
    a.out, a.out_z, a.x = _ptr(out), _ptr(out_z), _ptr(x)
    if h0 is not None:
        _dev_check(h0)
        if tuple(h0.shape) != (b, d, A.shape[1]):
            raise RuntimeError(f"h0 must be (batch, dim, dstate) = {(b, d, A.shape[1])}, got {tuple(h0.shape)}")
        h0 = _f32c(h0)
        a.h0 = _ptr(h0)
    if out is not None:
        a.out_bs, a.out_ds = out.stride(0), out.stride(1)
    a.lanes_per_channel = int(split)
    if out_z is not None:
        if out is not None and (out_z.stride(0), out_z.stride(1)) != (out.stride(0), out.stride(1)):
            raise RuntimeError("out and a strided out_z_buf cannot be requested together (they share strides)")
        a.out_bs, a.out_ds = out_z.stride(0), out_z.stride(1)
    _launch("cm_selective_scan_fwd", N.lib().cm_selective_scan_fwd, a, units=b * l)
    return out, x, out_z


def selective_scan_bwd(u, delta, A, B, C, D, z, delta_bias, dout, x, delta_softplus=False, reverse=False,
                       dz: Optional[torch.Tensor] = None, recompute_out_z=False, du_buf: Optional[torch.Tensor] = None,
                       ddelta_buf: Optional[torch.Tensor] = None, out_z_buf: Optional[torch.Tensor] = None, split: int = 0, bufs=None):
    """-> (du, ddelta, dA, dB, dC, dD, ddelta_bias, dz, out_z): the tuple selective_scan_cuda.bwd
    returns (selective_scan_interface.py:67, 252).  ``dz`` may be a pre-allocated view (e.g. half of
    dxz, :249-256).  dB/dC are fp32 (batch, 1, dstate, seqlen).
    ``bufs``: caller-supplied ``du`` / ``ddelta`` / ``dz`` / ``out_z`` (time-contiguous views, as the *_buf keywords they stand for),
    ``dA`` / ``dB`` / ``dC`` / ``dD`` / ``ddelta_bias`` (contiguous fp32, ACCUMULATED into, not zeroed) and ``workspace``
    (cm_selective_scan_bwd_workspace_bytes / 4 floats; the deterministic path only)."""
    if bufs is not None:
        what = "selective_scan_bwd"
        _bufs(bufs, ("du", "ddelta", "dz", "out_z", "dA", "dB", "dC", "dD", "ddelta_bias", "workspace"), what)
        for name, kw in (("du", du_buf), ("ddelta", ddelta_buf), ("dz", dz), ("out_z", out_z_buf)):
            if kw is not None and bufs.get(name) is not None:
                raise RuntimeError(f"{what}: bufs[{name!r}] and the keyword name the same output")
        for name, made in (("dz", z is not None), ("out_z", z is not None and recompute_out_z), ("dD", D is not None),
                           ("ddelta_bias", delta_bias is not None), ("workspace", DETERMINISTIC)):
            if bufs.get(name) is not None and not made:
                raise RuntimeError(f"{what}: bufs[{name!r}] places a buffer this call does not use")
        placed = lambda name, kw: kw if bufs.get(name) is None else bufs[name]
        du_buf, ddelta_buf, dz, out_z_buf = placed("du", du_buf), placed("ddelta", ddelta_buf), placed("dz", dz), placed("out_z", out_z_buf)
        if dz is not None and (tuple(dz.shape) != tuple(u.shape) or dz.dtype != u.dtype):
            raise RuntimeError(f"{what}: bufs['dz'] must be a time-contiguous (batch, dim, seqlen) tensor of u's dtype")
    _dev_check(u, delta, A, B, C, D, z, delta_bias, dout, x)
    u, delta, z, dout = _time_contig(u), _time_contig(delta), _time_contig(z), _time_contig(dout)
    B, C = _bc4(B), _bc4(C)
    A, D, delta_bias = _f32c(A), _f32c(D), _f32c(delta_bias)
    b, d, l = u.shape
    n = A.shape[1]
    a = N.ScanBwdArgs()
    _fill_scan_args(a.fwd, u, delta, A, B, C, D, z, delta_bias, delta_softplus, reverse)
    if x is None:
        raise RuntimeError("selective_scan_bwd needs the forward's checkpoint tensor x")
    a.fwd.x = _ptr(x)
    a.fwd.lanes_per_channel = int(split)
    out_z = None
    def _buf(t, what):                       # optional pre-allocated time-contiguous (batch, dim, seqlen) views
        if t is None:
            return torch.empty((b, d, l), dtype=u.dtype, device=u.device)
        if t.shape != (b, d, l) or t.stride(-1) != 1 or t.dtype != u.dtype:
            raise RuntimeError(f"{what} must be a time-contiguous (batch, dim, seqlen) tensor of u's dtype")
        return t
    if z is not None and recompute_out_z:
        out_z = _buf(out_z_buf, "out_z_buf")
        a.fwd.out_z, a.fwd.out_bs, a.fwd.out_ds = _ptr(out_z), out_z.stride(0), out_z.stride(1)
    dev = u.device
    du = _buf(du_buf, "du_buf")
    ddelta = _buf(ddelta_buf, "ddelta_buf")
    if z is not None and dz is None:
        dz = torch.empty((b, d, l), dtype=u.dtype, device=dev)
    if z is not None and dz.stride(-1) != 1:
        raise RuntimeError("dz must be time-contiguous")
    dA = _accum(bufs, "dA", (d, n), dev, "selective_scan_bwd")
    dB = _accum(bufs, "dB", (b, 1, n, l), dev, "selective_scan_bwd")
    dC = _accum(bufs, "dC", (b, 1, n, l), dev, "selective_scan_bwd")
    dD = _accum(bufs, "dD", (d,), dev, "selective_scan_bwd") if D is not None else None
    dbias = _accum(bufs, "ddelta_bias", (d,), dev, "selective_scan_bwd") if delta_bias is not None else None
    a.dout, a.dout_bs, a.dout_ds = _ptr(dout), dout.stride(0), dout.stride(1)
    a.du, a.ddelta, a.dz = _ptr(du), _ptr(ddelta), _ptr(dz if z is not None else None)
    a.du_bs, a.du_ds, a.ddelta_bs, a.ddelta_ds = du.stride(0), du.stride(1), ddelta.stride(0), ddelta.stride(1)
    if z is not None:
        a.dz_bs, a.dz_ds = dz.stride(0), dz.stride(1)
    a.dA, a.dB, a.dC, a.dD, a.ddelta_bias = _ptr(dA), _ptr(dB), _ptr(dC), _ptr(dD), _ptr(dbias)
    if DETERMINISTIC:
        nbytes = int(N.lib().cm_selective_scan_bwd_workspace_bytes(ct.byref(a)))
        if bufs is not None and bufs.get("workspace") is not None:
            ws = _out_rows(bufs["workspace"], (nbytes // 4,), torch.float32, dev, "selective_scan_bwd: bufs['workspace']")
        else:
            ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)      # caching allocator: 16-byte aligned
        a.workspace, a.workspace_bytes = _ptr(ws), nbytes
    _launch("cm_selective_scan_bwd", N.lib().cm_selective_scan_bwd, a, units=b * l)
    return du, ddelta, dA, dB, dC, dD, dbias, (dz if z is not None else None), out_z


def causal_conv1d_fwd(x, weight, bias=None, silu=True, reverse=False, out: Optional[torch.Tensor] = None, bufs=None):
    """x (batch, dim, seqlen), weight (dim, width) -> y.  causal_conv1d_cuda.causal_conv1d_fwd
    (selective_scan_interface.py:182) with seq_idx=None.
    ``bufs``: caller-supplied ``y`` (a time-contiguous (batch, dim, seqlen) view of x's dtype; what ``out`` stands for)."""
    _dev_check(x, weight, bias)
    x = _time_contig(x)
    w, bs = _f32c(weight), _f32c(bias)
    b, d, l = x.shape
    if bufs is not None:
        _bufs(bufs, ("y",), "causal_conv1d_fwd")
        if out is not None and bufs.get("y") is not None:
            raise RuntimeError("causal_conv1d_fwd: bufs['y'] and out name the same output")
        out = _time_view(out if bufs.get("y") is None else bufs["y"], (b, d, l), x.dtype, x.device, "causal_conv1d_fwd: bufs['y']")
    y = out if out is not None else torch.empty((b, d, l), dtype=x.dtype, device=x.device)
    a = N.ConvArgs()
    a.batch, a.dim, a.seqlen, a.width = b, d, l, w.shape[1]
    a.io_dtype, a.silu, a.reverse_time = _DT[x.dtype], int(bool(silu)), int(bool(reverse))
    a.x, a.weight, a.bias, a.y = _ptr(x), _ptr(w), _ptr(bs), _ptr(y)
    a.x_bs, a.x_ds, a.y_bs, a.y_ds = x.stride(0), x.stride(1), y.stride(0), y.stride(1)
    a.stream = _stream()
    _launch("cm_causal_conv1d_fwd", N.lib().cm_causal_conv1d_fwd, a, units=b * l)
    return y


def causal_conv1d_bwd(x, weight, bias, dy, silu=True, reverse=False, dx: Optional[torch.Tensor] = None, bufs=None):
    """-> (dx, dweight (dim, width) fp32, dbias (dim) fp32 or None); dx may be a pre-allocated view
    (selective_scan_interface.py:286-288).
    ``bufs``: caller-supplied ``dx`` (a time-contiguous view, what the keyword stands for), ``dweight`` / ``dbias`` (contiguous fp32,
    ACCUMULATED into, not zeroed) and ``workspace`` (batch * dim * (width + 1) floats; the deterministic path only)."""
    _dev_check(x, weight, bias, dy, dx)
    x, dy = _time_contig(x), _time_contig(dy)
    w, bs = _f32c(weight), _f32c(bias)
    b, d, l = x.shape
    if bufs is not None:
        what = "causal_conv1d_bwd"
        _bufs(bufs, ("dx", "dweight", "dbias", "workspace"), what)
        if dx is not None and bufs.get("dx") is not None:
            raise RuntimeError(f"{what}: bufs['dx'] and dx name the same output")
        for name, made in (("dbias", bias is not None), ("workspace", DETERMINISTIC)):
            if bufs.get(name) is not None and not made:
                raise RuntimeError(f"{what}: bufs[{name!r}] places a buffer this call does not use")
        dx = _time_view(dx if bufs.get("dx") is None else bufs["dx"], (b, d, l), x.dtype, x.device, f"{what}: bufs['dx']")
    if dx is None:
        dx = torch.empty((b, d, l), dtype=x.dtype, device=x.device)
    if dx.stride(-1) != 1:
        raise RuntimeError("dx must be time-contiguous")
    dw = _accum(bufs, "dweight", tuple(w.shape), x.device, "causal_conv1d_bwd")
    db = _accum(bufs, "dbias", (d,), x.device, "causal_conv1d_bwd") if bias is not None else None
    a = N.ConvArgs()
    a.batch, a.dim, a.seqlen, a.width = b, d, l, w.shape[1]
    a.io_dtype, a.silu, a.reverse_time = _DT[x.dtype], int(bool(silu)), int(bool(reverse))
    a.x, a.weight, a.bias = _ptr(x), _ptr(w), _ptr(bs)
    a.x_bs, a.x_ds = x.stride(0), x.stride(1)
    a.dy, a.dx, a.dweight, a.dbias = _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db)
    a.dy_bs, a.dy_ds, a.dx_bs, a.dx_ds = dy.stride(0), dy.stride(1), dx.stride(0), dx.stride(1)
    a.stream = _stream()
    if DETERMINISTIC:
        ws = _out_rows(None if bufs is None else bufs.get("workspace"), (b * d * (w.shape[1] + 1),), torch.float32, x.device,
                       "causal_conv1d_bwd: bufs['workspace']")
        a.workspace = _ptr(ws)
    _launch("cm_causal_conv1d_bwd", N.lib().cm_causal_conv1d_bwd, a, units=b * l)
    return dx, dw, db


# ------------------------------------------------------------------------------------------
# channels-last ops (the fused BiMamba path)
# ------------------------------------------------------------------------------------------
def _rows_ok(t: torch.Tensor, what: str):
    if t.dim() != 3 or t.stride(2) != 1:
        raise RuntimeError(f"{what} must be (batch, seqlen, dim) with the channel axis contiguous")


def alloc_bc(nrows: int, batch: int, seqlen: int, device) -> torch.Tensor:
    """(nrows, batch, seqlen) fp32 buffer whose storage is readable 16 steps past the end, as
    cm_scan_cl_fwd requires of B/C (scalar loads fetch whole 16-step groups)."""
    n = nrows * batch * seqlen
    flat = torch.empty(n + 16, dtype=torch.float32, device=device)
    flat[n:].zero_()                                     # the readable tail must be finite
    return flat[:n].view(nrows, batch, seqlen)


def rows_dt_pad(dt_rank: int) -> int:
    """Width the dt features are zero-padded to in the x_dbl rows of cm_scan_cl_fwd's xdbl mode: 16, or 32 (bf16 only)."""
    if not 1 <= dt_rank <= 32:
        raise RuntimeError(f"the xdbl mode of cm_scan_cl_fwd needs 1 <= dt_rank <= 32 (got {dt_rank})")
    return 16 if dt_rank <= 16 else 32


def pad_dt_weight(dt_weight: torch.Tensor) -> torch.Tensor:
    """(dim, dt_rank <= 32) -> (dim, 16 | 32) fp32, zero padded: the dt_weight layout of cm_scan_cl_fwd's xdbl mode."""
    d, r = dt_weight.shape
    out = torch.zeros((d, rows_dt_pad(r)), dtype=torch.float32, device=dt_weight.device)
    out[:, :r] = dt_weight.detach().float()
    return out


def xproj_rows(x_weight: torch.Tensor, dt_rank: int, pad: int, dtype: torch.dtype) -> torch.Tensor:
    """x_proj's weight (dt_rank + 32, E) -> (pad + 32, E) in ``dtype``, rows [dt (zero padded to ``pad``) | B (16) | C (16)]: a GEMM with
    it writes the x_dbl rows as cm_scan_cl_fwd's xdbl mode reads them."""
    return xproj_rows_(torch.zeros(pad + 32, x_weight.shape[1], dtype=dtype, device=x_weight.device), x_weight, dt_rank, pad)


def xproj_rows_(out: torch.Tensor, x_weight: torch.Tensor, dt_rank: int, pad: int) -> torch.Tensor:
    """xproj_rows into an image that exists (its padding rows are zero already)."""
    out[:dt_rank].copy_(x_weight.detach()[:dt_rank])
    out[pad:].copy_(x_weight.detach()[dt_rank:])
    return out


def _scan_cl_dir_rows(x, dd, u0, z, keep):
    """One direction descriptor in xdbl mode: x_dbl rows (batch, seqlen, P + 32) = [dt P | B16 | C16] in the I/O dtype,
    P = 16, or 32 (bf16 only) for 16 < dt_rank <= 32."""
    u, xdbl, dt_w = dd["u"], dd["xdbl"], dd["dt_weight"]
    _dev_check(u, xdbl, dt_w, dd["A"])
    _rows_ok(u, "u")
    _rows_ok(xdbl, "xdbl")
    b, l, d = u0.shape
    pad = xdbl.shape[-1] - 32
    if pad not in (16, 32) or (pad == 32 and u0.dtype != torch.bfloat16):
        raise RuntimeError("xdbl mode: xdbl rows are 48 wide, or 64 wide (dt_rank > 16) in bf16")
    if u.shape != (b, l, d) or xdbl.shape != (b, l, pad + 32) or u.dtype != u0.dtype or xdbl.dtype != u0.dtype:
        raise RuntimeError("xdbl mode: u (batch, seqlen, dim) and xdbl (batch, seqlen, 48 | 64) must share shape prefix and dtype")
    if dt_w.shape != (d, pad):
        raise RuntimeError(f"xdbl mode: dt_weight must be (dim, {pad}), zero padded (ops.pad_dt_weight)")
    A, D, bias, dt_w = _f32c(dd["A"]), _f32c(dd.get("D")), _f32c(dd.get("delta_bias")), _f32c(dt_w)
    out = dd.get("out")
    if out is None:
        out = torch.empty((b, l, d), dtype=u.dtype, device=u.device)
    _rows_ok(out, "out")
    keep += [A, D, bias, dt_w]
    x.u, x.A, x.D, x.delta_bias, x.out, x.dt_weight, x.xdbl = _ptr(u), _ptr(A), _ptr(D), _ptr(bias), _ptr(out), _ptr(dt_w), _ptr(xdbl)
    x.u_bs, x.u_ts, x.out_bs, x.out_ts = u.stride(0), u.stride(1), out.stride(0), out.stride(1)
    x.xdbl_bs, x.xdbl_ts, x.dt_rank = xdbl.stride(0), xdbl.stride(1), pad
    x.reverse_time = int(bool(dd.get("reverse", False)))
    ck, yp = dd.get("ckpt"), dd.get("ypre")                  # what the training forward saves for scan_cl_bwd
    if ck is not None:
        _dev_check(ck)
        if ck.dtype != torch.float32 or not ck.is_contiguous() or tuple(ck.shape) != (b, 2 * ((l + 15) // 16), d, 16):
            raise RuntimeError("xdbl mode: ckpt must be a contiguous fp32 (batch, 2 * ceil(seqlen / 16), dim, 16) tensor")
        keep.append(ck)
        x.ckpt = _ptr(ck)
    if yp is not None:
        _dev_check(yp)
        _rows_ok(yp, "ypre")
        if yp.shape != (b, l, d) or yp.dtype != u0.dtype:
            raise RuntimeError("xdbl mode: ypre must be (batch, seqlen, dim) in the I/O dtype")
        keep.append(yp)
        x.ypre, x.ypre_bs, x.ypre_ts = _ptr(yp), yp.stride(0), yp.stride(1)
    for key in ("h0", "h_last", "decay"):                    # carry interface of the time-split scan: (batch, dim, 16) fp32
        t = dd.get(key)
        if t is not None:
            _dev_check(t)
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (b, d, 16):
                raise RuntimeError(f"xdbl mode: {key} must be a contiguous fp32 (batch, dim, 16) tensor")
            keep.append(t)
            setattr(x, key, _ptr(t))
    return out


# time chunks of cm_scan_cl_fwd's xdbl mode: "auto" (cm_scan_cl_fwd_auto_chunks: cut sequences when the batch is too small
# to fill the chip), or a fixed count (1 = never)
SCAN_CHUNKS = os.environ.get("CM_SCAN_CHUNKS", "auto")


def scan_chunks_policy(batch: int, seqlen: int, dim: int, ndir: int, lens=None) -> int:
    """The chunk count scan_cl_fwd picks for an xdbl-mode launch that names none: 1 under ``lens``, else CM_SCAN_CHUNKS."""
    if lens is not None:
        return 1
    return N.lib().cm_scan_cl_fwd_auto_chunks(batch, seqlen, dim, ndir) if SCAN_CHUNKS == "auto" else int(SCAN_CHUNKS)


def scan_cl_fwd(directions, z=None, delta_softplus=True, time_chunks=None, split: int = 0, lens=None, whole: bool = False, fold: bool = False,
                workspace=None):
    """Channels-last selective scan, 1 or 2 directions in one launch (cm_scan_cl_fwd).
    ``time_chunks`` (xdbl mode): None = the CM_SCAN_CHUNKS policy, else the chunk count.
    ``lens`` (cm_scan_cl_fwd_slots; xdbl mode, one direction, unchunked): int32 (batch,) device tensor, sequence b runs its first
    lens[b] steps only (h_last = h0 for 0); ``out`` rows at and past lens[b] are not written.  With two directions, or
    ``whole=True`` (cm_scan_cl_fwd_lens; xdbl mode, unchunked, no carried state): sequence b is a whole utterance of lens[b] steps --
    the reverse direction starts from a zero state at step lens[b] - 1.
    ``fold`` (cm_scan_cl_fwd_fold / _fold_lens; xdbl mode, two directions of opposite time, z, softplus, bf16, dt_rank <= 16, unchunked):
    the gated SUM of both directions goes into directions[0]["out"] (batch, seqlen, dim) -- directions[1]["out"] must be absent or that
    tensor -- and [out] is returned; ``workspace``: a caller-owned contiguous tensor of at least cm_scan_cl_fwd_fold_workspace_bytes
    bytes, 16-byte aligned (allocated here otherwise).  Logged as the unfolded launch is (cm_scan_cl_fwd, or cm_scan_cl_fwd_lens with lengths).

    ``directions``: list of dicts with u, delta (batch, seqlen, dim), A (dim, 16), B, C (16, batch, seqlen) fp32
    time-contiguous (see alloc_bc), D, delta_bias (dim) or None, out (batch, seqlen, dim) view or None, reverse.
    Returns the list of out tensors."""
    if not 1 <= len(directions) <= 2:
        raise RuntimeError("1 or 2 directions")
    u0 = directions[0]["u"]
    _dev_check(u0, z)
    _rows_ok(u0, "u")
    b, l, d = u0.shape
    a = N.ScanClArgs()
    a.batch, a.seqlen, a.dim, a.dstate = b, l, d, 16
    a.io_dtype, a.delta_softplus, a.ndir = _DT[u0.dtype], int(bool(delta_softplus)), len(directions)
    keep = []
    if z is not None:
        _rows_ok(z, "z")
        a.z, a.z_bs, a.z_ts = _ptr(z), z.stride(0), z.stride(1)
    outs = []
    if fold:
        if len(directions) != 2 or any(dd.get("xdbl") is None for dd in directions):
            raise RuntimeError("fold needs two directions in xdbl mode")
        if directions[1].get("out") is not None and directions[1]["out"] is not directions[0].get("out"):
            raise RuntimeError("fold writes one tensor: directions[1]['out'] must be absent or directions[0]['out']")
    for i, dd in enumerate(directions):
        if fold and i == 1:
            dd = dict(dd, out=outs[0])
        if dd.get("xdbl") is not None:
            outs.append(_scan_cl_dir_rows(a.dir[i], dd, u0, z, keep))
            continue
        u, delta = dd["u"], dd.get("delta")
        dt_low, dt_w = dd.get("dt_low"), dd.get("dt_weight")
        _dev_check(u, delta, dd["A"], dd["B"], dd["C"], dt_low, dt_w)
        _rows_ok(u, "u")
        if delta is not None:
            _rows_ok(delta, "delta")
        elif dt_low is None:
            raise RuntimeError("either delta or (dt_low, dt_weight) is required")
        if u.dtype != u0.dtype or (delta is not None and delta.dtype != u0.dtype) or (z is not None and z.dtype != u0.dtype):
            raise RuntimeError("u, delta, z must share one dtype")
        Bm, Cm = dd["B"], dd["C"]
        if Bm.dtype != torch.float32 or Bm.stride(2) != 1 or Bm.stride() != Cm.stride() or Bm.shape != (16, b, l):
            raise RuntimeError("B/C must be fp32 (16, batch, seqlen), time-contiguous, with equal strides")
        A, D, bias = _f32c(dd["A"]), _f32c(dd.get("D")), _f32c(dd.get("delta_bias"))
        dt_w = _f32c(dt_w)
        if dt_low is not None:
            if dt_low.dtype != torch.float32 or dt_low.stride(2) != 1 or dt_low.stride()[:2] != Bm.stride()[:2]:
                raise RuntimeError("dt_low must be fp32 (dt_rank, batch, seqlen) with the strides of B/C")
        out = dd.get("out")
        if out is None:
            out = torch.empty((b, l, d), dtype=u.dtype, device=u.device)
        _rows_ok(out, "out")
        keep += [A, D, bias, dt_w]
        x = a.dir[i]
        x.u, x.delta, x.A, x.B, x.C, x.D, x.delta_bias, x.out = (_ptr(u), _ptr(delta), _ptr(A), _ptr(Bm), _ptr(Cm),
                                                                   _ptr(D), _ptr(bias), _ptr(out))
        x.dt_low, x.dt_weight, x.dt_rank = _ptr(dt_low), _ptr(dt_w), (0 if dt_low is None else dt_low.shape[0])
        x.u_bs, x.u_ts = u.stride(0), u.stride(1)
        if delta is not None:
            x.delta_bs, x.delta_ts = delta.stride(0), delta.stride(1)
        x.out_bs, x.out_ts = out.stride(0), out.stride(1)
        x.bc_ns, x.bc_bs = Bm.stride(0), Bm.stride(1)
        x.reverse_time = int(bool(dd.get("reverse", False)))
        outs.append(out)
    a.stream = _stream()
    a.lanes_per_channel = int(split)                     # tuning of the state-split kernel: 4, 8, 16 lanes per channel; 0 = automatic
    if "xdbl" in directions[0]:
        if time_chunks is None:
            time_chunks = scan_chunks_policy(b, l, d, len(directions), lens)
        a.time_chunks = int(time_chunks)
        nbytes = N.lib().cm_scan_cl_fwd_workspace_bytes(ct.byref(a))
        if nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=u0.device)
            keep.append(ws)
            a.workspace, a.workspace_bytes = _ptr(ws), nbytes
    elif time_chunks not in (None, 0, 1):
        raise RuntimeError("time_chunks needs the xdbl mode")
    if fold:
        if a.time_chunks > 1:
            raise RuntimeError(f"fold: the unchunked launch only (time_chunks {a.time_chunks}); the caller asks the chunk policy first")
        nbytes = N.lib().cm_scan_cl_fwd_fold_workspace_bytes(ct.byref(a))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=u0.device) if workspace is None else workspace
        _dev_check(ws)
        if not ws.is_contiguous() or ws.numel() * ws.element_size() < nbytes:
            raise RuntimeError(f"fold: workspace must be a contiguous tensor of at least {nbytes} bytes")
        keep.append(ws)
        a.workspace, a.workspace_bytes = _ptr(ws), ws.numel() * ws.element_size()
        if lens is not None:
            lp, fn = _slot_lens(lens, b, u0.device, "scan_cl_fwd"), N.lib().cm_scan_cl_fwd_fold_lens
            _launch("cm_scan_cl_fwd_lens", lambda ref: fn(ref, lp), a, units=b * l * 2)
        else:
            _launch("cm_scan_cl_fwd", N.lib().cm_scan_cl_fwd_fold, a, units=b * l * 2)
        return outs[:1]
    if lens is not None and (whole or len(directions) == 2):
        lp, fn = _slot_lens(lens, b, u0.device, "scan_cl_fwd"), N.lib().cm_scan_cl_fwd_lens
        _launch("cm_scan_cl_fwd_lens", lambda ref: fn(ref, lp), a, units=b * l * len(directions))
        return outs
    if lens is not None:
        lp, fn = _slot_lens(lens, b, u0.device, "scan_cl_fwd"), N.lib().cm_scan_cl_fwd_slots
        _launch("cm_scan_cl_fwd_slots", lambda ref: fn(ref, lp), a, units=b * l)
        return outs
    _launch("cm_scan_cl_fwd", N.lib().cm_scan_cl_fwd, a, units=b * l * len(directions))
    return outs


def _elem_args(rows, dim, io_dtype, act, p, alpha):
    a = N.FfnElemArgs()
    a.rows, a.dim, a.io_dtype, a.act, a.p, a.alpha, a.stream = rows, dim, _DT[io_dtype], int(act), float(p), float(alpha), _stream()
    a.seed_epoch = _seed_epoch_ptr()
    return a


def draw_seed() -> int:
    """64-bit seed for a dropout mask from torch's (seedable) CPU generator: no device synchronisation."""
    return int(torch.randint(0, 2 ** 62, (1,)).item())


# Dropout under hipGraph replay.  A seed drawn on the host is a constant of the captured launch; with SEED_EPOCH set to a
# one-element int64 DEVICE tensor every dropout kernel adds  *SEED_EPOCH * CM_SEED_EPOCH_MUL  to its seed when it runs
# (cm_ffn_elem_args.seed_epoch), so a graph whose first node increments the word draws new decisions per replay while the
# forward and backward kernels of one replay still agree.  None (default): the host seed alone.  graphs.GraphedTrainStep sets it.
SEED_EPOCH = None
SEED_EPOCH_MUL = N.CM_SEED_EPOCH_MUL


def _seed_epoch_ptr():
    t = SEED_EPOCH
    if t is None:
        return None
    if not (t.is_cuda and t.dtype == torch.int64 and t.numel() == 1):
        raise RuntimeError("ops.SEED_EPOCH must be a one-element int64 device tensor")
    return _ptr(t)


def effective_seed(seed: int, epoch: int) -> int:
    """The seed a kernel uses when the device word holds ``epoch`` (for tests and for reproducing a replay eagerly)."""
    return (int(seed) + int(epoch) * SEED_EPOCH_MUL) & (2 ** 64 - 1)


def bias_act_dropout_fwd(a, bias, act=0, p=0.0, res=None, alpha=1.0, seed=None, store_mask=True, bufs=None):
    """y = dropout(act(a + bias)) in a's dtype, or with ``res`` (fp32, a's shape) y = res + alpha * dropout(a + bias) in fp32
    (cm_bias_act_dropout_fwd).  a (rows, dim) contiguous bf16 / fp32; act 0 none, 1 GELU.  -> (y, mask or None).
    The keep decisions are a function of (seed, element index) (csrc/cm_dropout.h): with ``seed`` given (draw_seed()) and
    ``store_mask=False`` no mask is written and bias_act_dropout_bwd re-derives it from the same seed.  ``bufs``: caller-supplied ``y`` and ``mask``."""
    _dev_check(a, bias, res)
    if a.dim() != 2 or not a.is_contiguous() or a.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError("bias_act_dropout_fwd: a must be a contiguous (rows, dim) bf16 / fp32 tensor")
    rows, dim = a.shape
    args = _elem_args(rows, dim, a.dtype, act, p, alpha)
    bs = _f32c(bias)
    take = _bufs(bufs, ("y", "mask"), "bias_act_dropout_fwd")
    mask = take("mask", (rows, dim), torch.uint8, a.device) if (p > 0.0 and store_mask) else None
    if res is not None and (res.dtype != torch.float32 or not res.is_contiguous() or res.shape != a.shape):
        raise RuntimeError("bias_act_dropout_fwd: res must be a contiguous fp32 tensor of a's shape")
    y = take("y", (rows, dim), torch.float32 if res is not None else a.dtype, a.device)
    args.a, args.bias, args.res, args.y, args.mask = _ptr(a), _ptr(bs), _ptr(res), _ptr(y), _ptr(mask)
    if p > 0.0:
        args.seed = draw_seed() if seed is None else int(seed)
    _launch("cm_bias_act_dropout_fwd", N.lib().cm_bias_act_dropout_fwd, args, units=rows)
    return y, mask


def bias_act_dropout_bwd(dy, mask, p, a=None, bias=None, act=0, alpha=1.0, out_dtype=None, want_dbias=True, seed=None, want_act=False,
                         bufs=None):
    """da = alpha * dy * mask / (1 - p) * act'(a + bias) in ``out_dtype`` (default a's / dy's dtype); dbias = column sums of da
    (fp32, deterministic) (cm_bias_act_dropout_bwd).  dy (rows, dim) fp32 or the I/O dtype.  -> (da, dbias or None).
    ``mask`` None with ``seed`` given: the decisions are re-derived from the seed.  ``want_act`` (act 1, bf16): also returns
    dropout(GELU(a + bias)) recomputed, as cm_ffn_fused's training forward fed it to its second GEMM -> (da, dbias, act).
    ``bufs``: caller-supplied ``da``, ``act_out``, ``dbias`` and ``dbias_part`` (cm_bias_act_dropout_bwd_workspace_floats)."""
    _dev_check(dy, mask, a, bias)
    if dy.dim() != 2 or not dy.is_contiguous():
        raise RuntimeError("bias_act_dropout_bwd: dy must be a contiguous (rows, dim) tensor")
    rows, dim = dy.shape
    io = out_dtype or (a.dtype if a is not None else dy.dtype)
    if io not in (torch.float32, torch.bfloat16) or dy.dtype not in (torch.float32, io):
        raise RuntimeError("bias_act_dropout_bwd: dtypes must be fp32 / bf16, dy fp32 or the I/O dtype")
    if a is not None and (a.dtype != io or not a.is_contiguous() or a.shape != dy.shape):
        raise RuntimeError("bias_act_dropout_bwd: a must be contiguous, of dy's shape, in the I/O dtype")
    args = _elem_args(rows, dim, io, act, p if (mask is not None or seed is not None) else 0.0, alpha)
    if seed is not None:
        args.seed = int(seed)
    bs = _f32c(bias)
    take = _bufs(bufs, ("da", "act_out", "dbias", "dbias_part"), "bias_act_dropout_bwd")
    da = take("da", (rows, dim), io, dy.device)
    act_out = None
    if want_act:
        act_out = take("act_out", (rows, dim), io, dy.device)
        args.act_out = _ptr(act_out)
    args.a, args.bias, args.mask, args.dy, args.da = _ptr(a), _ptr(bs), _ptr(mask), _ptr(dy), _ptr(da)
    args.dy_f32 = int(dy.dtype == torch.float32 and io != torch.float32)
    dbias = None
    if want_dbias:
        nws = int(N.lib().cm_bias_act_dropout_bwd_workspace_floats(rows, dim))
        if bufs is None:
            ws = torch.empty((nws + dim,), dtype=torch.float32, device=dy.device)
            dbias = ws[nws:]
        else:
            ws, dbias = take("dbias_part", (nws,), torch.float32, dy.device), take("dbias", (dim,), torch.float32, dy.device)
        args.dbias, args.dbias_part, args.overwrite = _ptr(dbias), _ptr(ws), 1
    _launch("cm_bias_act_dropout_bwd", N.lib().cm_bias_act_dropout_bwd, args, units=rows)
    return (da, dbias, act_out) if want_act else (da, dbias)


def bias_glu_fwd(a, bias, bufs=None):
    """(rows, 2 dim) -> (rows, dim): (a[:, :dim] + b[:dim]) * sigmoid(a[:, dim:] + b[dim:])  (cm_bias_act_dropout_fwd, act 2)."""
    _dev_check(a, bias)
    rows, d2 = a.shape
    if not a.is_contiguous() or a.dtype not in (torch.float32, torch.bfloat16) or d2 % 16:
        raise RuntimeError("bias_glu_fwd: a must be a contiguous (rows, 2 dim) bf16 / fp32 tensor, dim a multiple of 8")
    args = _elem_args(rows, d2 // 2, a.dtype, 2, 0.0, 1.0)
    bs = _f32c(bias)
    y = _bufs(bufs, ("y",), "bias_glu_fwd")("y", (rows, d2 // 2), a.dtype, a.device)
    args.a, args.bias, args.y = _ptr(a), _ptr(bs), _ptr(y)
    _launch("cm_bias_act_dropout_fwd", N.lib().cm_bias_act_dropout_fwd, args, units=rows)
    return y


def bias_glu_bwd(dy, a, bias, bufs=None):
    """-> (da (rows, 2 dim) in a's dtype, dbias (2 dim) fp32) of bias_glu_fwd (cm_bias_act_dropout_bwd, act 2; deterministic)."""
    _dev_check(dy, a, bias)
    rows, d = dy.shape
    if not dy.is_contiguous() or dy.dtype != a.dtype or a.shape != (rows, 2 * d) or not a.is_contiguous():
        raise RuntimeError("bias_glu_bwd: dy (rows, dim) and a (rows, 2 dim) must be contiguous and share a dtype")
    args = _elem_args(rows, d, a.dtype, 2, 0.0, 1.0)
    bs = _f32c(bias)
    nws = int(N.lib().cm_bias_act_dropout_bwd_workspace_floats(rows, d))
    if bufs is None:
        da = torch.empty_like(a)
        ws = torch.empty((nws + 2 * d,), dtype=torch.float32, device=dy.device)
        dbias = ws[nws:]
    else:
        take = _bufs(bufs, ("da", "dbias", "dbias_part"), "bias_glu_bwd")
        da = take("da", a.shape, a.dtype, a.device)
        ws, dbias = take("dbias_part", (nws,), torch.float32, dy.device), take("dbias", (2 * d,), torch.float32, dy.device)
    args.overwrite = 1
    args.a, args.bias, args.dy, args.da, args.dbias, args.dbias_part = _ptr(a), _ptr(bs), _ptr(dy), _ptr(da), _ptr(dbias), _ptr(ws)
    _launch("cm_bias_act_dropout_bwd", N.lib().cm_bias_act_dropout_bwd, args, units=rows)
    return da, dbias


def ctc_supported(log_probs, targets) -> bool:
    return log_probs.is_cuda and log_probs.dim() == 3 and targets.dim() == 2 and targets.shape[1] <= 511 and log_probs.shape[2] > 1


def ctc_loss_grad(log_probs, targets, input_lengths, target_lengths, blank=0, bufs=None):
    """log_probs (batch, T, V) -> (nll (batch) fp32, grad (batch, T, V) fp32) (cm_ctc_loss): per-utterance negative log-likelihood
    (0 where no alignment exists) and its gradient w.r.t. log_probs; lengths are integer tensors.  targets (batch, 0) -- every
    target empty -- is passed as NULL (the library takes that exactly when S == 0).  bufs: caller-placed "nll", "grad" and
    "workspace" (fp32, cm_ctc_workspace_floats)."""
    _dev_check(log_probs, targets, input_lengths, target_lengths)
    lp = log_probs.detach().float().contiguous()
    b, t, v = lp.shape
    tg = targets.detach().to(torch.int64).contiguous()
    il, tl = input_lengths.detach().to(torch.int32).contiguous(), target_lengths.detach().to(torch.int32).contiguous()
    s = tg.shape[1]
    take = _bufs(bufs, ("nll", "grad", "workspace"), "ctc_loss_grad")
    nll = take("nll", (b,), torch.float32, lp.device)
    grad = take("grad", (b, t, v), torch.float32, lp.device)
    nws = int(N.lib().cm_ctc_workspace_floats(b, t, s))
    ws = take("workspace", (nws,), torch.float32, lp.device)
    a = N.CtcArgs()
    a.batch, a.T, a.V, a.S, a.blank = b, t, v, s, int(blank)
    a.log_probs, a.targets, a.input_lengths, a.target_lengths, a.nll, a.grad = _ptr(lp), _ptr(tg), _ptr(il), _ptr(tl), _ptr(nll), _ptr(grad)
    a.workspace, a.workspace_floats, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_ctc_loss", N.lib().cm_ctc_loss, a, units=b * t)
    return nll, grad


def ctc_align(log_probs, targets, input_lengths, target_lengths, blank=0, rows=None, bufs=None):
    """CTC forced alignment (cm_ctc_align; the contract is in mamba_asr_amd.ctc_decode's docstring).  log_probs (R, T, V) fp32 /
    bf16 passed with its strides (unit vocabulary stride; other dtypes are cast to fp32), targets (batch, S) integer labels padded,
    input_lengths / target_lengths (batch) integer tensors; rows (batch) or None: the log_probs row each utterance reads (None:
    its own, and R = batch), so several label sequences can share one utterance's frames.
    -> (score (batch) fp64, status (batch) int32, states (batch, T) int32, starts, ends (batch, S) int32, label_logp (batch, S)
    fp64).  bufs: caller-placed "score", "status", "states", "starts", "ends", "label_logp" and "workspace" (uint8,
    cm_ctc_align_workspace_bytes)."""
    _dev_check(log_probs, targets, input_lengths, target_lengths, rows)
    if log_probs.dim() != 3 or targets.dim() != 2:
        raise RuntimeError(f"ctc_align: log_probs must be (rows, T, V) and targets (batch, S), got {tuple(log_probs.shape)} and {tuple(targets.shape)}")
    if log_probs.dtype not in (torch.float32, torch.bfloat16):
        log_probs = log_probs.float()
    lp = log_probs.detach()
    if lp.stride(2) != 1:
        lp = lp.contiguous()
    r, t, v = lp.shape
    dev = lp.device
    tg = targets.detach().to(torch.int64).contiguous()
    b, s = tg.shape
    il, tl = input_lengths.detach().to(torch.int32).contiguous(), target_lengths.detach().to(torch.int32).contiguous()
    rw = None if rows is None else rows.detach().to(torch.int32).contiguous()
    if il.numel() != b or tl.numel() != b or (rw is not None and rw.numel() != b) or (rw is None and r != b):
        raise RuntimeError(f"ctc_align: {b} target rows need {b} input_lengths, target_lengths and rows (or, without rows, {b} rows of log_probs)")
    take = _bufs(bufs, ("score", "status", "states", "starts", "ends", "label_logp", "workspace"), "ctc_align")
    score, status = take("score", (b,), torch.float64, dev), take("status", (b,), torch.int32, dev)
    states = take("states", (b, t), torch.int32, dev)
    starts, ends = take("starts", (b, s), torch.int32, dev), take("ends", (b, s), torch.int32, dev)
    label_logp = take("label_logp", (b, s), torch.float64, dev)
    a = N.CtcAlignArgs()
    a.batch, a.T, a.V, a.S, a.blank, a.dtype = b, t, v, s, int(blank), _DT[lp.dtype]
    a.lp_rows, a.lp_bs, a.lp_ts = r, lp.stride(0), lp.stride(1)
    a.log_probs, a.targets, a.input_lengths, a.target_lengths, a.rows = _ptr(lp), (_ptr(tg) if s else None), _ptr(il), _ptr(tl), _ptr(rw)
    a.score, a.status, a.states = _ptr(score), _ptr(status), _ptr(states)
    if s:
        a.starts, a.ends, a.label_logp = _ptr(starts), _ptr(ends), _ptr(label_logp)
    nws = int(N.lib().cm_ctc_align_workspace_bytes(ct.byref(a)))
    ws = take("workspace", (max(nws, 1),), torch.uint8, dev)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_ctc_align", N.lib().cm_ctc_align, a, units=b * t)
    return score, status, states, starts, ends, label_logp


def ctc_greedy(log_probs, input_lengths, blank=0, bufs=None):
    """Greedy CTC decode (cm_ctc_greedy; the contract is in mamba_asr_amd.ctc_decode's docstring).  log_probs (batch, T, V) fp32 /
    bf16 passed with its strides (unit vocabulary stride; other dtypes are cast to fp32), input_lengths (batch) integer tensor.
    -> (tokens (batch, T) int32, token_len (batch) int32, starts, ends (batch, T) int32, token_logp (batch, T) fp64, status (batch)
    int32).  bufs: caller-placed "tokens", "token_len", "starts", "ends", "token_logp", "status" and "workspace" (uint8,
    cm_ctc_greedy_workspace_bytes)."""
    _dev_check(log_probs, input_lengths)
    if log_probs.dim() != 3 or 0 in log_probs.shape:
        raise RuntimeError(f"ctc_greedy: log_probs must be a non-empty (batch, T, V) tensor, got {tuple(log_probs.shape)}")
    if log_probs.dtype not in (torch.float32, torch.bfloat16):
        log_probs = log_probs.float()
    lp = log_probs.detach()
    if lp.stride(2) != 1:
        lp = lp.contiguous()
    b, t, v = lp.shape
    dev = lp.device
    il = input_lengths.detach().to(torch.int32).contiguous()
    if il.numel() != b:
        raise RuntimeError(f"ctc_greedy: {b} rows of log_probs need {b} input_lengths, got {il.numel()}")
    take = _bufs(bufs, ("tokens", "token_len", "starts", "ends", "token_logp", "status", "workspace"), "ctc_greedy")
    tokens, token_len = take("tokens", (b, t), torch.int32, dev), take("token_len", (b,), torch.int32, dev)
    starts, ends = take("starts", (b, t), torch.int32, dev), take("ends", (b, t), torch.int32, dev)
    token_logp, status = take("token_logp", (b, t), torch.float64, dev), take("status", (b,), torch.int32, dev)
    a = N.CtcGreedyArgs()
    a.batch, a.T, a.V, a.blank, a.dtype = b, t, v, int(blank), _DT[lp.dtype]
    a.lp_bs, a.lp_ts = lp.stride(0), lp.stride(1)
    a.log_probs, a.input_lengths = _ptr(lp), _ptr(il)
    a.tokens, a.token_len, a.starts, a.ends, a.token_logp, a.status = _ptr(tokens), _ptr(token_len), _ptr(starts), _ptr(ends), _ptr(token_logp), _ptr(status)
    nws = int(N.lib().cm_ctc_greedy_workspace_bytes(ct.byref(a)))
    ws = take("workspace", (max(nws, 1),), torch.uint8, dev)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_ctc_greedy", N.lib().cm_ctc_greedy, a, units=b * t)
    return tokens, token_len, starts, ends, token_logp, status


def edit_distance(refs, ref_len, hyps, hyp_len, ref_index=None, want_ops=False, bufs=None):
    """Edit distance with alignment counts (cm_edit_distance; the contract is in mamba_asr_amd.metrics' docstring).  refs (NR, SR)
    and hyps (N, SH) integer ids padded, ref_len (NR) / hyp_len (N) integer tensors, ref_index (N) the reference of each hypothesis
    (None: its own, and NR = N).  Sequences longer than CM_EDIT_MAX_LEN are refused by the library (CM_EUNSUPPORTED).
    -> (counts (N, 4) int32 [ins, del, sub, hits], dist (N) int32, status (N) int32), and with want_ops also (ops (N, SR + SH) int8,
    n_ops (N) int32).  bufs: caller-placed "counts", "dist", "status", "ops", "n_ops" and "workspace" (uint8,
    cm_edit_distance_workspace_bytes)."""
    _dev_check(refs, ref_len, hyps, hyp_len, ref_index)
    if refs.dim() != 2 or hyps.dim() != 2 or refs.shape[0] == 0 or hyps.shape[0] == 0:
        raise RuntimeError(f"edit_distance: refs must be (NR, SR) and hyps (N, SH) with NR, N >= 1, got {tuple(refs.shape)} and {tuple(hyps.shape)}")
    rf, hy = refs.detach().to(torch.int32).contiguous(), hyps.detach().to(torch.int32).contiguous()
    (nr, sr), (n, sh) = rf.shape, hy.shape
    dev = hy.device
    rl, hl = ref_len.detach().to(torch.int32).contiguous(), hyp_len.detach().to(torch.int32).contiguous()
    if ref_index is None:
        if nr != n:
            raise RuntimeError(f"edit_distance: without ref_index every hypothesis has its own reference, got {nr} references for {n} hypotheses")
        ri = torch.arange(n, dtype=torch.int32, device=dev)
    else:
        ri = ref_index.detach().to(torch.int32).contiguous()
    if rl.numel() != nr or hl.numel() != n or ri.numel() != n:
        raise RuntimeError(f"edit_distance: need {nr} ref_len and {n} hyp_len / ref_index, got {rl.numel()}, {hl.numel()}, {ri.numel()}")
    take = _bufs(bufs, ("counts", "dist", "status", "ops", "n_ops", "workspace"), "edit_distance")
    counts = take("counts", (n, 4), torch.int32, dev)
    dist, status = take("dist", (n,), torch.int32, dev), take("status", (n,), torch.int32, dev)
    a = N.EditDistanceArgs()
    a.N, a.NR, a.SR, a.SH = n, nr, sr, sh
    a.refs, a.ref_len, a.hyps, a.hyp_len, a.ref_index = (_ptr(rf) if sr else None), _ptr(rl), (_ptr(hy) if sh else None), _ptr(hl), _ptr(ri)
    a.counts, a.dist, a.status = _ptr(counts), _ptr(dist), _ptr(status)
    ops_out = n_ops = None
    if want_ops:
        n_ops = take("n_ops", (n,), torch.int32, dev)
        if sr + sh:
            ops_out = take("ops", (n, sr + sh), torch.int8, dev)
            a.ops, a.n_ops = _ptr(ops_out), _ptr(n_ops)
        else:                                                        # every sequence empty: no path, and an empty tensor has no address
            ops_out = torch.empty((n, 0), dtype=torch.int8, device=dev)
            n_ops.zero_()
    nws = int(N.lib().cm_edit_distance_workspace_bytes(ct.byref(a)))
    ws = take("workspace", (max(nws, 16),), torch.uint8, dev)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_edit_distance", N.lib().cm_edit_distance, a, units=n)
    return (counts, dist, status, ops_out, n_ops) if want_ops else (counts, dist, status)


def _ctc_beam_args(what, a, log_probs, dev, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep, blank, beam_size, topk,
                   prune_history, beam_prune_logp, token_prune_min_logp, blank_skip_threshold):
    """What the three CTC beam searches prepare alike, filled into their argument struct ``a``: log_probs as fp32 / bf16 with unit
    vocabulary stride (None: no rows, V from tok_class), the token tables on the device (dev, or None for log_probs'), checked to
    cover the V tokens (tok_len: the LM search's, else None), the hash constants, beam and thresholds.
    -> (lp, T, V, keep): keep holds the converted tensors ``a`` points at."""
    if log_probs is None:
        lp, t, v = None, 0, int(tok_class.shape[0])
        a.dtype = N.CM_F32
    else:
        if log_probs.dtype not in (torch.float32, torch.bfloat16):
            log_probs = log_probs.float()
        lp = log_probs.detach()
        if lp.stride(2) != 1:
            lp = lp.contiguous()
        _, t, v = lp.shape
        a.dtype, a.lp_bs, a.lp_ts = _DT[lp.dtype], lp.stride(0), lp.stride(1)
        dev = lp.device if dev is None else dev
    tc = tok_class.detach().to(device=dev, dtype=torch.int32).contiguous()
    th = tok_hash.detach().to(device=dev, dtype=torch.int64).contiguous()
    tp = tok_pow.detach().to(device=dev, dtype=torch.int64).contiguous()
    tl = None if tok_len is None else tok_len.detach().to(device=dev, dtype=torch.int32).contiguous()
    if tc.numel() != v or th.numel() != 2 * v or tp.numel() != 2 * v or (tl is not None and tl.numel() != v):
        raise RuntimeError(f"{what}: token tables must cover the {v} tokens of log_probs")
    a.T, a.V = t, v
    a.log_probs, a.tok_class, a.tok_hash, a.tok_pow = _ptr(lp), _ptr(tc), _ptr(th), _ptr(tp)
    if tl is not None:
        a.tok_len = _ptr(tl)
    a.hash_base[0], a.hash_base[1], a.hash_sep = int(hash_base[0]), int(hash_base[1]), int(hash_sep)
    a.blank, a.beam_size, a.topk, a.prune_history = int(blank), int(beam_size), int(topk), int(bool(prune_history))
    a.beam_prune_logp, a.token_prune_min_logp = float(beam_prune_logp), float(token_prune_min_logp)
    a.blank_skip_threshold = float(blank_skip_threshold)
    return lp, t, v, (lp, tc, th, tp, tl)


def _ctc_beam_whole(what, a, workspace_bytes, lp, lengths, topk, bufs):
    """Lengths, outputs and workspace of a whole-utterance CTC beam search into its argument struct ``a`` (filled by
    _ctc_beam_args; lm_scores where the struct has it) -> (the outputs in the struct's order, the tensors to keep until launch).
    A caller-placed token_len / scores / lm_scores is not zeroed: rows past num_hyps keep what the buffer held."""
    b, t, _ = lp.shape
    dev = lp.device
    ln = lengths.detach().to(device=dev, dtype=torch.int32).contiguous()
    with_lm = hasattr(a, "lm_scores")
    take = _bufs(bufs, ("tokens", "token_len", "scores") + (("lm_scores",) if with_lm else ()) + ("num_hyps", "bad_frame", "workspace"), what)

    def per_hyp(name, dtype):                   # (batch, topk): zero where the caller places none (rows past num_hyps are not written)
        if bufs is None or bufs.get(name) is None:
            return torch.zeros((b, topk), dtype=dtype, device=dev)
        return take(name, (b, topk), dtype, dev)
    tokens = take("tokens", (b, topk, t), torch.int32, dev)
    token_len, scores = per_hyp("token_len", torch.int32), per_hyp("scores", torch.float64)
    num_hyps = take("num_hyps", (b,), torch.int32, dev)
    bad_frame = take("bad_frame", (b,), torch.int32, dev)
    a.tokens, a.token_len, a.scores, a.num_hyps, a.bad_frame = _ptr(tokens), _ptr(token_len), _ptr(scores), _ptr(num_hyps), _ptr(bad_frame)
    out = (tokens, token_len, scores, num_hyps, bad_frame)
    if with_lm:
        lm_scores = per_hyp("lm_scores", torch.float64)
        a.lm_scores = _ptr(lm_scores)
        out = out[:3] + (lm_scores,) + out[3:]
    a.batch, a.lengths = b, _ptr(ln)
    nws = int(workspace_bytes(ct.byref(a)))
    ws = take("workspace", (max(nws, 1),), torch.uint8, dev)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), nws, _stream()
    return out, (ln, ws)


def ctc_beam_search(log_probs, lengths, tok_class, tok_hash, tok_pow, hash_base, hash_sep, blank=0, beam_size=100, topk=1,
                    prune_history=False, beam_prune_logp=-10.0, token_prune_min_logp=-5.0, blank_skip_threshold=1.0, bufs=None):
    """LM-free CTC beam search (cm_ctc_beam_search).  log_probs (batch, T, V) fp32 / bf16, lengths (batch) frames to decode;
    tok_class (V) int32, tok_hash / tok_pow (V, 2) int64 holding the unsigned hash tables (mamba_asr_amd.ctc_decode builds them).
    -> (tokens (batch, topk, T) int32, token_len (batch, topk) int32, scores (batch, topk) fp64, num_hyps (batch) int32,
    bad_frame (batch) int32): hypothesis h < num_hyps[b] of utterance b is its text-changing tokens tokens[b, h, :token_len[b, h]].
    bufs: caller-placed "tokens", "token_len", "scores", "num_hyps", "bad_frame" and "workspace" (uint8,
    cm_ctc_beam_workspace_bytes)."""
    _dev_check(log_probs, lengths, tok_class, tok_hash, tok_pow)
    a = N.CtcBeamArgs()
    lp, t, _, held = _ctc_beam_args("ctc_beam_search", a, log_probs, None, tok_class, tok_hash, tok_pow, None, hash_base, hash_sep, blank,
                                    beam_size, topk, prune_history, beam_prune_logp, token_prune_min_logp, blank_skip_threshold)
    out, held_whole = _ctc_beam_whole("ctc_beam_search", a, N.lib().cm_ctc_beam_workspace_bytes, lp, lengths, topk, bufs)   # held: alive until the launch
    _launch("cm_ctc_beam_search", N.lib().cm_ctc_beam_search, a, units=lp.shape[0] * t)
    return out


_LM_TABLES = dict(word_keys=torch.int64, word_ids=torch.int32, prefix_keys=torch.int64, ngram_keys=torch.int64, ngram_vals=torch.int32,
                  prob=torch.float32, backoff=torch.float32)


def _ctc_lm_args(what, a, lm, order, n_words, lm_bos, lm_eos, lm_unk, alpha, beta, unk_score_offset):
    """What the two LM-fused CTC beam searches prepare alike: the dict of device tensors of ngram_lm.NgramLM.tables() checked
    (dtypes, contiguity, shapes) and, with the constants that describe it, filled into the argument struct ``a``."""
    for n, dtype in _LM_TABLES.items():
        if lm[n].dtype != dtype or not lm[n].is_contiguous():
            raise RuntimeError(f"{what}: lm[{n!r}] must be a contiguous {dtype} tensor")
    if lm["word_keys"].dim() != 2 or lm["word_keys"].shape[1] != 2 or lm["prefix_keys"].dim() != 2 or lm["prefix_keys"].shape[1] != 2:
        raise RuntimeError(f"{what}: word_keys and prefix_keys must be (capacity, 2)")
    if lm["word_ids"].numel() != lm["word_keys"].shape[0] or lm["ngram_vals"].numel() != lm["ngram_keys"].numel() \
            or lm["backoff"].numel() != lm["prob"].numel():
        raise RuntimeError(f"{what}: keys / values of a table, or prob / backoff, differ in length")
    a.order, a.n_words, a.lm_bos, a.lm_eos, a.lm_unk = int(order), int(n_words), int(lm_bos), int(lm_eos), int(lm_unk)
    a.n_entries, a.word_cap, a.prefix_cap, a.ngram_cap = (lm["prob"].numel(), lm["word_ids"].numel(), lm["prefix_keys"].shape[0],
                                                          lm["ngram_keys"].numel())
    a.word_keys, a.word_ids, a.prefix_keys = _ptr(lm["word_keys"]), _ptr(lm["word_ids"]), _ptr(lm["prefix_keys"])
    a.ngram_keys, a.ngram_vals, a.lm_prob, a.lm_backoff = _ptr(lm["ngram_keys"]), _ptr(lm["ngram_vals"]), _ptr(lm["prob"]), _ptr(lm["backoff"])
    a.alpha, a.beta, a.unk_score_offset = float(alpha), float(beta), float(unk_score_offset)


def ctc_beam_search_lm(log_probs, lengths, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep, lm, *, order, n_words,
                       lm_bos=-1, lm_eos=-1, lm_unk=-1, alpha=0.5, beta=1.5, unk_score_offset=-10.0, blank=0, beam_size=100, topk=1,
                       prune_history=False, beam_prune_logp=-10.0, token_prune_min_logp=-5.0, blank_skip_threshold=1.0, bufs=None):
    """CTC beam search with a fused backoff n-gram LM (cm_ctc_beam_lm_search).  The arguments of ctc_beam_search, plus tok_len
    (V) int32 (code points of each clean piece) and ``lm``, the dict of device tensors of ngram_lm.NgramLM.tables(): word_keys
    (cap, 2) / prefix_keys (cap, 2) / ngram_keys (cap) int64 bit patterns, word_ids / ngram_vals int32, prob / backoff fp32; order,
    n_words and the word ids lm_bos / lm_eos / lm_unk (-1: not used) describe it.
    -> (tokens, token_len, scores (acoustic), lm_scores (total, the ranking score), num_hyps, bad_frame) as ctc_beam_search.
    bufs: caller-placed "tokens", "token_len", "scores", "lm_scores", "num_hyps", "bad_frame" and "workspace" (uint8,
    cm_ctc_beam_lm_workspace_bytes)."""
    _dev_check(log_probs, lengths, tok_class, tok_hash, tok_pow, tok_len, *[lm[n] for n in _LM_TABLES])
    a = N.CtcBeamLmArgs()
    _ctc_lm_args("ctc_beam_search_lm", a, lm, order, n_words, lm_bos, lm_eos, lm_unk, alpha, beta, unk_score_offset)
    lp, t, _, held = _ctc_beam_args("ctc_beam_search_lm", a, log_probs, None, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep,
                                    blank, beam_size, topk, prune_history, beam_prune_logp, token_prune_min_logp, blank_skip_threshold)
    out, held_whole = _ctc_beam_whole("ctc_beam_search_lm", a, N.lib().cm_ctc_beam_lm_workspace_bytes, lp, lengths, topk, bufs)   # held: alive until the launch
    _launch("cm_ctc_beam_lm_search", N.lib().cm_ctc_beam_lm_search, a, units=lp.shape[0] * t)
    return out


def ctc_beam_stream_state(slots, beam_size, max_frames, device):
    """The zeroed state of ``slots`` streamed CTC beam searches: (slots, cm_ctc_beam_stream_state_bytes(beam_size, max_frames)) uint8.
    An all-zero slab is a slot that was never reset; a row is plain memory, so copying it copies the stream."""
    nbytes = int(N.lib().cm_ctc_beam_stream_state_bytes(int(beam_size), int(max_frames)))
    if nbytes <= 0 or slots < 1:
        raise RuntimeError(f"ctc_beam_stream_state: slots {slots} < 1, beam_size {beam_size} not in [1, 256] or max_frames "
                           f"{max_frames} not in [1, {0x7fff0000 // 256}]")
    return torch.zeros((int(slots), nbytes), dtype=torch.uint8, device=device)


def _ctc_beam_stream_run(what, a, sym, log_probs, chunk_len, state, max_frames, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep,
                         reset, emit, blank, beam_size, topk, prune_history, beam_prune_logp, token_prune_min_logp, blank_skip_threshold,
                         bufs):
    """The body of ctc_beam_stream and ctc_beam_lm_stream: the checks, the argument struct ``a`` (of cm_<sym>; its LM fields, if
    any, are filled already), the outputs (lm_scores where the struct has it) and the launch -> the outputs in the struct's order."""
    dev = state.device
    slots = state.shape[0]
    if state.dim() != 2 or state.dtype != torch.uint8 or state.stride(1) != 1:
        raise RuntimeError(f"{what}: state must be the (slots, bytes) uint8 tensor of {what}_state (or row slices of it)")
    for name, flag in (("chunk_len", chunk_len), ("reset", reset), ("emit", emit)):
        if flag is not None and (flag.dtype != torch.int32 or tuple(flag.shape) != (slots,) or not flag.is_contiguous() or flag.device != dev):
            raise RuntimeError(f"{what}: {name} must be a contiguous int32 tensor of shape ({slots},) on {dev}")
    if log_probs is not None and (log_probs.dim() != 3 or log_probs.shape[0] != slots or log_probs.device != dev):
        raise RuntimeError(f"{what}: log_probs must be ({slots}, t, V) on {dev}, got {tuple(log_probs.shape)} on {log_probs.device}")
    _, t, _, held = _ctc_beam_args(what, a, log_probs, dev, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep, blank,
                                   beam_size, topk, prune_history, beam_prune_logp, token_prune_min_logp, blank_skip_threshold)
    a.batch, a.chunk_len, a.reset, a.emit = slots, _ptr(chunk_len), _ptr(reset), _ptr(emit)
    a.state, a.state_stride_bytes, a.max_frames = _ptr(state), state.stride(0), int(max_frames)
    nws = int(getattr(N.lib(), f"cm_{sym}_workspace_bytes")(ct.byref(a)))
    with_lm = hasattr(a, "lm_scores")
    names = ("tokens", "token_len", "scores") + (("lm_scores",) if with_lm else ()) + ("num_hyps", "status")
    take = _bufs(bufs, names + ("workspace",), what)
    tokens = take("tokens", (slots, topk, int(max_frames)), torch.int32, dev)
    token_len = take("token_len", (slots, topk), torch.int32, dev)
    scores = take("scores", (slots, topk), torch.float64, dev)
    out = (tokens, token_len, scores)
    if with_lm:
        lm_scores = take("lm_scores", (slots, topk), torch.float64, dev)
        a.lm_scores = _ptr(lm_scores)
        out += (lm_scores,)
    num_hyps, status = take("num_hyps", (slots,), torch.int32, dev), take("status", (slots,), torch.int32, dev)
    ws = take("workspace", (nws,), torch.uint8, dev) if nws else None
    a.tokens, a.token_len, a.scores, a.num_hyps, a.status = _ptr(tokens), _ptr(token_len), _ptr(scores), _ptr(num_hyps), _ptr(status)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), nws, _stream()
    _launch(f"cm_{sym}", getattr(N.lib(), f"cm_{sym}"), a, units=slots * t)
    return out + (num_hyps, status)


def ctc_beam_stream(log_probs, chunk_len, state, max_frames, tok_class, tok_hash, tok_pow, hash_base, hash_sep, reset=None, emit=None,
                    blank=0, beam_size=100, topk=1, prune_history=False, beam_prune_logp=-10.0, token_prune_min_logp=-5.0,
                    blank_skip_threshold=1.0, bufs=None):
    """The next chunk of every stream through the CTC beam search (cm_ctc_beam_stream): one launch, no host synchronisation.
    log_probs (slots, t, V) fp32 / bf16 with unit vocabulary stride, or None for a reset / emit-only call; chunk_len (slots) int32
    on the device, the rows each slot consumes; state (slots, >= state bytes) uint8 from ctc_beam_stream_state, updated in place;
    reset / emit (slots) int32 device tensors or None; the token tables as for ctc_beam_search.
    -> (tokens (slots, topk, max_frames) int32, token_len (slots, topk) int32, scores (slots, topk) fp64, num_hyps (slots) int32,
    status (slots) int32).  Only the rows of slots that were active in this call are written (status), those of emitting slots
    (the rest); everything else is uninitialised memory.  bufs: caller-placed "tokens", "token_len", "scores", "num_hyps",
    "status" and "workspace" (uint8, cm_ctc_beam_stream_workspace_bytes)."""
    _dev_check(log_probs, chunk_len, state, reset, emit, tok_class, tok_hash, tok_pow)
    return _ctc_beam_stream_run("ctc_beam_stream", N.CtcBeamStreamArgs(), "ctc_beam_stream", log_probs, chunk_len, state, max_frames,
                                tok_class, tok_hash, tok_pow, None, hash_base, hash_sep, reset, emit, blank, beam_size, topk, prune_history,
                                beam_prune_logp, token_prune_min_logp, blank_skip_threshold, bufs)


def ctc_beam_lm_stream_state(slots, beam_size, max_frames, device):
    """The zeroed state of ``slots`` streamed LM-fused CTC beam searches: (slots, cm_ctc_beam_lm_stream_state_bytes(beam_size,
    max_frames)) uint8 -- ctc_beam_stream_state's slab with 36 more bytes per beam, the LM state.  A slab belongs to the LM tables
    it is advanced with."""
    nbytes = int(N.lib().cm_ctc_beam_lm_stream_state_bytes(int(beam_size), int(max_frames)))
    if nbytes <= 0 or slots < 1:
        raise RuntimeError(f"ctc_beam_lm_stream_state: slots {slots} < 1, beam_size {beam_size} not in [1, 256] or max_frames "
                           f"{max_frames} not in [1, {0x7fff0000 // 256}]")
    return torch.zeros((int(slots), nbytes), dtype=torch.uint8, device=device)


def ctc_beam_lm_stream(log_probs, chunk_len, state, max_frames, tok_class, tok_hash, tok_pow, tok_len, hash_base, hash_sep, lm, *, order,
                       n_words, lm_bos=-1, lm_eos=-1, lm_unk=-1, alpha=0.5, beta=1.5, unk_score_offset=-10.0, reset=None, emit=None,
                       blank=0, beam_size=100, topk=1, prune_history=False, beam_prune_logp=-10.0, token_prune_min_logp=-5.0,
                       blank_skip_threshold=1.0, bufs=None):
    """The next chunk of every stream through the LM-fused CTC beam search (cm_ctc_beam_lm_stream): ctc_beam_stream with the LM of
    ctc_beam_search_lm (tok_len, the ``lm`` dict of device tensors and the constants that describe it); state from
    ctc_beam_lm_stream_state.
    -> (tokens, token_len, scores (acoustic), lm_scores (total, the ranking score), num_hyps, status), written as ctc_beam_stream
    writes its outputs.  bufs: caller-placed "tokens", "token_len", "scores", "lm_scores", "num_hyps", "status" and "workspace"."""
    _dev_check(log_probs, chunk_len, state, reset, emit, tok_class, tok_hash, tok_pow, tok_len, *[lm[n] for n in _LM_TABLES])
    a = N.CtcBeamLmStreamArgs()
    _ctc_lm_args("ctc_beam_lm_stream", a, lm, order, n_words, lm_bos, lm_eos, lm_unk, alpha, beta, unk_score_offset)
    return _ctc_beam_stream_run("ctc_beam_lm_stream", a, "ctc_beam_lm_stream", log_probs, chunk_len, state, max_frames, tok_class,
                                tok_hash, tok_pow, tok_len, hash_base, hash_sep, reset, emit, blank, beam_size, topk, prune_history,
                                beam_prune_logp, token_prune_min_logp, blank_skip_threshold, bufs)


def _ctc_prefix_args(what, logp, n_u, row_utt, last, r_n, r_b, psi_g, blank, eos, validated):
    """The arguments cm_ctc_prefix_score and cm_ctc_prefix_advance share, checked: sizes, dtypes and (one host read, skipped
    with validated=True for a row_utt the caller has checked already) row_utt's range."""
    _dev_check(logp, n_u, row_utt, last, r_n, r_b, psi_g)
    if logp.dim() != 3 or logp.dtype != torch.float32 or not logp.is_contiguous():
        raise RuntimeError(f"{what}: logp must be a contiguous fp32 (U, T, V) tensor")
    U, T, V = logp.shape
    rows = row_utt.shape[0]
    for name, t, shape, dtype in (("n_u", n_u, (U,), torch.int32), ("row_utt", row_utt, (rows,), torch.int32),
                                  ("last", last, (rows,), torch.int32), ("r_n", r_n, (rows, T), torch.float32),
                                  ("r_b", r_b, (rows, T), torch.float32), ("psi_g", psi_g, (rows,), torch.float32)):
        if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous {dtype} tensor of shape {shape}, got {t.dtype} {tuple(t.shape)}")
    if not validated and rows and bool(((row_utt < 0) | (row_utt >= U)).any()):
        raise RuntimeError(f"{what}: row_utt holds an utterance index outside [0, {U})")
    a = N.CtcPrefixArgs()
    a.U, a.T, a.V, a.rows, a.blank, a.eos = U, T, V, rows, int(blank), int(eos)
    a.logp, a.n_u, a.row_utt, a.last, a.r_n, a.r_b, a.psi_g = _ptr(logp), _ptr(n_u), _ptr(row_utt), _ptr(last), _ptr(r_n), _ptr(r_b), _ptr(psi_g)
    a.stream = _stream()
    return a


def ctc_prefix_score(logp, n_u, row_utt, last, r_n, r_b, psi_g, blank, eos, candidates=None, validated=False, bufs=None):
    """CTC prefix score deltas (cm_ctc_prefix_score).  logp (U, T, V) fp32 CTC log-posteriors, n_u (U) int32 frames per
    utterance; per hypothesis row: row_utt (rows) int32, last (rows) int32 (-1: empty prefix), r_n / r_b (rows, T) fp32,
    psi_g (rows) fp32.  -> (rows, V) fp32 psi(prefix + c) - psi_g, or (rows, K) for candidates (rows, K) int32 (-inf for a
    candidate outside [0, V)); -inf for blank and for impossible extensions; column eos holds the prefix's CTC log-likelihood.
    bufs: a caller-placed "out"."""
    a = _ctc_prefix_args("ctc_prefix_score", logp, n_u, row_utt, last, r_n, r_b, psi_g, blank, eos, validated)
    ncol = a.V
    if candidates is not None:
        _dev_check(candidates)
        if candidates.dim() != 2 or candidates.shape[0] != a.rows or candidates.shape[1] < 1 or candidates.dtype != torch.int32 \
                or not candidates.is_contiguous():
            raise RuntimeError("ctc_prefix_score: candidates must be a contiguous int32 (rows, K >= 1) tensor")
        ncol = a.K = candidates.shape[1]
        a.candidates = _ptr(candidates)
    out = _bufs(bufs, ("out",), "ctc_prefix_score")("out", (a.rows, ncol), torch.float32, logp.device)
    a.out = _ptr(out)
    _launch("cm_ctc_prefix_score", N.lib().cm_ctc_prefix_score, a, units=a.rows * a.T)
    return out


def ctc_prefix_advance(logp, n_u, row_utt, last, r_n, r_b, psi_g, tokens, blank, eos, validated=False, bufs=None):
    """Every row's prefix extended by tokens (rows) int32 (cm_ctc_prefix_advance; arguments as ctc_prefix_score) ->
    new (r_n, r_b, psi_g, last) in fresh tensors.  A row whose token is eos keeps its state.  bufs: caller-placed "r_n_out",
    "r_b_out", "psi_out" and "last_out"."""
    a = _ctc_prefix_args("ctc_prefix_advance", logp, n_u, row_utt, last, r_n, r_b, psi_g, blank, eos, validated)
    _dev_check(tokens)
    if tuple(tokens.shape) != (a.rows,) or tokens.dtype != torch.int32 or not tokens.is_contiguous():
        raise RuntimeError("ctc_prefix_advance: tokens must be a contiguous int32 (rows,) tensor")
    take = _bufs(bufs, ("r_n_out", "r_b_out", "psi_out", "last_out"), "ctc_prefix_advance")
    dev = logp.device
    r_n2, r_b2 = take("r_n_out", (a.rows, a.T), torch.float32, dev), take("r_b_out", (a.rows, a.T), torch.float32, dev)
    psi2, last2 = take("psi_out", (a.rows,), torch.float32, dev), take("last_out", (a.rows,), torch.int32, dev)
    a.tokens, a.r_n_out, a.r_b_out, a.psi_out, a.last_out = _ptr(tokens), _ptr(r_n2), _ptr(r_b2), _ptr(psi2), _ptr(last2)
    _launch("cm_ctc_prefix_advance", N.lib().cm_ctc_prefix_advance, a, units=a.rows * a.T)
    return r_n2, r_b2, psi2, last2


def beam_select(att, alive, B, eos, delta=None, weight=0.0, eos_blocked=None, bufs=None):
    """One token's selection of an S2S beam search (cm_beam_select).  att (U * B, V) fp32 decoder
    log-probabilities and alive (U * B) fp32 running scores (-inf: dead slot) of rows u * B + k; delta (U * B, V) fp32 CTC
    prefix scores added with ``weight``, or None; eos_blocked (U) int32, nonzero where <eos> may not be chosen, or None.
    -> (score, inc, parent, token), each (U, B): per utterance the B best candidates under (alive + inc descending, flat index
    k * V + c ascending), inc = att [+ weight * delta] as separately rounded fp32 operations; parent / token int32.
    bufs: caller-placed "score", "inc", "parent", "token" and "workspace" (uint8, cm_beam_select_workspace_bytes, 8-byte aligned)."""
    _dev_check(att, alive, delta, eos_blocked)
    B = int(B)
    if not 1 <= B <= N.CM_BEAM_SELECT_MAX_B:
        raise RuntimeError(f"beam_select: B must be in [1, {N.CM_BEAM_SELECT_MAX_B}], got {B}")
    if att.dim() != 2 or att.dtype != torch.float32 or not att.is_contiguous() or att.shape[0] < B or att.shape[0] % B or att.shape[1] < 1:
        raise RuntimeError(f"beam_select: att must be a contiguous fp32 (U * {B}, V) tensor, got {att.dtype} {tuple(att.shape)}")
    rows, V = att.shape
    U = rows // B
    if B * V >= 2 ** 31:
        raise RuntimeError(f"beam_select: B * V = {B * V} must stay below 2^31")
    for name, t, shape, dtype in (("alive", alive, (rows,), torch.float32), ("delta", delta, (rows, V), torch.float32),
                                  ("eos_blocked", eos_blocked, (U,), torch.int32)):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != att.device):
            raise RuntimeError(f"beam_select: {name} must be a contiguous {dtype} tensor of shape {shape} on {att.device}, "
                               f"got {t.dtype} {tuple(t.shape)}")
    lib = N.lib()
    nws = lib.cm_beam_select_workspace_bytes(U, B, V)
    if nws <= 0:
        raise RuntimeError(f"beam_select: unsupported sizes U={U} B={B} V={V}")
    take = _bufs(bufs, ("score", "inc", "parent", "token", "workspace"), "beam_select")
    if bufs is not None and bufs.get("workspace") is not None:
        ws = take("workspace", (nws,), torch.uint8, att.device)
        ws_bytes = nws
    else:
        ws = torch.empty((nws + 7) // 8, dtype=torch.int64, device=att.device)  # int64: the 8-byte alignment the library asks for
        ws_bytes = ws.numel() * 8
    score, inc = (take(n, (U, B), torch.float32, att.device) for n in ("score", "inc"))
    parent, token = (take(n, (U, B), torch.int32, att.device) for n in ("parent", "token"))
    a = N.BeamSelectArgs()
    a.U, a.B, a.V, a.eos, a.weight = U, B, V, int(eos), float(weight)
    a.att, a.delta, a.alive, a.eos_blocked = _ptr(att), _ptr(delta), _ptr(alive), _ptr(eos_blocked)
    a.score, a.inc, a.parent, a.token = _ptr(score), _ptr(inc), _ptr(parent), _ptr(token)
    a.workspace, a.workspace_bytes, a.stream = _ptr(ws), ws_bytes, _stream()
    _launch("cm_beam_select", lib.cm_beam_select, a, units=rows * V)
    return score, inc, parent, token


def _attn_step_shapes(qkv, kc, vc, anc, t, H):
    """The shape checks both routes of attn_step share -> (R, D, Lcap)."""
    if qkv.dim() != 2 or qkv.shape[0] < 1 or qkv.shape[1] % 3 or not qkv.is_contiguous():
        raise RuntimeError(f"attn_step: qkv must be a contiguous (R, 3 * D) tensor, got {tuple(qkv.shape)}")
    R, D = qkv.shape[0], qkv.shape[1] // 3
    H, t = int(H), int(t)
    if H < 1 or D % H:
        raise RuntimeError(f"attn_step: D = {D} is no multiple of H = {H}")
    for name, c in (("kc", kc), ("vc", vc)):
        if (c.dim() != 3 or tuple(c.shape[1:]) != (R, D) or c.dtype != qkv.dtype or c.device != qkv.device or c.stride(2) != 1
                or c.stride(1) != D or (c.shape[0] > 1 and c.stride(0) < R * D)):
            raise RuntimeError(f"attn_step: {name} must be a (Lcap, {R}, {D}) {qkv.dtype} tensor with contiguous positions on "
                               f"{qkv.device}, got {c.dtype} {tuple(c.shape)} strides {tuple(c.stride())}")
    Lcap = kc.shape[0]
    if vc.shape[0] != Lcap or vc.stride(0) != kc.stride(0):
        raise RuntimeError("attn_step: kc and vc must have the same positions and position stride")
    if tuple(anc.shape) != (Lcap, R) or anc.dtype != torch.int32 or not anc.is_contiguous() or anc.device != qkv.device:
        raise RuntimeError(f"attn_step: anc must be a contiguous int32 ({Lcap}, {R}) tensor on {qkv.device}, got {anc.dtype} "
                           f"{tuple(anc.shape)}")
    if not 0 <= t < Lcap:
        raise RuntimeError(f"attn_step: position t = {t} does not fit caches of {Lcap} positions")
    return R, D, Lcap


def attn_step(qkv, kc, vc, anc, t, H, bufs=None):
    """One decoding step of H-head self-attention over a KV cache addressed through a beam-ancestry table (cm_attn_step,
    DESIGN.md §4f).  qkv (R, 3 D) bf16 / fp32: this step's q | k | v; kc, vc (Lcap, R, D) caches of qkv's dtype, written in place
    at position t and nowhere else; anc (Lcap, R) int32: anc[s, r] is the row in which row r's prefix token of position s < t was
    cached (an entry outside [0, R) scores -inf); -> out (R, D) in qkv's dtype.  fp32 arithmetic; D / H in {32, 64}, H <= 32,
    t < 4096.  bufs: a caller-placed "out"."""
    _dev_check(qkv, kc, vc, anc)
    if qkv.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"attn_step: unsupported dtype {qkv.dtype} (fp32 / bf16)")
    R, D, Lcap = _attn_step_shapes(qkv, kc, vc, anc, t, H)
    out = _bufs(bufs, ("out",), "attn_step")("out", (R, D), qkv.dtype, qkv.device)
    a = N.AttnStepArgs()
    a.R, a.D, a.H, a.t, a.Lcap, a.io_dtype = R, D, int(H), int(t), Lcap, _DT[qkv.dtype]
    a.kv_stride = kc.stride(0) if Lcap > 1 else R * D
    a.qkv, a.kc, a.vc, a.anc, a.out, a.stream = _ptr(qkv), _ptr(kc), _ptr(vc), _ptr(anc), _ptr(out), _stream()
    _launch("cm_attn_step", N.lib().cm_attn_step, a, units=R * int(H) * (int(t) + 1))
    return out


def attn_step_torch(qkv, kc, vc, anc, t, H):
    """attn_step's contract restated in torch (the CM_ATTN_STEP=0 route; any device): gather the cached K and V by ``anc``,
    matmul, softmax, matmul.  Arithmetic in fp32 (fp64 for fp64 tensors), the result rounded to qkv's dtype."""
    R, D, _ = _attn_step_shapes(qkv, kc, vc, anc, t, H)
    H, t = int(H), int(t)
    dh = D // H
    q, k, v = qkv.split(D, dim=1)
    kc[t].copy_(k)
    vc[t].copy_(v)
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    idx = anc[:t].long()
    valid = (idx >= 0) & (idx < R)
    take = idx.clamp(0, R - 1).unsqueeze(-1).expand(t, R, D)
    K = torch.cat([kc[:t].gather(1, take), k.unsqueeze(0)]).to(ct).view(t + 1, R, H, dh).permute(1, 2, 0, 3)   # (R, H, t + 1, dh)
    V = torch.cat([vc[:t].gather(1, take), v.unsqueeze(0)]).to(ct).view(t + 1, R, H, dh).permute(1, 2, 0, 3)
    x = torch.matmul(K, q.to(ct).view(R, H, dh, 1)).squeeze(-1) / math.sqrt(dh)                                # (R, H, t + 1)
    valid = torch.cat([valid, torch.ones((1, R), dtype=torch.bool, device=qkv.device)]).t().unsqueeze(1)       # (R, 1, t + 1)
    p = torch.softmax(x.masked_fill(~valid, float("-inf")), dim=-1)
    V = V.masked_fill(~valid.unsqueeze(-1), 0.0)                   # a position without weight adds nothing, whatever it holds
    return torch.matmul(p.unsqueeze(2), V).reshape(R, D).to(qkv.dtype)


def _xattn_step_shapes(q, k, v, row_utt, enc_len, H):
    """The shape checks both routes of xattn_step share -> (R, D, U, T)."""
    if q.dim() != 2 or q.shape[0] < 1 or not q.is_contiguous():
        raise RuntimeError(f"xattn_step: q must be a contiguous (R, D) tensor, got {tuple(q.shape)}")
    R, D = q.shape
    H = int(H)
    if H < 1 or D % H:
        raise RuntimeError(f"xattn_step: D = {D} is no multiple of H = {H}")
    for name, c in (("k", k), ("v", v)):
        if (c.dim() != 3 or c.shape[0] < 1 or c.shape[1] < 1 or c.shape[2] != D or c.dtype != q.dtype or c.device != q.device
                or c.stride(2) != 1 or (c.shape[1] > 1 and c.stride(1) < D)
                or (c.shape[0] > 1 and c.stride(0) < (c.shape[1] - 1) * c.stride(1) + D)):
            raise RuntimeError(f"xattn_step: {name} must be a (U, T, {D}) {q.dtype} view on {q.device} with unit element stride and "
                               f"non-overlapping frames, got {c.dtype} {tuple(c.shape)} strides {tuple(c.stride())}")
    U, T = k.shape[0], k.shape[1]
    if tuple(v.shape) != (U, T, D):
        raise RuntimeError(f"xattn_step: k {tuple(k.shape)} and v {tuple(v.shape)} differ")
    for name, c, n in (("row_utt", row_utt, R), ("enc_len", enc_len, U)):
        if tuple(c.shape) != (n,) or c.dtype != torch.int32 or not c.is_contiguous() or c.device != q.device:
            raise RuntimeError(f"xattn_step: {name} must be a contiguous int32 ({n},) tensor on {q.device}, got {c.dtype} "
                               f"{tuple(c.shape)}")
    return R, D, U, T


def xattn_step(q, k, v, row_utt, enc_len, H, bufs=None):
    """One decoding step of H-head cross-attention of R hypothesis rows over the encoder memory of their utterance
    (cm_xattn_step).  q (R, D) bf16 / fp32; k, v (U, T, D) views of q's dtype, projected once per utterance
    (any utterance / frame strides: the two halves of one (U, T, 2 D) GEMM result work); row_utt (R) int32: the utterance of
    each row; enc_len (U) int32: its valid frames -> out (R, D) in q's dtype, softmax over frames s < min(enc_len[u], T) only;
    a row with row_utt outside [0, U) or no valid frame is zero.  fp32 arithmetic; D / H in {32, 36, 64}, H <= 32, T < 8192.
    bufs: a caller-placed "out"."""
    _dev_check(q, k, v, row_utt, enc_len)
    if q.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"xattn_step: unsupported dtype {q.dtype} (fp32 / bf16)")
    R, D, U, T = _xattn_step_shapes(q, k, v, row_utt, enc_len, H)
    out = _bufs(bufs, ("out",), "xattn_step")("out", (R, D), q.dtype, q.device)
    a = N.XattnStepArgs()
    a.R, a.U, a.T, a.D, a.H, a.io_dtype = R, U, T, D, int(H), _DT[q.dtype]
    for name, c in (("k", k), ("v", v)):
        fs = c.stride(1) if T > 1 else D
        setattr(a, name + "_frame_stride", fs)
        setattr(a, name + "_utt_stride", c.stride(0) if U > 1 else (T - 1) * fs + D)
    a.q, a.k, a.v, a.row_utt, a.enc_len, a.out, a.stream = _ptr(q), _ptr(k), _ptr(v), _ptr(row_utt), _ptr(enc_len), _ptr(out), _stream()
    _launch("cm_xattn_step", N.lib().cm_xattn_step, a, units=R * int(H) * T)
    return out


def xattn_step_torch(q, k, v, row_utt, enc_len, H, grouped=None):
    """xattn_step's contract restated in torch (the CM_XATTN_STEP=0 route; any device, fp64 included): scores, a length mask,
    softmax, the weighted sum.  Where row_utt is arange(U).repeat_interleave(B) -- a beam search's rows -- the B rows of an
    utterance form one (B, dh) x (dh, T) product per head against the shared K and V (the grouped form); otherwise K and V are
    gathered by row_utt.  ``grouped``: True / False when the caller knows which holds; None reads it from row_utt (one host
    read).  Arithmetic in fp32 (fp64 for fp64 tensors), the result rounded to q's dtype."""
    R, D, U, T = _xattn_step_shapes(q, k, v, row_utt, enc_len, H)
    H = int(H)
    dh = D // H
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    if grouped is None:
        grouped = R % U == 0 and torch.equal(row_utt, torch.arange(U, dtype=torch.int32, device=q.device).repeat_interleave(R // U))
    frames = torch.arange(T, device=q.device)
    n = enc_len.clamp(max=T)
    if grouped:
        B = R // U
        valid = (frames[None, :] < n[:, None]).view(U, 1, 1, T)
        qh = q.to(ct).view(U, B, H, dh).permute(0, 2, 1, 3)                          # (U, H, B, dh)
        K = k.to(ct).view(U, T, H, dh).permute(0, 2, 3, 1)                           # (U, H, dh, T)
        V = v.to(ct).view(U, T, H, dh).permute(0, 2, 1, 3)                           # (U, H, T, dh)
        V = V.masked_fill(~valid.view(U, 1, T, 1), 0.0)                              # a masked frame adds nothing, whatever it holds
    else:
        ok = (row_utt >= 0) & (row_utt < U)
        take = row_utt.clamp(0, U - 1).long()
        valid = (frames[None, :] < torch.where(ok, n[take], torch.zeros_like(n[take]))[:, None]).view(R, 1, 1, T)
        qh = q.to(ct).view(R, H, 1, dh)
        K = k[take].to(ct).view(R, T, H, dh).permute(0, 2, 3, 1)
        V = v[take].to(ct).view(R, T, H, dh).permute(0, 2, 1, 3)
        V = V.masked_fill(~valid.view(R, 1, T, 1), 0.0)
    x = (torch.matmul(qh, K) / math.sqrt(dh)).masked_fill(~valid, float("-inf"))
    p = torch.softmax(x, dim=-1).masked_fill(~valid, 0.0)                            # a row without a valid frame: zeros, not NaN
    return torch.matmul(p, V).permute(0, 2, 1, 3).reshape(R, D).to(q.dtype)


class CtcLossFn(torch.autograd.Function):
    """sum over the batch of the per-utterance CTC negative log-likelihoods (zero_infinity), gradient from the same call."""

    @staticmethod
    def forward(ctx, log_probs, targets, input_lengths, target_lengths, blank):
        nll, grad = ctc_loss_grad(log_probs, targets, input_lengths, target_lengths, blank)
        ctx.save_for_backward(grad)
        ctx.in_dtype = log_probs.dtype
        return nll.sum()

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        return (grad * gout).to(ctx.in_dtype), None, None, None, None


def sum_leading(t: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """t (batch, ...) -> sum over the leading axis with fp32 accumulation in a fixed order (cm_sum_leading): folds per-utterance
    weight-gradient products; output in ``out_dtype`` (fp32 = a parameter's gradient dtype, no cast afterwards)."""
    _dev_check(t)
    n = t[0].numel()
    vec = 8 if t.dtype == torch.bfloat16 else 4
    if t.dtype not in (torch.float32, torch.bfloat16) or n % vec or not t.is_contiguous():
        return t.sum(0).to(out_dtype)
    out = torch.empty(t.shape[1:], dtype=out_dtype, device=t.device)
    N.check(N.lib().cm_sum_leading(_ptr(t), _ptr(out), t.shape[0], n, _DT[t.dtype], _DT[out_dtype], _stream()), "cm_sum_leading")
    return out


def conv_cl_bwd(x, weight_f, bias_f, du_f, weight_b=None, bias_b=None, du_b=None, dz_f=None, dz_b=None, dx=None, dz=None):
    """Backward of the channels-last causal depthwise conv + SiLU, one or both BiMamba directions in one pass
    (cm_conv_cl_bwd).  x, du_*, dz_* (batch, seqlen, dim) views; weights (dim, 4).  dx = dx_fwd + dx_bwd; dz = dz_f + dz_b
    when given.  Returns (dx, dz or None, dweight_f, dbias_f, dweight_b, dbias_b) with fp32 parameter gradients."""
    _dev_check(x, weight_f, bias_f, du_f, weight_b, bias_b, du_b, dz_f, dz_b, dx, dz)
    for t, nm in ((x, "x"), (du_f, "du_f"), (du_b, "du_b"), (dz_f, "dz_f"), (dz_b, "dz_b"), (dx, "dx"), (dz, "dz")):
        if t is not None:
            _rows_ok(t, nm)
            if t.shape != x.shape or t.dtype != x.dtype:
                raise RuntimeError(f"conv_cl_bwd: {nm} must match x in shape and dtype")
    b, l, d = x.shape
    two = du_b is not None
    wf, bf, wb, bb = _f32c(weight_f).reshape(d, -1), _f32c(bias_f), (_f32c(weight_b).reshape(d, -1) if two else None), (_f32c(bias_b) if two else None)
    if dx is None:
        dx = torch.empty((b, l, d), dtype=x.dtype, device=x.device)
    if dz is None and dz_f is not None:
        dz = torch.empty((b, l, d), dtype=x.dtype, device=x.device)
    dev = x.device
    kw = wf.shape[1]
    a = N.ConvClBwdArgs()
    a.batch, a.seqlen, a.dim, a.width, a.io_dtype = b, l, d, wf.shape[1], _DT[x.dtype]
    a.x, a.weight_f, a.bias_f, a.weight_b, a.bias_b = _ptr(x), _ptr(wf), _ptr(bf), _ptr(wb), _ptr(bb)
    a.du_f, a.du_b, a.dz_f, a.dz_b, a.dx, a.dz = _ptr(du_f), _ptr(du_b), _ptr(dz_f), _ptr(dz_b), _ptr(dx), _ptr(dz)
    # the kernel writes contiguous (dim, 4) / (dim) tensors: hand it contiguous staging slices of one buffer (overwrite: no memset)
    flat = torch.empty((2 * d * (kw + 1),), dtype=torch.float32, device=dev)
    a.overwrite = 1
    dwf, dwb_ = flat[:d * kw].view(d, kw), flat[d * kw:2 * d * kw].view(d, kw)
    dbf_, dbb_ = flat[2 * d * kw:2 * d * kw + d], flat[2 * d * kw + d:]
    dbf = dbf_ if bf is not None else None
    dwb = dwb_ if two else None
    dbb = dbb_ if (two and bb is not None) else None
    a.dweight_f, a.dbias_f, a.dweight_b, a.dbias_b = _ptr(dwf), _ptr(dbf), _ptr(dwb), _ptr(dbb)
    a.x_bs, a.x_ts, a.duf_bs, a.duf_ts = x.stride(0), x.stride(1), du_f.stride(0), du_f.stride(1)
    if two:
        a.dub_bs, a.dub_ts = du_b.stride(0), du_b.stride(1)
    if dz_f is not None:
        a.dzf_bs, a.dzf_ts = dz_f.stride(0), dz_f.stride(1)
    if dz_b is not None:
        a.dzb_bs, a.dzb_ts = dz_b.stride(0), dz_b.stride(1)
    a.dx_bs, a.dx_ts = dx.stride(0), dx.stride(1)
    if dz is not None:
        a.dz_bs, a.dz_ts = dz.stride(0), dz.stride(1)
    nws = int(N.lib().cm_conv_cl_bwd_workspace_floats(b, l, d))
    ws = torch.empty((nws,), dtype=torch.float32, device=dev)
    a.workspace, a.workspace_floats, a.stream = _ptr(ws), nws, _stream()
    _launch("cm_conv_cl_bwd", N.lib().cm_conv_cl_bwd, a, units=b * l)
    return dx, dz, dwf, dbf, dwb, dbb


def scan_ckpt_shape(batch: int, seqlen: int, dim: int):
    """Shape of the checkpoint tensor the training forward writes (cm_scan_cl_dir.ckpt)."""
    return (batch, 2 * ((seqlen + 15) // 16), dim, 16)


def scan_cl_bwd(directions, z, time_chunks=0, da_log=False):
    """Channels-last selective scan backward, 1 or 2 directions in one launch (cm_scan_cl_bwd): the gradient of
    scan_cl_fwd's xdbl mode (z and softplus on) including the dt_proj part.

    ``directions``: list of dicts with u (batch, seqlen, dim), xdbl (batch, seqlen, P + 32), A (dim, 16), dt_weight (dim, P)
    zero padded (pad_dt_weight), D, delta_bias (dim), ckpt and ypre as the forward wrote them, dout (batch, seqlen, dim),
    reverse; optional pre-allocated du, dz, dxdbl views.  Returns a list of dicts du, dz (this direction's share), dxdbl
    (I/O dtype, [d dt | dB | dC]), and fp32 dA (dim, 16), ddt_weight (dim, P), dD, ddelta_bias (dim).
    ``time_chunks``: 0 lets the library cut launches that would leave CUs idle along time, 1 never, n asks for n chunks.
    ``da_log``: dA is returned as the gradient w.r.t. A_log (A = -exp(A_log)): dA * A, formed in the reduce pass."""
    if not 1 <= len(directions) <= 2:
        raise RuntimeError("1 or 2 directions")
    u0 = directions[0]["u"]
    _dev_check(u0, z)
    _rows_ok(u0, "u"), _rows_ok(z, "z")
    b, l, d = u0.shape
    if z.shape != (b, l, d) or z.dtype != u0.dtype:
        raise RuntimeError("scan_cl_bwd: z must be (batch, seqlen, dim) in u's dtype")
    a = N.ScanClBwdArgs()
    a.batch, a.seqlen, a.dim, a.dstate, a.io_dtype, a.ndir = b, l, d, 16, _DT[u0.dtype], len(directions)
    a.z, a.z_bs, a.z_ts = _ptr(z), z.stride(0), z.stride(1)
    a.time_chunks = int(time_chunks)
    a.da_log = int(bool(da_log))
    keep, outs = [], []
    for i, dd in enumerate(directions):
        u, xdbl, dout, ypre, ck = dd["u"], dd["xdbl"], dd["dout"], dd["ypre"], dd["ckpt"]
        _dev_check(u, xdbl, dout, ypre, ck, dd["A"], dd["dt_weight"])
        for t, nm in ((u, "u"), (xdbl, "xdbl"), (dout, "dout"), (ypre, "ypre")):
            _rows_ok(t, nm)
        pad = xdbl.shape[-1] - 32
        if pad not in (16, 32) or (pad == 32 and u0.dtype != torch.bfloat16):
            raise RuntimeError("scan_cl_bwd: xdbl rows are 48 wide, or 64 wide (dt_rank > 16) in bf16")
        if any(t.shape != (b, l, d) or t.dtype != u0.dtype for t in (u, dout, ypre)) or xdbl.shape != (b, l, pad + 32) or xdbl.dtype != u0.dtype:
            raise RuntimeError("scan_cl_bwd: u / dout / ypre (batch, seqlen, dim) and xdbl (batch, seqlen, 48 | 64) must share shape prefix and dtype")
        if tuple(ck.shape) != scan_ckpt_shape(b, l, d) or ck.dtype != torch.float32 or not ck.is_contiguous():
            raise RuntimeError("scan_cl_bwd: ckpt must be the contiguous fp32 tensor the forward wrote (ops.scan_ckpt_shape)")
        dt_w = dd["dt_weight"]
        if dt_w.shape != (d, pad):
            raise RuntimeError(f"scan_cl_bwd: dt_weight must be (dim, {pad}), zero padded (ops.pad_dt_weight)")
        A, D, bias, dt_w = _f32c(dd["A"]), _f32c(dd.get("D")), _f32c(dd.get("delta_bias")), _f32c(dt_w)
        du = dd.get("du") if dd.get("du") is not None else torch.empty((b, l, d), dtype=u.dtype, device=u.device)
        dz = dd.get("dz") if dd.get("dz") is not None else torch.empty((b, l, d), dtype=u.dtype, device=u.device)
        dx = dd.get("dxdbl") if dd.get("dxdbl") is not None else torch.empty((b, l, pad + 32), dtype=u.dtype, device=u.device)
        for t, nm in ((du, "du"), (dz, "dz"), (dx, "dxdbl")):
            _rows_ok(t, nm)
        if i == 0:                                            # one buffer for every parameter gradient of the launch (overwrite: no memset)
            npar = d * (16 + pad + 2)
            zeros = torch.empty((len(directions) * npar,), dtype=torch.float32, device=u.device)
            a.overwrite = 1
        zp = zeros[i * npar:(i + 1) * npar]
        dA, dW = zp[:16 * d].view(d, 16), zp[16 * d:(16 + pad) * d].view(d, pad)
        dD = zp[(16 + pad) * d:(17 + pad) * d] if D is not None else None
        db = zp[(17 + pad) * d:] if bias is not None else None
        keep += [A, D, bias, dt_w]
        x = a.dir[i]
        x.u, x.xdbl, x.A, x.dt_weight, x.D, x.delta_bias, x.ckpt, x.ypre, x.dout = (_ptr(u), _ptr(xdbl), _ptr(A), _ptr(dt_w), _ptr(D),
                                                                                    _ptr(bias), _ptr(ck), _ptr(ypre), _ptr(dout))
        x.du, x.dz, x.dxdbl, x.dA, x.ddt_weight, x.dD, x.ddelta_bias = _ptr(du), _ptr(dz), _ptr(dx), _ptr(dA), _ptr(dW), _ptr(dD), _ptr(db)
        x.u_bs, x.u_ts, x.xdbl_bs, x.xdbl_ts = u.stride(0), u.stride(1), xdbl.stride(0), xdbl.stride(1)
        x.ypre_bs, x.ypre_ts, x.dout_bs, x.dout_ts = ypre.stride(0), ypre.stride(1), dout.stride(0), dout.stride(1)
        x.du_bs, x.du_ts, x.dz_bs, x.dz_ts, x.dxdbl_bs, x.dxdbl_ts = du.stride(0), du.stride(1), dz.stride(0), dz.stride(1), dx.stride(0), dx.stride(1)
        x.reverse_time, x.dt_rank = int(bool(dd.get("reverse", False))), pad
        outs.append(dict(du=du, dz=dz, dxdbl=dx, dA=dA, ddt_weight=dW, dD=dD, ddelta_bias=db))
    a.stream = _stream()
    nbytes = int(N.lib().cm_scan_cl_bwd_workspace_bytes(ct.byref(a)))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=u0.device)
    a.workspace, a.workspace_bytes = _ptr(ws), nbytes
    _launch("cm_scan_cl_bwd", N.lib().cm_scan_cl_bwd, a, units=b * l * len(directions))
    return outs


def conv_xproj_supported(dim: int, dt_pad: int, d_conv: int = 4, ndir: int = 2) -> bool:
    """cm_conv_xproj (``ndir`` 2) / cm_conv_xproj_uni (1) take the mixer: conv width 4, channels in whole 32-column groups up to 2048,
    and for both directions with 64-wide x_dbl rows (dt_pad 32: 16 < dt_rank <= 32) a 16-step tile pair within 80 KiB of LDS -- 1248
    channels at the most (the entry points' own checks, csrc/conv_xproj.hip)."""
    return d_conv == 4 and dim % 32 == 0 and dim <= 2048 and (dt_pad != 32 or ndir == 1 or 2 * 16 * (dim + 16) * 2 <= 80 * 1024)


def conv_xproj(x, weight_f, bias_f, weight_b, bias_b, wx_f, wx_b, out_f, out_b, xdbl=None, variant: int = 0, lens=None):
    """Both directions' depthwise conv + SiLU and x_proj GEMMs in one kernel (cm_conv_xproj, bf16).
    x (batch, seqlen, dim) view; conv weights (dim, 4) fp32; wx_f / wx_b PackedWeight of the (P + 32, dim) re-rowed x_proj
    weights [dt P | B | C], P = 16, or 32 for 16 < dt_rank <= 32; out_f / out_b (batch, seqlen, dim) views.
    ``lens`` (cm_conv_xproj_lens): int32 (batch,) device tensor, utterance b has lens[b] rows -- the backward direction's taps past
    them read the conv's zero padding; rows at and past lens[b] of the three outputs are not written.
    Returns xdbl (batch, seqlen, 2 * (P + 32)) bf16."""
    _dev_check(x, weight_f, bias_f, weight_b, bias_b, out_f, out_b)
    _rows_ok(x, "x"), _rows_ok(out_f, "out_f"), _rows_ok(out_b, "out_b")
    b, l, d = x.shape
    if x.dtype != torch.bfloat16 or out_f.dtype != torch.bfloat16 or out_b.dtype != torch.bfloat16:
        raise RuntimeError("conv_xproj: bf16 only")
    rw = wx_f.shape[0]
    if rw not in (48, 64) or wx_f.shape != (rw, d) or wx_b.shape != (rw, d):
        raise RuntimeError("conv_xproj: wx must be PackedWeight of shape (48 | 64, dim)")
    wf, bf, wb, bb = _f32c(weight_f), _f32c(bias_f), _f32c(weight_b), _f32c(bias_b)
    if xdbl is None:
        xdbl = torch.empty((b, l, 2 * rw), dtype=torch.bfloat16, device=x.device)
    elif xdbl.shape != (b, l, 2 * rw) or xdbl.dtype != torch.bfloat16:
        raise RuntimeError(f"conv_xproj: xdbl must be bf16 (batch, seqlen, {2 * rw})")
    a = N.ConvXprojArgs()
    a.batch, a.seqlen, a.dim, a.width = b, l, d, wf.shape[1]
    a.x, a.weight_f, a.bias_f, a.weight_b, a.bias_b = _ptr(x), _ptr(wf), _ptr(bf), _ptr(wb), _ptr(bb)
    a.wx_f, a.wx_b, a.y_fwd, a.y_bwd, a.xdbl = _ptr(wx_f.data), _ptr(wx_b.data), _ptr(out_f), _ptr(out_b), _ptr(xdbl)
    a.x_bs, a.x_ts, a.yf_bs, a.yf_ts = x.stride(0), x.stride(1), out_f.stride(0), out_f.stride(1)
    a.yb_bs, a.yb_ts, a.xdbl_bs, a.xdbl_ts = out_b.stride(0), out_b.stride(1), xdbl.stride(0), xdbl.stride(1)
    a.stream, a.dt_pad, a.variant = _stream(), rw - 32, int(variant)     # variant 1: always the 16-step tiles
    if lens is not None:
        lp, fn = _slot_lens(lens, b, x.device, "conv_xproj"), N.lib().cm_conv_xproj_lens
        _launch("cm_conv_xproj_lens", lambda ref: fn(ref, lp), a, units=b * l)
        return xdbl
    _launch("cm_conv_xproj", N.lib().cm_conv_xproj, a, units=b * l)
    return xdbl


def _out_rows(t, shape, dtype, device, what):
    """A caller-supplied contiguous output of the given shape and dtype (the guard-band tests place it), or a fresh one."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous() or t.device != device:
        raise RuntimeError(f"{what} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {device}")
    return t


class SlotLens:
    """Per-slot lengths that were checked once (slot_lens) for the many launches of one streamed call: the tensor, kept alive, its
    device address and what it was checked against."""
    __slots__ = ("tensor", "ptr", "batch", "device")

    def __init__(self, tensor, batch, device):
        self.tensor, self.ptr, self.batch, self.device = tensor, tensor.data_ptr(), batch, device


def slot_lens(lens, batch, device, what="lens"):
    """Per-slot lengths of a streamed launch: a contiguous int32 (batch,) tensor on the launch's device.  The kernel reads it (and
    clamps it to [0, seqlen]); nothing is read back on the host.  -> SlotLens, which the wrappers take in place of the tensor."""
    if not isinstance(lens, torch.Tensor) or lens.dtype != torch.int32 or tuple(lens.shape) != (batch,) or not lens.is_contiguous() \
            or lens.device != device:
        raise RuntimeError(f"{what}: lens must be a contiguous int32 tensor of shape ({batch},) on {device}")
    return SlotLens(lens, batch, device)


def _slot_lens(lens, batch, device, what):
    """-> the device address of the per-slot lengths: a SlotLens made for this batch and device, or a tensor checked here."""
    if type(lens) is SlotLens:
        if lens.batch != batch or lens.device != device:
            raise RuntimeError(f"{what}: lens was checked for batch {lens.batch} on {lens.device}, the launch has batch {batch} on {device}")
        return lens.ptr
    return slot_lens(lens, batch, device, what).ptr


def _hist_rows(t, shape, dtype, what):
    if t is not None and (tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous()):
        raise RuntimeError(f"{what} must be a contiguous {dtype} tensor of shape {shape}")
    return t


def conv_xproj_uni(x, weight, bias, wx, out, xdbl=None, x_hist=None, x_hist_out=None, variant: int = 0, lens=None):
    """One causal direction's depthwise conv + SiLU and x_proj GEMM in one kernel (cm_conv_xproj_uni, bf16), whole sequences
    or a stream of chunks.  x (batch, seqlen, dim) view; weight (dim, 4) fp32; wx PackedWeight of the (P + 32, dim) re-rowed
    x_proj weight; out (batch, seqlen, dim) view.  x_hist (batch, 3, dim) bf16: the rows in front of x, None = zeros;
    x_hist_out (batch, 3, dim): receives the last three rows of [x_hist | x], and must be another buffer than x_hist.
    ``lens`` (cm_conv_xproj_uni_slots): int32 (batch,) device tensor, slot b has lens[b] valid rows -- x_hist_out[b] is cut behind
    row lens[b] - 1, rows at and past it are unspecified in both outputs.  Returns xdbl (batch, seqlen, P + 32) bf16."""
    _dev_check(x, weight, bias, out, x_hist, x_hist_out)
    _rows_ok(x, "x"), _rows_ok(out, "out")
    b, l, d = x.shape
    if x.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
        raise RuntimeError("conv_xproj_uni: bf16 only")
    rw = wx.shape[0]
    if rw not in (48, 64) or wx.shape != (rw, d):
        raise RuntimeError("conv_xproj_uni: wx must be PackedWeight of shape (48 | 64, dim)")
    w, bs = _f32c(weight), _f32c(bias)
    if xdbl is None:
        xdbl = torch.empty((b, l, rw), dtype=torch.bfloat16, device=x.device)
    elif xdbl.shape != (b, l, rw) or xdbl.dtype != torch.bfloat16:
        raise RuntimeError(f"conv_xproj_uni: xdbl must be bf16 (batch, seqlen, {rw})")
    _hist_rows(x_hist, (b, 3, d), torch.bfloat16, "conv_xproj_uni: x_hist")
    _hist_rows(x_hist_out, (b, 3, d), torch.bfloat16, "conv_xproj_uni: x_hist_out")
    a = N.ConvXprojUniArgs()
    a.batch, a.seqlen, a.dim, a.width = b, l, d, w.shape[1]
    a.x, a.weight, a.bias, a.wx, a.y, a.xdbl = _ptr(x), _ptr(w), _ptr(bs), _ptr(wx.data), _ptr(out), _ptr(xdbl)
    a.x_hist, a.x_hist_out = _ptr(x_hist), _ptr(x_hist_out)
    a.x_bs, a.x_ts, a.y_bs, a.y_ts = x.stride(0), x.stride(1), out.stride(0), out.stride(1)
    a.xdbl_bs, a.xdbl_ts = xdbl.stride(0), xdbl.stride(1)
    a.stream, a.dt_pad, a.variant = _stream(), rw - 32, int(variant)     # variant 1: always the 16-step tiles
    if lens is not None:
        lp, fn = _slot_lens(lens, b, x.device, "conv_xproj_uni"), N.lib().cm_conv_xproj_uni_slots
        _launch("cm_conv_xproj_uni_slots", lambda ref: fn(ref, lp), a, units=b * l)
        return xdbl
    _launch("cm_conv_xproj_uni", N.lib().cm_conv_xproj_uni, a, units=b * l)
    return xdbl


def conv_cl_fwd(x, weight_f, bias_f, weight_b=None, bias_b=None, silu=True, out_f=None, out_b=None):
    """Channels-last depthwise conv (+SiLU) for one or both BiMamba directions in one pass (cm_conv_cl_fwd).
    x (batch, seqlen, dim) view; weights (dim, 4); returns (y_fwd, y_bwd or None)."""
    _dev_check(x, weight_f, bias_f, weight_b, bias_b)
    _rows_ok(x, "x")
    b, l, d = x.shape
    wf, bf, wb, bb = _f32c(weight_f), _f32c(bias_f), _f32c(weight_b), _f32c(bias_b)
    if out_f is None:
        out_f = torch.empty((b, l, d), dtype=x.dtype, device=x.device)
    if wb is not None and out_b is None:
        out_b = torch.empty((b, l, d), dtype=x.dtype, device=x.device)
    a = N.ConvClArgs()
    a.batch, a.seqlen, a.dim, a.width, a.io_dtype, a.silu = b, l, d, wf.shape[1], _DT[x.dtype], int(bool(silu))
    a.x, a.weight_f, a.bias_f, a.weight_b, a.bias_b = _ptr(x), _ptr(wf), _ptr(bf), _ptr(wb), _ptr(bb)
    a.y_fwd, a.y_bwd = _ptr(out_f), _ptr(out_b if wb is not None else None)
    a.x_bs, a.x_ts, a.yf_bs, a.yf_ts = x.stride(0), x.stride(1), out_f.stride(0), out_f.stride(1)
    if wb is not None:
        a.yb_bs, a.yb_ts = out_b.stride(0), out_b.stride(1)
    a.stream = _stream()
    _launch("cm_conv_cl_fwd", N.lib().cm_conv_cl_fwd, a, units=b * l)
    return out_f, (out_b if wb is not None else None)


def add_layernorm(x, y=None, alpha=1.0, norm1=None, norm2=None, x_out=None, out_dtype=None, want_out=True,
                  out_act=0, out=None):
    """r = x + alpha*y; r1 = LN1(r) if norm1 else r; x_out <- r1 (fp32, may alias x); out = LN2(r1) if norm2 else r1.
    x (rows.., dim) fp32 contiguous; norm = (weight, bias, eps); ``out``: optional contiguous tensor of x's shape in out_dtype
    to receive the result.  Returns (x_out or None, out or None)."""
    _dev_check(x, y)
    ref = x if x is not None else y
    if x is not None and (x.dtype != torch.float32 or not x.is_contiguous()):
        raise RuntimeError("add_layernorm: x must be contiguous fp32")
    od = out_dtype or torch.bfloat16
    for t, what in ((y.dtype if y is not None else None, "y"), (od if want_out else None, "out_dtype")):
        if t is not None and t not in (torch.float32, torch.bfloat16):     # cm_add_layernorm has fp32 / bf16 instances only
            raise RuntimeError(f"add_layernorm: {what} must be fp32 or bf16, not {t}")
    if x_out is not None and (x_out.dtype != torch.float32 or not x_out.is_contiguous() or x_out.numel() != ref.numel()):
        raise RuntimeError("add_layernorm: x_out must be contiguous fp32 with x's size")
    d = ref.shape[-1]
    rows = ref.numel() // d
    a = N.AddLnArgs()
    a.rows, a.dim, a.out_act = rows, d, int(out_act)
    keep = []
    if y is not None:
        if not y.is_contiguous() or y.shape != ref.shape:
            raise RuntimeError("add_layernorm: y must be contiguous with x's shape")
        a.y, a.y_dtype = _ptr(y), _DT[y.dtype]
    a.alpha = float(alpha)
    if norm1 is not None:
        g, bt = _f32c(norm1[0]), _f32c(norm1[1])
        keep += [g, bt]
        a.g1, a.b1, a.eps1 = _ptr(g), _ptr(bt), float(norm1[2])
    if norm2 is not None:
        g, bt = _f32c(norm2[0]), _f32c(norm2[1])
        keep += [g, bt]
        a.g2, a.b2, a.eps2 = _ptr(g), _ptr(bt), float(norm2[2])
    if out is not None and not want_out:
        raise RuntimeError("add_layernorm: out given with want_out=False")
    if want_out:
        out = _out_rows(out, ref.shape, od, ref.device, "add_layernorm: out")
        a.out, a.out_dtype = _ptr(out), _DT[od]
    a.x = _ptr(x)
    a.x_out = _ptr(x_out)
    a.stream = _stream()
    _launch("cm_add_layernorm", N.lib().cm_add_layernorm, a, units=rows)
    return x_out, out


def causal_conv1d_update(x, conv_state, weight, bias=None, silu=True, bufs=None):
    """Decode-time conv step (cm_causal_conv1d_update; reference bimamba.py:331-343): conv_state (batch, dim, width) fp32 is
    shifted and gets x (batch, dim) appended IN PLACE; returns out (batch, dim) in x's dtype.  bufs: a caller-placed "out"."""
    _dev_check(x, conv_state, weight, bias)
    if conv_state.dtype != torch.float32 or not conv_state.is_contiguous():
        raise RuntimeError("causal_conv1d_update: conv_state must be a contiguous fp32 (batch, dim, width) tensor")
    x = x.contiguous()
    w, bs = _f32c(weight).reshape(conv_state.shape[1], -1), _f32c(bias)
    out = _bufs(bufs, ("out",), "causal_conv1d_update")("out", x.shape, x.dtype, x.device)
    a = N.ConvUpdateArgs()
    a.batch, a.dim, a.width, a.io_dtype, a.silu = x.shape[0], x.shape[1], conv_state.shape[2], _DT[x.dtype], int(bool(silu))
    a.x, a.conv_state, a.weight, a.bias, a.out, a.stream = _ptr(x), _ptr(conv_state), _ptr(w), _ptr(bs), _ptr(out), _stream()
    _launch("cm_causal_conv1d_update", N.lib().cm_causal_conv1d_update, a, units=x.shape[0])
    return out


def selective_state_update(state, x, dt, A, B, C, D=None, z=None, dt_bias=None, dt_softplus=False, bufs=None):
    """Decode-time SSM step (cm_selective_state_update; reference bimamba.py:350-362): state (batch, dim, dstate) fp32 is
    updated IN PLACE; x, dt, z (batch, dim), B, C (batch, dstate) share one dtype; returns y (batch, dim).  bufs: a
    caller-placed "out"."""
    _dev_check(state, x, dt, A, B, C, D, z, dt_bias)
    if state.dtype != torch.float32 or not state.is_contiguous():
        raise RuntimeError("selective_state_update: state must be a contiguous fp32 (batch, dim, dstate) tensor")
    x = x.contiguous()
    dt, B, C = dt.to(x.dtype).contiguous(), B.to(x.dtype).contiguous(), C.to(x.dtype).contiguous()
    z = None if z is None else z.to(x.dtype).contiguous()
    A, D, dt_bias = _f32c(A), _f32c(D), _f32c(dt_bias)
    out = _bufs(bufs, ("out",), "selective_state_update")("out", x.shape, x.dtype, x.device)
    a = N.StateUpdateArgs()
    a.batch, a.dim, a.dstate, a.io_dtype, a.dt_softplus = x.shape[0], x.shape[1], state.shape[2], _DT[x.dtype], int(bool(dt_softplus))
    a.state, a.x, a.dt, a.A, a.B, a.C, a.D, a.z, a.dt_bias, a.out = (_ptr(state), _ptr(x), _ptr(dt), _ptr(A), _ptr(B), _ptr(C), _ptr(D),
                                                                     _ptr(z), _ptr(dt_bias), _ptr(out))
    a.stream = _stream()
    _launch("cm_selective_state_update", N.lib().cm_selective_state_update, a, units=x.shape[0])
    return out


def mamba_step_supported(d_inner: int, d_state: int, d_conv: int, dt_rank: int, dtype) -> bool:
    """The shapes cm_mamba_step is built for (include/conmamba_hip.h)."""
    return (d_state == 16 and d_conv == 4 and d_inner % 8 == 0 and 8 <= d_inner <= 4096 and 1 <= dt_rank <= 32
            and dtype in (torch.float32, torch.bfloat16))


def mamba_step(xz, conv_state, ssm_state, conv_weight, conv_bias, x_proj_weight, dt_proj_weight, dt_bias, A, D, bufs=None):
    """One mixer decoding step between in_proj and out_proj in one launch (cm_mamba_step; reference bimamba.py:331-362):
    xz (batch, 2 * dim) in fp32 / bf16; conv_state (batch, dim, 4) and ssm_state (batch, dim, 16), fp32, updated IN PLACE;
    conv_weight (dim, 4), x_proj_weight (dt_rank + 32, dim), dt_proj_weight (dim, dt_rank), A = -exp(A_log) (dim, 16), conv_bias,
    dt_bias, D (dim) or None -- all used in fp32.  Returns y (batch, dim) in xz's dtype.  A shape the kernel is not built
    for raises (code -2): nothing is launched.  bufs: a caller-placed "out"."""
    _dev_check(xz, conv_state, ssm_state, conv_weight, conv_bias, x_proj_weight, dt_proj_weight, dt_bias, A, D)
    if xz.dim() != 2 or xz.shape[1] % 2:
        raise RuntimeError("mamba_step: xz must be (batch, 2 * dim)")
    batch, dim = xz.shape[0], xz.shape[1] // 2
    for t, what in ((conv_state, "conv_state"), (ssm_state, "ssm_state")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 3 or tuple(t.shape[:2]) != (batch, dim):
            raise RuntimeError(f"mamba_step: {what} must be a contiguous fp32 (batch, dim, width) tensor")
    if xz.dtype not in _DT:
        raise RuntimeError(f"mamba_step: unsupported dtype {xz.dtype}")
    xz = xz.contiguous()
    cw, cb, wx, wdt = _f32c(conv_weight).reshape(dim, -1), _f32c(conv_bias), _f32c(x_proj_weight), _f32c(dt_proj_weight)
    dt_bias, A, D = _f32c(dt_bias), _f32c(A), _f32c(D)
    a = N.MambaStepArgs()
    a.batch, a.dim, a.dstate, a.dconv, a.dt_rank, a.io_dtype = batch, dim, ssm_state.shape[2], conv_state.shape[2], wdt.shape[1], _DT[xz.dtype]
    if cw.shape != (dim, a.dconv) or wx.shape != (a.dt_rank + 2 * a.dstate, dim) or wdt.shape[0] != dim or A.shape != (dim, a.dstate):
        raise RuntimeError("mamba_step: weight shapes do not match the states")
    out = _bufs(bufs, ("out",), "mamba_step")("out", (batch, dim), xz.dtype, xz.device)
    a.xz, a.conv_state, a.ssm_state, a.out = _ptr(xz), _ptr(conv_state), _ptr(ssm_state), _ptr(out)
    a.conv_weight, a.conv_bias, a.x_proj_weight, a.dt_proj_weight = _ptr(cw), _ptr(cb), _ptr(wx), _ptr(wdt)
    a.dt_bias, a.A, a.D, a.stream = _ptr(dt_bias), _ptr(A), _ptr(D), _stream()
    _launch("cm_mamba_step", N.lib().cm_mamba_step, a, units=batch)
    return out


def _dwconv_args(x, weight, bias, pad_left):
    _dev_check(x, weight, bias)
    x = _time_contig(x)
    if x.dim() != 3:
        raise RuntimeError("dwconv1d: x must be (batch, dim, seqlen)")
    w = _f32c(weight).reshape(x.shape[1], -1)
    bs = _f32c(bias)
    a = N.Dwconv1dArgs()
    a.batch, a.dim, a.seqlen, a.ksize, a.pad_left, a.io_dtype = x.shape[0], x.shape[1], x.shape[2], w.shape[1], int(pad_left), _DT[x.dtype]
    a.x, a.weight, a.bias, a.x_bs, a.x_ds = _ptr(x), _ptr(w), _ptr(bs), x.stride(0), x.stride(1)
    a.stream = _stream()
    return a, x, w, bs


def dwconv1d_fwd(x, weight, bias=None, pad_left=None):
    """Depthwise Conv1d over time (cm_dwconv1d_fwd): x (batch, dim, seqlen), weight (dim, 1, k) or (dim, k), zero
    padding with ``pad_left`` zeros in front (default k // 2 = 'same'); returns y of the same shape."""
    k = weight.shape[-1]
    a, x, w, bs = _dwconv_args(x, weight, bias, k // 2 if pad_left is None else pad_left)
    y = torch.empty_like(x, memory_format=torch.contiguous_format)
    a.y, a.y_bs, a.y_ds = _ptr(y), y.stride(0), y.stride(1)
    _launch("cm_dwconv1d_fwd", N.lib().cm_dwconv1d_fwd, a, units=x.shape[0] * x.shape[2])
    return y


def dwconv1d_bwd(x, weight, dy, has_bias=True, pad_left=None):
    """-> (dx, dweight (dim, k) fp32, dbias (dim) fp32 or None) of dwconv1d_fwd (cm_dwconv1d_bwd)."""
    k = weight.shape[-1]
    a, x, w, _ = _dwconv_args(x, weight, None, k // 2 if pad_left is None else pad_left)
    _dev_check(dy)
    dy = _time_contig(dy)
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise RuntimeError("dwconv1d_bwd: dy must match x in shape and dtype")
    dx = torch.empty_like(x, memory_format=torch.contiguous_format)
    dw = torch.zeros_like(w)
    db = torch.zeros((x.shape[1],), dtype=torch.float32, device=x.device) if has_bias else None
    a.dy, a.dy_bs, a.dy_ds, a.dx, a.dx_bs, a.dx_ds = _ptr(dy), dy.stride(0), dy.stride(1), _ptr(dx), dx.stride(0), dx.stride(1)
    a.dweight, a.dbias = _ptr(dw), _ptr(db)
    _launch("cm_dwconv1d_bwd", N.lib().cm_dwconv1d_bwd, a, units=x.shape[0] * x.shape[2])
    return dx, dw, db


class DepthwiseConv1dFn(torch.autograd.Function):
    """autograd node over cm_dwconv1d_fwd / _bwd (drop-in for the depthwise nn.Conv1d of the ConvolutionModule)."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad_left):
        ctx.save_for_backward(x, weight)
        ctx.has_bias, ctx.pad_left = bias is not None, pad_left
        return dwconv1d_fwd(x, weight, bias, pad_left)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw, db = dwconv1d_bwd(x, weight, dy.to(x.dtype), ctx.has_bias, ctx.pad_left)
        return dx, dw.reshape(weight.shape).to(weight.dtype), (db.to(weight.dtype) if db is not None else None), None


def _dwconv_cl_args(x, weight, bias, pad_left):
    _dev_check(x, weight, bias)
    _rows_ok(x, "x")
    w = _f32c(weight).reshape(x.shape[2], -1)
    bs = _f32c(bias)
    a = N.DwconvClArgs()
    a.batch, a.seqlen, a.dim, a.ksize, a.pad_left, a.io_dtype = x.shape[0], x.shape[1], x.shape[2], w.shape[1], int(pad_left), _DT[x.dtype]
    a.x, a.weight, a.bias, a.x_bs, a.x_ts = _ptr(x), _ptr(w), _ptr(bs), x.stride(0), x.stride(1)
    a.stream = _stream()
    return a, w, bs


def dwconv_cl_fwd(x, weight, bias=None, pad_left=None, bufs=None):
    """Depthwise Conv1d over time on channels-last rows (cm_dwconv_cl_fwd): x (batch, seqlen, dim), channel axis
    contiguous; weight (dim, 1, k) or (dim, k); returns y (batch, seqlen, dim).  ``bufs``: a caller-supplied ``y`` (any view with
    the channel axis contiguous)."""
    k = weight.shape[-1]
    a, w, bs = _dwconv_cl_args(x, weight, bias, k // 2 if pad_left is None else pad_left)
    y = _bufs(bufs, ("y",), "dwconv_cl_fwd")("y", x.shape, x.dtype, x.device, rows3=True)
    a.y, a.y_bs, a.y_ts = _ptr(y), y.stride(0), y.stride(1)
    _launch("cm_dwconv_cl_fwd", N.lib().cm_dwconv_cl_fwd, a, units=x.shape[0] * x.shape[1])
    return y


def dwconv_cl_bwd(x, weight, dy, has_bias=True, pad_left=None, bufs=None):
    """-> (dx, dweight (dim, k) fp32, dbias (dim) fp32 or None) of dwconv_cl_fwd (cm_dwconv_cl_bwd, deterministic).
    ``bufs``: caller-supplied ``dx`` (any view with the channel axis contiguous), ``dweight``, ``dbias`` and ``partial``
    (cm_dwconv_cl_workspace_floats)."""
    k = weight.shape[-1]
    a, w, _ = _dwconv_cl_args(x, weight, None, k // 2 if pad_left is None else pad_left)
    _dev_check(dy)
    if dy.stride(2) != 1:
        dy = dy.contiguous()
    if dy.dtype != x.dtype or dy.shape != x.shape:
        raise RuntimeError("dwconv_cl_bwd: dy must match x in shape and dtype")
    take = _bufs(bufs, ("dx", "dweight", "dbias", "partial"), "dwconv_cl_bwd")
    dx = take("dx", x.shape, x.dtype, x.device, rows3=True)
    dw = take("dweight", w.shape, torch.float32, x.device)
    db = take("dbias", (x.shape[2],), torch.float32, x.device) if has_bias else None
    a.overwrite = 1
    part = take("partial", (N.lib().cm_dwconv_cl_workspace_floats(x.shape[0], x.shape[1], x.shape[2]),), torch.float32, x.device)
    a.dy, a.dy_bs, a.dy_ts, a.dx, a.dx_bs, a.dx_ts = _ptr(dy), dy.stride(0), dy.stride(1), _ptr(dx), dx.stride(0), dx.stride(1)
    a.dweight, a.dbias, a.partial = _ptr(dw), _ptr(db), _ptr(part)
    _launch("cm_dwconv_cl_bwd", N.lib().cm_dwconv_cl_bwd, a, units=x.shape[0] * x.shape[1])
    return dx, dw, db


class DepthwiseConvClFn(torch.autograd.Function):
    """autograd node over cm_dwconv_cl_fwd / _bwd: the ConvolutionModule's depthwise conv on (batch, time, channel) rows."""

    @staticmethod
    def forward(ctx, x, weight, bias, pad_left):
        ctx.save_for_backward(x, weight)
        ctx.has_bias, ctx.pad_left = bias is not None, pad_left
        return dwconv_cl_fwd(x, weight, bias, pad_left)

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dx, dw, db = dwconv_cl_bwd(x, weight, dy.to(x.dtype), ctx.has_bias, ctx.pad_left)
        return dx, dw.reshape(weight.shape).to(weight.dtype), (db.to(weight.dtype) if db is not None else None), None


def _layernorm_args(x2, weight, eps, y_dtype):
    a = N.LayerNormArgs()
    a.rows, a.dim, a.x_dtype, a.y_dtype, a.eps = x2.shape[0], x2.shape[1], _DT[x2.dtype], _DT[y_dtype], float(eps)
    a.x, a.gamma, a.stream = _ptr(x2), _ptr(weight), _stream()
    return a


def _ln_epilogue(a, x2, leaky_slope, chan_mask, mask_rows):
    """Fill the optional activation + channel-mask epilogue of cm_layernorm_args."""
    if leaky_slope is not None:
        a.act, a.act_slope = 1, float(leaky_slope)
    if chan_mask is not None:
        _dev_check(chan_mask)
        if chan_mask.dtype != torch.float32 or not chan_mask.is_contiguous() or chan_mask.dim() != 2:
            raise RuntimeError("layernorm: chan_mask must be a contiguous fp32 (groups, channels) tensor")
        c = chan_mask.shape[1]
        if c % 4 or x2.shape[1] % c or x2.shape[0] != chan_mask.shape[0] * mask_rows:
            raise RuntimeError("layernorm: chan_mask (groups, channels) needs channels % 4 == 0, dim % channels == 0, rows == groups * mask_rows")
        a.chan_mask, a.mask_rows, a.mask_c = _ptr(chan_mask), int(mask_rows), c


def layernorm_fwd(x, weight, bias, eps, out_dtype=None, leaky_slope=None, chan_mask=None, mask_rows=1, bufs=None):
    """LayerNorm over the last axis (cm_layernorm_fwd) -> (y, mean, rstd); x fp32 or bf16, contiguous rows; y in
    `out_dtype` (default fp32: what torch's autocast gives, reference modules/Conmamba.py:597-620).  ``bufs``: caller-supplied ``y`` (rows, dim)
    and ``mean`` ((2, rows): [mean | rstd], the one statistics tensor returned)."""
    _dev_check(x, weight, bias)
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"layernorm_fwd: unsupported dtype {x.dtype}")
    x2 = x.reshape(-1, x.shape[-1])
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out_dtype = out_dtype or torch.float32
    w, b = weight.detach().float().contiguous(), bias.detach().float().contiguous()
    take = _bufs(bufs, ("y", "mean"), "layernorm_fwd")
    y = take("y", x2.shape, out_dtype, x.device)
    stats = take("mean", (2, x2.shape[0]), torch.float32, x.device)
    a = _layernorm_args(x2, w, eps, out_dtype)
    a.beta, a.y, a.mean, a.rstd = _ptr(b), _ptr(y), _ptr(stats[0]), _ptr(stats[1])
    _ln_epilogue(a, x2, leaky_slope, chan_mask, mask_rows)
    _launch("cm_layernorm_fwd", N.lib().cm_layernorm_fwd, a, units=x2.shape[0])
    return y.view(x.shape), x2, stats


def layernorm_bwd(dy, x2, stats, weight, eps, need_dx=True, dres=None, bias=None, leaky_slope=None, chan_mask=None, mask_rows=1,
                  bufs=None):
    """-> (dx (x2's dtype and shape) or None, dgamma, dbeta (dim) fp32) of layernorm_fwd (cm_layernorm_bwd, deterministic).
    ``dres`` (fp32, x2's shape; fp32 x2, dim <= 1024): added to dx in the same pass (the residual branch's gradient).
    ``bufs``: caller-supplied ``dx``, ``dgamma`` ((2, dim): [dgamma | dbeta], the one tensor both are returned from) and
    ``workspace`` (cm_layernorm_bwd_workspace_floats)."""
    _dev_check(dy, x2, stats, weight)
    dy2 = dy.reshape(x2.shape)
    if not dy2.is_contiguous():
        dy2 = dy2.contiguous()
    w = weight.detach().float().contiguous()
    take = _bufs(bufs, ("dx", "dgamma", "workspace"), "layernorm_bwd")
    dx = (torch.empty_like(x2) if bufs is None else take("dx", x2.shape, x2.dtype, x2.device)) if need_dx else None
    dgb = take("dgamma", (2, x2.shape[1]), torch.float32, x2.device)
    ws = take("workspace", (N.lib().cm_layernorm_bwd_workspace_floats(x2.shape[0], x2.shape[1]),), torch.float32, x2.device)
    a = _layernorm_args(x2, w, eps, dy2.dtype)
    a.mean, a.rstd, a.dy, a.dx = _ptr(stats[0]), _ptr(stats[1]), _ptr(dy2), _ptr(dx)
    a.dgamma, a.dbeta, a.workspace = _ptr(dgb[0]), _ptr(dgb[1]), _ptr(ws)
    if leaky_slope is not None or chan_mask is not None:
        bb = bias.detach().float().contiguous()                   # the activation's derivative needs LN's output: beta
        a.beta = _ptr(bb)
        _ln_epilogue(a, x2, leaky_slope, chan_mask, mask_rows)
    fused_res = dres is not None and need_dx and x2.dtype == torch.float32 and x2.shape[1] <= 1024
    if fused_res:
        _dev_check(dres)
        if dres.dtype != torch.float32 or not dres.is_contiguous() or dres.shape != x2.shape:
            raise RuntimeError("layernorm_bwd: dres must be a contiguous fp32 tensor of x2's shape")
        a.dres = _ptr(dres)
    _launch("cm_layernorm_bwd", N.lib().cm_layernorm_bwd, a, units=x2.shape[0])
    if dres is not None and need_dx and not fused_res:
        dx = dx + dres
    return dx, dgb[0], dgb[1]


class LayerNormFn(torch.autograd.Function):
    """autograd node over cm_layernorm_fwd / _bwd.  Output fp32 under autocast or for fp32 input (torch's rule), else the
    input dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, low_dtype=None):
        out_dtype = torch.float32 if (x.dtype == torch.float32 or torch.is_autocast_enabled("cuda")) else x.dtype
        if low_dtype is not None:                             # the consumer is a projection that would round to low_dtype anyway
            out_dtype = low_dtype
        y, x2, stats = layernorm_fwd(x, weight, bias, eps, out_dtype)
        ctx.save_for_backward(x2, stats, weight)
        ctx.eps, ctx.shape = eps, x.shape
        return y

    @staticmethod
    def backward(ctx, dy):
        x2, stats, weight = ctx.saved_tensors
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        dx, dg, db = layernorm_bwd(dy, x2, stats, weight, ctx.eps, need_dx=ctx.needs_input_grad[0])
        return (dx.view(ctx.shape) if dx is not None else None), dg.to(weight.dtype), db.to(weight.dtype), None, None


class LnActDropFn(torch.autograd.Function):
    """y = LeakyReLU(LayerNorm(x)) * chan_mask -- the tail of a front-end Conv2d block (LayerNorm over (freq, channel) -> LeakyReLU ->
    Dropout2d with one factor per (sample, channel)) as ONE kernel forward and ONE backward (cm_layernorm_fwd / _bwd with the
    epilogue fields).  x (batch, time, freq, channel) contiguous; weight / bias (freq * channel); chan_mask (batch, channel) fp32 with
    the 1 / keep scale folded in, or None.  ``out_dtype``: what the consumer (the next Conv2d / Linear under autocast) rounds to anyway:
    the fp32 result is rounded once, here."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, slope, chan_mask, out_dtype):
        b, t, f, c = x.shape
        x2 = x.reshape(b * t, f * c)
        y, x2s, stats = layernorm_fwd(x2, weight, bias, eps, out_dtype, leaky_slope=slope, chan_mask=chan_mask, mask_rows=t)
        ctx.save_for_backward(x2s, stats, weight, bias, chan_mask if chan_mask is not None else weight.new_empty(0))
        ctx.cfg = (eps, slope, t, chan_mask is not None, x.shape)
        return y.view(x.shape)

    @staticmethod
    def backward(ctx, dy):
        x2, stats, weight, bias, mask = ctx.saved_tensors
        eps, slope, t, has_mask, shape = ctx.cfg
        if dy.dtype not in (torch.float32, torch.bfloat16):
            dy = dy.float()
        dy = dy if dy.is_contiguous() else dy.contiguous()
        dx, dg, db = layernorm_bwd(dy.view(x2.shape[0], -1), x2, stats, weight, eps, need_dx=ctx.needs_input_grad[0], bias=bias, leaky_slope=slope,
                                   chan_mask=mask if has_mask else None, mask_rows=t)
        return (dx.view(shape) if dx is not None else None), dg.to(weight.dtype), db.to(weight.dtype), None, None, None, None


def ln_pw_glu(x, y, alpha, norm, w, bias, x_out=None, ycat=None, out_w=None, out=None):
    """Mixer -> convolution-module seam (cm_ln_pw_glu): x_out = x + alpha*y; g = GLU(LayerNorm(x_out) @ W^T + bias).
    x (rows, D) fp32 contiguous, D = 256 or 144; y (rows, D) bf16 or None; norm = (weight, bias, eps); w: PackedWeight of the
    (2D, D) pointwise-conv weight (at D = 144 padded to 160 columns: PackedWeight(w, pad=(288, 160))); bias (2D) fp32.  x_out defaults
    to x (in place).  Returns g (rows, D) bf16 (``out`` if given: a contiguous bf16 (rows, D) tensor).
    With ``ycat`` (rows, K) bf16 contiguous and ``out_w`` (PackedWeight of a (256, K) matrix, K a multiple of 128) instead of
    ``y``, y = ycat @ out_w^T is formed inside the kernel (cm_ln_pw_glu_mix, D = 256 only) and never written."""
    _dev_check(x, y, bias, ycat)
    rows, d = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous() or d not in (256, 144):
        raise RuntimeError("ln_pw_glu: x must be a contiguous fp32 (rows, 256) or (rows, 144) tensor")
    if y is not None and (y.dtype != torch.bfloat16 or not y.is_contiguous() or y.shape != x.shape):
        raise RuntimeError("ln_pw_glu: y must be a contiguous bf16 tensor shaped like x")
    if not isinstance(w, PackedWeight) or w.layout != 16 or w.shape != (2 * d, d) or w.padded != (2 * d, _kpad(d)):
        raise RuntimeError("ln_pw_glu: w must be a PackedWeight (16-row tiles) of shape (2D, D), at D = 144 padded to (288, 160)")
    if d != 256 and ycat is not None:
        raise RuntimeError("ln_pw_glu: the projection in front (ycat, out_w) needs d_model 256")
    g_, b_, bs = _f32c(norm[0]), _f32c(norm[1]), _f32c(bias)
    xo = x if x_out is None else x_out
    out = _out_rows(out, (rows, d), torch.bfloat16, x.device, "ln_pw_glu: out")
    if (ycat is None) != (out_w is None) or (ycat is not None and y is not None):
        raise RuntimeError("ln_pw_glu: give either y, or ycat together with out_w")
    if ycat is not None:
        if ycat.dtype != torch.bfloat16 or not ycat.is_contiguous() or ycat.dim() != 2 or ycat.shape[0] != rows:
            raise RuntimeError("ln_pw_glu: ycat must be a contiguous bf16 (rows, K) tensor")
        if not isinstance(out_w, PackedWeight) or out_w.layout != 16 or out_w.shape != (256, ycat.shape[1]):
            raise RuntimeError("ln_pw_glu: out_w must be a PackedWeight (16-row tiles) of shape (256, K)")
        m = N.LnPwGluMixArgs()
        m.rows, m.dim, m.x, m.ln_g, m.ln_b, m.w, m.bias = rows, d, _ptr(x), _ptr(g_), _ptr(b_), _ptr(w.data), _ptr(bs)
        m.x_out, m.out, m.alpha, m.eps, m.stream = _ptr(xo), _ptr(out), float(alpha), float(norm[2]), _stream()
        m.ycat, m.proj_w, m.proj_k = _ptr(ycat), _ptr(out_w.data), ycat.shape[1]
        _launch("cm_ln_pw_glu", N.lib().cm_ln_pw_glu_mix, m, units=rows)     # the same kernel with a phase in front
        return out
    a = N.LnPwGluArgs()
    a.rows, a.dim, a.x, a.y, a.ln_g, a.ln_b, a.w, a.bias = rows, d, _ptr(x), _ptr(y), _ptr(g_), _ptr(b_), _ptr(w.data), _ptr(bs)
    a.x_out, a.out, a.alpha, a.eps, a.stream = _ptr(xo), _ptr(out), float(alpha), float(norm[2]), _stream()
    _launch("cm_ln_pw_glu", N.lib().cm_ln_pw_glu, a, units=rows)
    return out


def glu_dwconv_ln_gelu(inp, weight, bias, ln_weight, ln_bias, eps=1e-5, weight_t=None, glu_done=False, lin_w=None, lin_b=None,
                       variant: int = 0, causal: bool = False, hist=None, hist_out=None, out=None, lens=None):
    """(batch, seqlen, 2*dim) -> (batch, seqlen, dim): GLU, depthwise conv (k=31, same padding), LayerNorm, GELU
    (cm_glu_dwconv_ln_gelu).  weight (dim, 1, k) or (dim, k); weight_t: optional precomputed fp32 (k, dim) copy of the
    taps (made here per call otherwise) so that the kernel's per-channel tap reads are coalesced.
    ``causal`` (cm_glu_dwconv_ln_gelu_causal): all k - 1 padding rows in front; hist (batch, k - 1, dim) in inp's dtype are
    the gated rows in front of inp (None = zeros), hist_out (another buffer than hist) receives the last k - 1 gated rows of
    [hist | inp].  ``lens`` (cm_glu_dwconv_ln_gelu_causal_slots): int32 (batch,) device tensor, slot b has lens[b] valid rows --
    hist_out[b] is cut behind gated row lens[b] - 1, output rows at and past it are unspecified.  ``lens`` without ``causal``
    (cm_glu_dwconv_ln_gelu_lens): utterance b has lens[b] rows, the 'same' padding starts behind its own last row, output rows at and
    past lens[b] are not written.
    ``out``: optional contiguous (batch, seqlen, dim) tensor in inp's dtype to receive the result."""
    _dev_check(inp, weight, bias, ln_weight, ln_bias, hist, hist_out)
    if (hist is not None or hist_out is not None) and not causal:
        raise RuntimeError("glu_dwconv_ln_gelu: hist / hist_out belong to the causal form")
    if not inp.is_contiguous():
        inp = inp.contiguous()
    b, l, d2 = inp.shape
    d = d2 if glu_done else d2 // 2                       # glu_done: the input is already gated (cm_ln_pw_glu), dim wide
    w = _f32c(weight).reshape(d, -1)
    bs, g, bt = _f32c(bias), _f32c(ln_weight), _f32c(ln_bias)
    out = _out_rows(out, (b, l, d), inp.dtype, inp.device, "glu_dwconv_ln_gelu: out")
    a = N.GluDwconvCausalArgs() if causal else N.GluDwconvArgs()
    if causal:
        hs = (b, w.shape[1] - 1, d)
        a.hist, a.hist_out = _ptr(_hist_rows(hist, hs, inp.dtype, "glu_dwconv_ln_gelu: hist")), _ptr(_hist_rows(hist_out, hs, inp.dtype, "glu_dwconv_ln_gelu: hist_out"))
    a.batch, a.seqlen, a.dim, a.ksize, a.io_dtype, a.glu_done = b, l, d, w.shape[1], _DT[inp.dtype], int(bool(glu_done))
    a.in_, a.weight, a.bias, a.ln_g, a.ln_b, a.eps, a.out = _ptr(inp), _ptr(w), _ptr(bs), _ptr(g), _ptr(bt), float(eps), _ptr(out)
    wt = w.t().contiguous() if weight_t is None else weight_t
    if wt.dtype != torch.float32 or wt.shape != (w.shape[1], d) or not wt.is_contiguous():
        raise RuntimeError("glu_dwconv_ln_gelu: weight_t must be a contiguous fp32 (k, dim) tensor")
    a.weight_t = _ptr(wt)
    if lin_w is not None:                                 # closing Linear(dim, dim) of the module, applied in the same kernel
        if not isinstance(lin_w, PackedWeight) or lin_w.shape != (d, d) or lin_b is None:
            raise RuntimeError("glu_dwconv_ln_gelu: lin_w must be a PackedWeight of shape (dim, dim), with lin_b")
        lb = _f32c(lin_b)
        a.lin_w, a.lin_b = _ptr(lin_w.data), _ptr(lb)
    a.stream, a.variant = _stream(), int(variant)        # variant 1: always the generic 16-step kernel
    if lens is not None and not causal:
        lp, fn = _slot_lens(lens, b, inp.device, "glu_dwconv_ln_gelu"), N.lib().cm_glu_dwconv_ln_gelu_lens
        _launch("cm_glu_dwconv_ln_gelu_lens", lambda ref: fn(ref, lp), a, units=b * l)
    elif lens is not None:
        lp, fn = _slot_lens(lens, b, inp.device, "glu_dwconv_ln_gelu"), N.lib().cm_glu_dwconv_ln_gelu_causal_slots
        _launch("cm_glu_dwconv_ln_gelu_causal_slots", lambda ref: fn(ref, lp), a, units=b * l)
    elif causal:
        _launch("cm_glu_dwconv_ln_gelu_causal", N.lib().cm_glu_dwconv_ln_gelu_causal, a, units=b * l)
    else:
        _launch("cm_glu_dwconv_ln_gelu", N.lib().cm_glu_dwconv_ln_gelu, a, units=b * l)
    return out


def cnn_block1(feats, weight, bias, ln_weight, ln_bias, eps=1e-5, slope=0.01, out_dtype=torch.bfloat16, pad_out=1):
    """feats (batch, T, F) fp32 -> (batch, ceil(T/2) + 2*pad_out, ceil(F/2) + 2*pad_out, C): 3x3 stride-2 conv, LayerNorm
    over (freq, channel), LeakyReLU, with the reflect border of the next 3x3 block already in place (cm_cnn_block1)."""
    _dev_check(feats, weight, bias, ln_weight, ln_bias)
    feats = feats.float().contiguous()
    b, t, f = feats.shape
    w, bs, g, bt = _f32c(weight), _f32c(bias), _f32c(ln_weight), _f32c(ln_bias)
    cch = w.shape[0]
    t1, f1 = (t + 1) // 2, (f + 1) // 2
    out = torch.empty((b, t1 + 2 * pad_out, f1 + 2 * pad_out, cch), dtype=out_dtype, device=feats.device)
    a = N.CnnBlock1Args()
    a.batch, a.T, a.F, a.C, a.io_dtype, a.pad_out = b, t, f, cch, _DT[out_dtype], pad_out
    a.feats, a.weight, a.bias, a.ln_g, a.ln_b, a.eps, a.slope, a.out = (_ptr(feats), _ptr(w), _ptr(bs), _ptr(g), _ptr(bt),
                                                                          float(eps), float(slope), _ptr(out))
    a.stream = _stream()
    _launch("cm_cnn_block1", N.lib().cm_cnn_block1, a, units=b * t)
    return out


def cnn_front_supported(feats, w1, w2_ohwi) -> bool:
    return (feats.shape[-1] == 80 and tuple(w1.shape) == (64, 1, 3, 3) and tuple(w2_ohwi.shape) == (32, 3, 3, 64)
            and w2_ohwi.dtype == torch.bfloat16 and feats.shape[1] >= 5)


def cnn_front(feats, w1, b1, ln1_w, ln1_b, eps1, w2_ohwi, b2, ln2_w, ln2_b, eps2, slope=0.01, lens=None, out=None):
    """feats (batch, T, 80) fp32 -> (batch, T2, 640) bf16: both ConvolutionFrontEnd blocks in one kernel (cm_cnn_front).
    ``lens`` (cm_cnn_front_lens): int32 (batch,) device tensor of FRAME counts, utterance b has lens[b] frames and
    ceil(ceil(lens[b] / 2) / 2) rows -- both reflections at its own ends, rows past its own not written, frames past its own not read.
    ``out``: optional contiguous (batch, T2, 640) bf16 tensor to receive the result."""
    _dev_check(feats, w1, b1, ln1_w, ln1_b, w2_ohwi, b2, ln2_w, ln2_b)
    feats = feats.float().contiguous()
    if not cnn_front_supported(feats, w1, w2_ohwi) or not w2_ohwi.is_contiguous():
        raise RuntimeError("cnn_front: needs 80 bins, a (64, 1, 3, 3) first conv and a contiguous bf16 (32, 3, 3, 64) second conv")
    b, t, f = feats.shape
    t1 = (t + 1) // 2
    t2 = (t1 - 1) // 2 + 1
    w1f, b1f, g1, bt1 = _f32c(w1), _f32c(b1), _f32c(ln1_w).reshape(-1), _f32c(ln1_b).reshape(-1)
    b2f, g2, bt2 = _f32c(b2), _f32c(ln2_w).reshape(-1), _f32c(ln2_b).reshape(-1)
    if g1.numel() != 40 * 64 or g2.numel() != 20 * 32:
        raise RuntimeError("cnn_front: LayerNorm parameters must have 40*64 and 20*32 elements")
    out = _out_rows(out, (b, t2, 640), torch.bfloat16, feats.device, "cnn_front: out")
    a = N.CnnFrontArgs()
    a.batch, a.T, a.F, a.C1, a.C2 = b, t, f, 64, 32
    a.feats, a.w1, a.b1, a.ln1_g, a.ln1_b = _ptr(feats), _ptr(w1f), _ptr(b1f), _ptr(g1), _ptr(bt1)
    a.w2, a.b2, a.ln2_g, a.ln2_b = _ptr(w2_ohwi), _ptr(b2f), _ptr(g2), _ptr(bt2)
    a.eps1, a.eps2, a.slope, a.out, a.stream = float(eps1), float(eps2), float(slope), _ptr(out), _stream()
    if lens is not None:
        lp, fn = _slot_lens(lens, b, feats.device, "cnn_front"), N.lib().cm_cnn_front_lens
        _launch("cm_cnn_front_lens", lambda ref: fn(ref, lp), a, units=b * t)
        return out
    _launch("cm_cnn_front", N.lib().cm_cnn_front, a, units=b * t)
    return out


def cnn_block2(y1, weight_ohwi, bias, ln_weight, ln_bias, eps=1e-5, slope=0.01):
    """y1 (batch, T_in, F_in, 64) bf16 channels-last (cnn_block1 output with its reflect border) ->
    (batch, T2, F2*32) bf16: 3x3 stride-2 conv 64 -> 32, LayerNorm over (freq, channel), LeakyReLU (cm_cnn_block2).
    weight_ohwi: (32, 3, 3, 64) bf16 contiguous (a Conv2d weight permuted to output, row, column, input)."""
    _dev_check(y1, weight_ohwi, bias, ln_weight, ln_bias)
    if y1.dtype != torch.bfloat16 or not y1.is_contiguous() or y1.dim() != 4:
        raise RuntimeError("cnn_block2: input must be a contiguous bf16 (batch, T, F, C) tensor")
    if weight_ohwi.dtype != torch.bfloat16 or not weight_ohwi.is_contiguous() or weight_ohwi.dim() != 4:
        raise RuntimeError("cnn_block2: weight must be a contiguous bf16 (C_out, 3, 3, C_in) tensor")
    b, t, f, cin = y1.shape
    cout = weight_ohwi.shape[0]
    if tuple(weight_ohwi.shape[1:]) != (3, 3, cin):
        raise RuntimeError("cnn_block2: weight shape does not match the input channels / 3x3 taps")
    t2, f2 = (t - 3) // 2 + 1, (f - 3) // 2 + 1
    bs, g, bt = _f32c(bias), _f32c(ln_weight).reshape(-1), _f32c(ln_bias).reshape(-1)
    if g.numel() != f2 * cout or bt.numel() != f2 * cout:
        raise RuntimeError("cnn_block2: LayerNorm parameters must have F2 * C_out elements")
    out = torch.empty((b, t2, f2 * cout), dtype=torch.bfloat16, device=y1.device)
    a = N.CnnBlock2Args()
    a.batch, a.T_in, a.F_in, a.C_in, a.C_out = b, t, f, cin, cout
    a.in_, a.weight, a.bias, a.ln_g, a.ln_b, a.eps, a.slope, a.out = (_ptr(y1), _ptr(weight_ohwi), _ptr(bs), _ptr(g), _ptr(bt),
                                                                      float(eps), float(slope), _ptr(out))
    a.stream = _stream()
    _launch("cm_cnn_block2", N.lib().cm_cnn_block2, a, units=b * t2)
    return out


def gemm_supported(m: int, n: int, k: int, epilogue: int) -> bool:
    return k % 64 == 0 and n % 256 == 0 and (epilogue != 2 or n == 256)


def gemm_bf16(a, w, bias=None, epilogue=0, x=None, alpha=1.0, norm1=None, norm2=None, want_out=True, out=None):
    """acc = a @ w.T (a (M, K) bf16 row view, w (N, K) bf16) with a fused epilogue (cm_gemm_bf16):
    0: + bias -> bf16;  1: gelu(+ bias) -> bf16;  2: x += alpha*(acc + bias) [optional LN1 into x], out = LN2(x) bf16.
    bias / LayerNorm parameters are fp32 tensors; norm = (weight, bias, eps); ``out``: optional contiguous bf16 (M, N) tensor to
    receive the result.  Returns out (or None)."""
    _dev_check(a, w, bias, x)
    if a.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or a.dim() != 2 or a.stride(1) != 1 or not w.is_contiguous():
        raise RuntimeError("gemm_bf16: a must be a (M, K) bf16 row-major view and w a contiguous (N, K) bf16 tensor")
    m, k = a.shape
    n = w.shape[0]
    g = N.GemmArgs()
    g.M, g.N, g.K, g.epilogue = m, n, k, epilogue
    g.A, g.lda, g.W, g.ldw, g.bias = _ptr(a), a.stride(0), _ptr(w), w.stride(0), _ptr(bias)
    if epilogue != 2 or want_out:
        out = _out_rows(out, (m, n), torch.bfloat16, a.device, "gemm_bf16: out")
        g.out, g.ldo = _ptr(out), n
    elif out is not None:
        raise RuntimeError("gemm_bf16: out given with want_out=False")
    if epilogue == 2:
        if x is None or x.dtype != torch.float32 or not x.is_contiguous() or x.shape != (m, n):
            raise RuntimeError("gemm_bf16: epilogue 2 needs a contiguous fp32 residual x of shape (M, N)")
        g.x, g.alpha = _ptr(x), float(alpha)
        if norm1 is not None:
            g.g1, g.b1, g.eps1 = _ptr(norm1[0]), _ptr(norm1[1]), float(norm1[2])
        if norm2 is not None:
            g.g2, g.b2, g.eps2 = _ptr(norm2[0]), _ptr(norm2[1]), float(norm2[2])
    g.stream = _stream()
    _launch("cm_gemm_bf16", N.lib().cm_gemm_bf16, g, units=m)
    return out


def ffn_supported(d_model: int, hidden: int, dtype) -> bool:
    """cm_ffn_fused's inference forward covers the module: d_model 256, or 144 on the 16x16x32 kernel (csrc/fused_d144.hip); the hidden
    width in whole 256-column slabs, 2048 at the most (the entry point's own limit, csrc/ffn_fused.hip)."""
    return (dtype == torch.bfloat16 and (d_model == 256 or (d_model == 144 and FFN_LAYOUT == 16)) and hidden >= 256 and hidden % 256 == 0
            and hidden <= 2048)


# cm_ffn_fused's inference forward on v_mfma_f32_32x32x16_bf16 (csrc/ffn_fused32.hip, weights in the 32 x 16 tile image) instead of
# 16x16x32 (csrc/ffn_fused.hip): CM_FFN_MFMA32=1
FFN_LAYOUT = 32 if os.environ.get("CM_FFN_MFMA32", "0") == "1" else 16
# CM_FFN_SMALL_ROWS=N: launches of at most N rows run the 32x32x16 kernel with 32-token workgroups (fused.py then keeps both weight
# images).  Off by default: alone it wins below ~12 k rows (8000 rows: 28.5 / 19.4 vs 34.4 / 24.4 us; 16000: 42.8 / 31.2 vs 40.5 / 28.8),
# in the encoder at 16 x 40 s (two parts of 8000 rows whose kernels share the chip) it changes nothing (4.78 vs 4.78 ms)
SMALL_FFN_ROWS = int(os.environ.get("CM_FFN_SMALL_ROWS", "0"))
# cm_ffn_fused (16x16x32 kernel, inference, alpha a power of two) fetches the residual rows once and carries them in the second GEMM's
# accumulators; CM_FFN_RESID_ACC=0 = the rows are loaded a second time behind the last GEMM (cm_ffn_args.flags, per launch)
FFN_RESID_ACC = os.environ.get("CM_FFN_RESID_ACC", "1") == "1"


def _kpad(d: int) -> int:
    """A width padded to whole 32-column k-tiles: 144 -> 160 (the d_model-144 kernels' weight images), 256 -> 256."""
    return (d + 31) // 32 * 32


class PackedWeight:
    """A bf16 (rows, cols) matrix in a fragment-tiled image: ``layout`` 16 = 16-row x 32-column tiles (cm_ffn_pack_weights: every
    kernel that streams packed weights), 32 = 32 x 16 tiles (cm_ffn_pack_weights32: cm_ffn_fused with cm_ffn_args.layout = 1).
    ``pad`` = (rows, cols) >= the matrix's: the image is that of the matrix padded with zeros at the bottom and on the right (the
    d_model-144 kernels read 160-column / 160-row images); ``shape`` stays the matrix's own, ``padded`` is the image's."""

    def __init__(self, w: torch.Tensor, layout: int = 16, pad=None):
        _dev_check(w)
        if w.dtype != torch.bfloat16 or w.dim() != 2:
            raise RuntimeError("PackedWeight: expected a 2-D bf16 tensor")
        if layout not in (16, 32):
            raise RuntimeError("PackedWeight: layout must be 16 or 32")
        w = w.contiguous()
        self.shape = tuple(w.shape)
        self.padded = self.shape if pad is None else (int(pad[0]), int(pad[1]))
        if self.padded[0] < self.shape[0] or self.padded[1] < self.shape[1]:
            raise RuntimeError("PackedWeight: pad must be at least the matrix's shape")
        self.layout = layout
        self.data = torch.empty(self.padded[0] * self.padded[1], dtype=torch.bfloat16, device=w.device)
        self.repack_(w)

    def repack_(self, w: torch.Tensor) -> "PackedWeight":
        """Rewrite the image from a new (rows, cols) bf16 matrix of the same shape, in place (the address a captured graph holds)."""
        if w.dtype != torch.bfloat16 or tuple(w.shape) != self.shape or w.device != self.data.device:
            raise RuntimeError("PackedWeight.repack_: expected a bf16 tensor of the packed shape on the image's device")
        w = w.contiguous()
        if self.padded != self.shape:
            w = torch.nn.functional.pad(w, (0, self.padded[1] - self.shape[1], 0, self.padded[0] - self.shape[0]))
        fn = N.lib().cm_ffn_pack_weights if self.layout == 16 else N.lib().cm_ffn_pack_weights32
        rc = fn(_ptr(w), w.shape[0], w.shape[1], _ptr(self.data), _stream())
        N.check(rc, "cm_ffn_pack_weights")
        return self


def ffn_fused(x, pre_norm, w1, b1, w2, b2, alpha=0.5, addend=None, add_scale=1.0, norm1=None, norm2=None,
              x_out=None, want_h=True, h_dtype=torch.bfloat16, proj_w=None, proj_b=None, proj_out=None, train=None, tokens=None,
              resid_acc=None, h_out=None, train_out=None):
    """Whole feed-forward module on the fp32 residual stream (cm_ffn_fused):
        xin = x + add_scale*addend;  r = xin + alpha*(W2 gelu(W1 LN_pre(xin) + b1) + b2);  r = LN1(r) if norm1;
        x_out <- r (x itself when x_out is None);  returns h = LN2(r) (or r when norm2 is None) in h_dtype if want_h.
    x (rows, D) fp32, D = 256 or 144; w1 (hidden, D) / w2 (D, hidden) bf16 tensors or PackedWeight (pack once, reuse); b1/b2 and
    LayerNorm parameters fp32; addend (rows, D) bf16; norm = (weight, bias, eps).
    With ``proj_w`` (PackedWeight (P, D), P % 256 == 0; ``proj_b`` fp32 (P) or None) the Linear that consumes h runs in the
    same kernel and (rows, P) bf16 = h @ proj_w^T (+ proj_b) is returned in h's place; h itself is not stored.
    D = 144 (inference, layout 16 only): P % 64 == 0, and the images are padded to whole tiles -- PackedWeight(w1, pad=(hidden, 160)),
    PackedWeight(w2, pad=(160, hidden)), PackedWeight(proj_w, pad=(P, 160)); bf16 tensors given in their place are padded here.
    ``train`` = (p1, p2, seed1, seed2): the module's TRAINING forward, x_out = x + alpha * drop_p2(W2 drop_p1(gelu(bf16(W1 LN(x) + b1))) + b2)
    with the backward's inputs stored on the way (D = 256 only) -> (x_out, (pre, xn, stats)): pre (rows, hidden) bf16 = W1 LN(x) + b1, xn (rows, 256)
    bf16 = LN(x), stats (2, rows) fp32 = the rows' mean and 1/std (layernorm_bwd's input); the dropout decisions are cm_dropout.h's function of (seed, element index) (no mask is stored).
    ``resid_acc`` (default: CM_FFN_RESID_ACC): False = the residual rows are loaded again behind the last GEMM instead of riding in the
    accumulators (any alpha that is no power of two takes that path by itself).
    ``h_out`` (contiguous (rows, D) in h_dtype) / ``train_out`` = (pre, xn, stats) (contiguous, shaped and typed as above): optional
    tensors to receive h / the training forward's stored outputs instead of fresh ones."""
    _dev_check(x, b1, b2, addend, proj_b)
    rows, d = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("ffn_fused: x must be a contiguous fp32 (rows, d_model) tensor")
    if d != 256 and (d != 144 or train is not None):
        raise RuntimeError(f"ffn_fused: d_model must be 256 (got {d}; 144 runs the inference forward only)")
    lay = w1.layout if isinstance(w1, PackedWeight) else (w2.layout if isinstance(w2, PackedWeight) else (16 if train is not None or d != 256 else FFN_LAYOUT))
    kp = _kpad(d)                                           # 144: images padded to 160 columns (w1, proj_w) / 160 rows (w2)
    w1 = w1 if isinstance(w1, PackedWeight) else PackedWeight(w1, lay, pad=(w1.shape[0], kp))
    w2 = w2 if isinstance(w2, PackedWeight) else PackedWeight(w2, lay, pad=(kp, w2.shape[1]))
    if w1.shape[1] != d or w2.shape != (d, w1.shape[0]):
        raise RuntimeError("ffn_fused: weight shapes do not match x")
    if w1.padded != (w1.shape[0], kp) or w2.padded != (kp, w2.shape[1]):
        raise RuntimeError("ffn_fused: at d_model 144 the images are padded: PackedWeight(w1, pad=(hidden, 160)), PackedWeight(w2, pad=(160, hidden))")
    if d != 256 and w1.layout != 16:
        raise RuntimeError("ffn_fused: d_model 144 takes layout-16 weights")
    if w1.layout != w2.layout or (proj_w is not None and isinstance(proj_w, PackedWeight) and proj_w.layout != w1.layout):
        raise RuntimeError("ffn_fused: w1, w2 and proj_w must be packed in the same layout")
    if train is not None and w1.layout != 16:
        raise RuntimeError("ffn_fused: the training forward takes layout-16 weights")
    for t in (b1, b2) + tuple(pre_norm[:2]):
        if t.dtype != torch.float32:
            raise RuntimeError("ffn_fused: biases and LayerNorm parameters must be fp32")
    a = N.FfnArgs()
    racc = FFN_RESID_ACC if resid_acc is None else bool(resid_acc)
    if not racc:
        a.flags = N.CM_FFN_RELOAD_RESIDUAL
    a.rows, a.dim, a.hidden = rows, d, w1.shape[0]
    a.x, a.pre_g, a.pre_b, a.pre_eps = _ptr(x), _ptr(pre_norm[0]), _ptr(pre_norm[1]), float(pre_norm[2])
    a.w1, a.b1, a.w2, a.b2, a.alpha = _ptr(w1.data), _ptr(b1), _ptr(w2.data), _ptr(b2), float(alpha)
    a.layout = 1 if w1.layout == 32 else 0
    if w1.layout == 32:
        # 32-token workgroups when 64-token ones would not fill the chip's 512 workgroup slots
        a.tokens = int(tokens) if tokens else (32 if rows <= SMALL_FFN_ROWS else 64)
    if addend is not None:
        if addend.dtype != torch.bfloat16 or not addend.is_contiguous() or addend.shape != x.shape:
            raise RuntimeError("ffn_fused: addend must be a contiguous bf16 tensor shaped like x")
        a.addend, a.add_scale = _ptr(addend), float(add_scale)
    if norm1 is not None:
        a.n1_g, a.n1_b, a.n1_eps = _ptr(norm1[0]), _ptr(norm1[1]), float(norm1[2])
    if norm2 is not None:
        a.n2_g, a.n2_b, a.n2_eps = _ptr(norm2[0]), _ptr(norm2[1]), float(norm2[2])
    xo = x if x_out is None else x_out
    a.x_out = _ptr(xo)
    h = None
    if train is not None:
        if addend is not None or norm1 is not None or norm2 is not None or proj_w is not None:
            raise RuntimeError("ffn_fused: the training forward takes no addend / norm1 / norm2 / projection")
        if h_out is not None:
            raise RuntimeError("ffn_fused: the training forward returns no h")
        pre, xn, stats = train_out if train_out is not None else (None, None, None)
        pre = _out_rows(pre, (rows, w1.shape[0]), torch.bfloat16, x.device, "ffn_fused: train_out[0] (pre)")
        xn = _out_rows(xn, (rows, d), torch.bfloat16, x.device, "ffn_fused: train_out[1] (xn)")
        stats = _out_rows(stats, (2, rows), torch.float32, x.device, "ffn_fused: train_out[2] (stats)")
        a.pre_out, a.xn_out, a.stats_out = _ptr(pre), _ptr(xn), _ptr(stats)
        a.p1, a.p2, a.seed1, a.seed2 = float(train[0]), float(train[1]), int(train[2]), int(train[3])
        a.seed_epoch = _seed_epoch_ptr()
        a.stream = _stream()
        _launch("cm_ffn_fused", N.lib().cm_ffn_fused, a, units=rows)
        return xo, (pre, xn, stats)
    if train_out is not None:
        raise RuntimeError("ffn_fused: train_out belongs to the training forward")
    if h_out is not None and (proj_w is not None or not want_h):
        raise RuntimeError("ffn_fused: h_out given, but h is not stored (projection epilogue or want_h=False)")
    if proj_w is not None:
        if (not isinstance(proj_w, PackedWeight) or proj_w.shape[1] != d or proj_w.shape[0] % (256 if d == 256 else 64) or proj_w.shape[0] > 4096
                or proj_w.padded != (proj_w.shape[0], kp)):
            raise RuntimeError("ffn_fused: proj_w must be a PackedWeight of shape (P, d_model), P a multiple of 256 up to 4096 "
                               "(d_model 144: padded to (P, 160), P a multiple of 64)")
        h = proj_out if proj_out is not None else torch.empty((rows, proj_w.shape[0]), dtype=torch.bfloat16, device=x.device)
        if h.shape != (rows, proj_w.shape[0]) or h.dtype != torch.bfloat16 or not h.is_contiguous():
            raise RuntimeError("ffn_fused: proj_out must be a contiguous bf16 (rows, P) tensor")
        _dev_check(h)
        pb = _f32c(proj_b)
        a.proj_w, a.proj_b, a.proj_out, a.proj_dim = _ptr(proj_w.data), _ptr(pb), _ptr(h), proj_w.shape[0]
    elif want_h:
        h = _out_rows(h_out, (rows, d), h_dtype, x.device, "ffn_fused: h_out")
        a.h_out, a.h_dtype = _ptr(h), _DT[h_dtype]
    a.stream = _stream()
    _launch("cm_ffn_fused", N.lib().cm_ffn_fused, a, units=rows)
    return xo, h


_BANDS = {}


def _mel_bands(fb: torch.Tensor):
    """Per-filter [lo, hi) range of non-zero bins (triangular filters are contiguous), cached per filterbank tensor."""
    key = (fb.data_ptr(), tuple(fb.shape))
    if key not in _BANDS:
        nz = (fb != 0)
        idx = torch.arange(fb.shape[0], device=fb.device)[:, None]
        lo = torch.where(nz, idx, fb.shape[0]).amin(0).to(torch.int32)
        hi = (torch.where(nz, idx, -1).amax(0) + 1).to(torch.int32)
        lo = torch.minimum(lo, hi)
        width = (hi - lo).to(torch.int64)
        off = torch.zeros(fb.shape[1] + 1, dtype=torch.int64, device=fb.device)
        off[1:] = torch.cumsum(width, 0)
        total = int(off[-1])
        packed = None
        if 0 < total <= 4096:                              # gather each filter's band into one packed vector
            m_of = torch.repeat_interleave(torch.arange(fb.shape[1], device=fb.device), width)
            f_of = torch.arange(total, device=fb.device) - off[m_of] + lo.to(torch.int64)[m_of]
            packed = fb[f_of, m_of].contiguous()
        _BANDS[key] = (lo.contiguous(), hi.contiguous(), off.to(torch.int32).contiguous(), packed)
    return _BANDS[key]


def fbank_from_stft(spec, fbank, amin=1e-10, top_db=80.0, mean=None, std=None):
    """torch.stft(..., return_complex=True) output (batch, n_freq, frames) -> (batch, frames, n_mels) fp32 log-mel
    features with the per-utterance top_db clamp and optional global normalisation (cm_fbank_mel_db + cm_fbank_finish)."""
    _dev_check(spec, fbank, mean, std)
    sr = torch.view_as_real(spec) if spec.is_complex() else spec
    if sr.dtype != torch.float32 or sr.stride(3) != 1 or any(st % 2 for st in sr.stride()[:3]):
        sr = sr.float().contiguous()
    b, nf, t, _ = sr.shape                               # strided view accepted as is (no 260 MB transpose copy)
    fb = _f32c(fbank)
    m = fb.shape[1]
    db = torch.empty((b, t, m), dtype=torch.float32, device=sr.device)
    umax = torch.empty((b,), dtype=torch.float32, device=sr.device)
    part = torch.empty((b, (t + 15) // 16), dtype=torch.float32, device=sr.device)      # per-tile maxima (no atomics)
    a = N.FbankArgs()
    a.batch, a.n_freq, a.frames, a.n_mels = b, nf, t, m
    a.spec, a.fbank, a.db, a.umax, a.amin, a.top_db = _ptr(sr), _ptr(fb), _ptr(db), _ptr(umax), float(amin), float(top_db)
    mean, std = _f32c(mean), _f32c(std)
    a.mean, a.std = _ptr(mean), _ptr(std)
    lo, hi, off, packed = _mel_bands(fb)
    a.band_lo, a.band_hi = _ptr(lo), _ptr(hi)
    if packed is not None:
        a.band_off, a.band_w = _ptr(off), _ptr(packed)
    a.spec_bs, a.spec_fs, a.spec_ts = sr.stride(0) // 2, sr.stride(1) // 2, sr.stride(2) // 2
    a.umax_part = _ptr(part)
    a.stream = _stream()
    _launch("cm_fbank_mel_db", N.lib().cm_fbank_mel_db, a, units=b * t)
    _launch("cm_fbank_finish", N.lib().cm_fbank_finish, a, units=b * t)
    return db


_FFT_TABLES = {}


def _fft_tables(window: torch.Tensor, n_fft: int):
    """(window zero-padded and centred to n_fft, twiddles exp(-2 pi i k / n_fft) computed in float64), cached."""
    key = (window.data_ptr(), window.numel(), n_fft, str(window.device))
    if key not in _FFT_TABLES:
        win = torch.zeros(n_fft, dtype=torch.float32, device=window.device)
        left = (n_fft - window.numel()) // 2
        win[left:left + window.numel()] = window.float()
        k = torch.arange(n_fft, dtype=torch.float64)
        ang = -2.0 * torch.pi * k / n_fft
        tw = torch.stack([torch.cos(ang), torch.sin(ang)], dim=1).to(torch.float32).to(window.device).contiguous()
        _FFT_TABLES[key] = (win, tw)
    return _FFT_TABLES[key]


def fbank_wav_supported(n_fft: int, hop: int, n_mels: int) -> bool:
    return n_fft == 512 and hop % 2 == 0 and n_mels <= 128


def fbank_from_wav(wav, window, n_fft, hop, fbank, amin=1e-10, top_db=80.0, mean=None, std=None, lens=None, bufs=None):
    """(batch, samples) fp32 waveform -> (batch, 1 + samples // hop, n_mels) fp32 log-mel features, STFT included
    (cm_fbank_wav + cm_fbank_finish): torch.stft(center=True, pad_mode='constant', window centred in n_fft) semantics.
    ``lens`` (cm_fbank_wav_lens + cm_fbank_finish_lens): int32 (batch,) device tensor of SAMPLE counts, utterance b has lens[b]
    samples and 1 + lens[b] // hop frames -- samples behind them read as zero, the top_db maximum runs over its own frames, frames
    at and past its own are not written.  ``bufs``: optional dict of contiguous fp32 outputs db (batch, frames, n_mels), umax (batch,),
    umax_part (batch, ceil(frames / 16))."""
    _dev_check(wav, window, fbank, mean, std)
    if wav.dtype != torch.float32 or wav.dim() != 2 or wav.stride(1) != 1:
        wav = wav.float().contiguous()
    if wav.stride(0) % 2 or wav.data_ptr() % 8:           # the kernel's 8-byte sample loads: even rows from an aligned start
        wav = wav.clone(memory_format=torch.contiguous_format) if wav.shape[1] % 2 == 0 else torch.nn.functional.pad(wav, (0, 1))[:, :wav.shape[1]]
    b, ns = wav.shape
    fb = _f32c(fbank)
    nf, m = fb.shape
    t = 1 + ns // hop
    win, tw = _fft_tables(window, n_fft)
    lo, hi, off, packed = _mel_bands(fb)
    if packed is None:
        raise RuntimeError("fbank_from_wav: filterbank is not banded (no packed band weights)")
    bufs = bufs or {}
    db = _out_rows(bufs.get("db"), (b, t, m), torch.float32, wav.device, "fbank_from_wav: db")
    umax = _out_rows(bufs.get("umax"), (b,), torch.float32, wav.device, "fbank_from_wav: umax")
    part = _out_rows(bufs.get("umax_part"), (b, (t + 15) // 16), torch.float32, wav.device, "fbank_from_wav: umax_part")
    a = N.FbankArgs()
    a.batch, a.n_freq, a.frames, a.n_mels = b, nf, t, m
    a.fbank, a.db, a.umax, a.amin, a.top_db = _ptr(fb), _ptr(db), _ptr(umax), float(amin), float(top_db)
    mean, std = _f32c(mean), _f32c(std)
    a.mean, a.std = _ptr(mean), _ptr(std)
    a.band_lo, a.band_hi, a.band_off, a.band_w = _ptr(lo), _ptr(hi), _ptr(off), _ptr(packed)
    a.umax_part = _ptr(part)
    a.wav, a.window, a.twiddle, a.wav_bs = _ptr(wav), _ptr(win), _ptr(tw), wav.stride(0)
    a.samples, a.hop, a.n_fft = ns, hop, n_fft
    a.stream = _stream()
    if lens is not None:
        lp, lib = _slot_lens(lens, b, wav.device, "fbank_from_wav"), N.lib()
        _launch("cm_fbank_wav_lens", lambda ref: lib.cm_fbank_wav_lens(ref, lp), a, units=b * t)
        _launch("cm_fbank_finish_lens", lambda ref: lib.cm_fbank_finish_lens(ref, lp), a, units=b * t)
        return db
    _launch("cm_fbank_wav", N.lib().cm_fbank_wav, a, units=b * t)
    _launch("cm_fbank_finish", N.lib().cm_fbank_finish, a, units=b * t)
    return db


FRONT_HIST_SAMPLES, FRONT_HIST_FRAMES = 512, 8      # per-stream history of cm_fbank_wav_stream / cm_cnn_front_stream


def _front_plan_ptrs(plan, batch, device, what):
    """The per-slot plan of the streamed front end: (host, device), two contiguous int32 (batch, 8) tensors with the same content,
    rows {n, consumed, total, f0, nf, r0, nr, T_total}.  The C entry point checks the host copy, the kernels read the device copy."""
    host, devt = plan
    for t, where in ((host, "cpu"), (devt, device.type)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != (batch, 8) or not t.is_contiguous() or t.device.type != where:
            raise RuntimeError(f"{what}: plan must be (host, device) contiguous int32 tensors of shape ({batch}, 8)")
    return host.data_ptr(), devt.data_ptr()


def fbank_wav_stream(chunk, hist, hist_out, consumed, f0, nf, window, n_fft, hop, fbank, amin=1e-10, total=-1, bufs=None, plan=None):
    """The frames [f0, f0 + nf) of every stream of an utterance that arrives in chunks (cm_fbank_wav_stream): chunk (batch, n) fp32,
    the samples ``consumed`` .. ``consumed + n`` of the utterance; hist / hist_out (batch, 512) fp32, the samples in front of the
    chunk and the buffer that receives the next call's (another one: the caller swaps); ``total``: the utterance's length when the
    chunk ends it (zero padding past it), else -1.  -> (db (batch, nf, n_mels) fp32 before the top_db clamp, fmax (batch, nf)
    per-frame maxima), or (None, None) for nf = 0, which only rolls the history.  ``bufs``: caller-supplied ``db`` / ``fmax``.
    ``plan`` (cm_fbank_wav_stream_slots): per-slot counts (_front_plan_ptrs); n and ``nf`` are then the maxima over the slots and
    ``consumed`` / ``f0`` / ``total`` are ignored; rows of db / fmax past a slot's own nf are not written."""
    _dev_check(chunk, hist, hist_out, window, fbank)
    b, n = chunk.shape
    if chunk.dtype != torch.float32 or (n and chunk.stride(1) != 1):
        raise RuntimeError("fbank_wav_stream: chunk must be fp32 (batch, n) with the sample axis contiguous")
    _hist_rows(hist, (b, FRONT_HIST_SAMPLES), torch.float32, "fbank_wav_stream: hist")
    _hist_rows(hist_out, (b, FRONT_HIST_SAMPLES), torch.float32, "fbank_wav_stream: hist_out")
    fb = _f32c(fbank)
    m = fb.shape[1]
    a = N.FbankStreamArgs()
    a.batch, a.n_mels, a.n_fft, a.hop, a.n, a.consumed, a.total, a.f0, a.nf = b, m, int(n_fft), int(hop), n, int(consumed), int(total), int(f0), int(nf)
    a.chunk, a.chunk_bs, a.hist, a.hist_out = (_ptr(chunk) if n else None), chunk.stride(0), _ptr(hist), _ptr(hist_out)
    db = fmax = None
    if nf:
        win, tw = _fft_tables(window, n_fft)
        lo, hi, off, packed = _mel_bands(fb)
        if packed is None:
            raise RuntimeError("fbank_wav_stream: filterbank is not banded (no packed band weights)")
        take = _bufs(bufs, ("db", "fmax"), "fbank_wav_stream")
        db = take("db", (b, nf, m), torch.float32, chunk.device)
        fmax = take("fmax", (b, nf), torch.float32, chunk.device)
        a.window, a.twiddle, a.band_lo, a.band_hi, a.band_off, a.band_w = _ptr(win), _ptr(tw), _ptr(lo), _ptr(hi), _ptr(off), _ptr(packed)
        a.db, a.fmax = _ptr(db), _ptr(fmax)
    a.amin, a.stream = float(amin), _stream()
    if plan is not None:
        ph, pd = _front_plan_ptrs(plan, b, chunk.device, "fbank_wav_stream")
        fn = N.lib().cm_fbank_wav_stream_slots
        _launch("cm_fbank_wav_stream_slots", lambda ref: fn(ref, ph, pd), a, units=b * nf)
        return db, fmax
    _launch("cm_fbank_wav_stream", N.lib().cm_fbank_wav_stream, a, units=b * nf)
    return db, fmax


def fbank_finish_stream(db, fmax, umax, f0, top_db=80.0, mean=None, std=None, feat_hist=None, feat_hist_out=None, n_fft=512, plan=None):
    """The causal top_db clamp and the global normalisation of fbank_wav_stream's frames, in place (cm_fbank_finish_stream): the
    floor of frame f is max(umax[b], fmax[b, :f + 1]) - top_db, and umax (batch) fp32 -- -inf at the start of an utterance --
    becomes the maximum over all frames so far.  feat_hist / feat_hist_out (batch, 8, n_mels) fp32: the feature rows in front of
    ``db`` and the buffer that receives the last 8 rows of [feat_hist | db] (another one).  ``plan``
    (cm_fbank_finish_stream_slots): per-slot f0 / nf, db's frame axis being the widest slot's.  -> db."""
    _dev_check(db, fmax, umax, mean, std, feat_hist, feat_hist_out)
    b, nf, m = db.shape
    if db.dtype != torch.float32 or not db.is_contiguous():
        raise RuntimeError("fbank_finish_stream: db must be contiguous fp32 (batch, frames, n_mels)")
    _hist_rows(fmax, (b, nf), torch.float32, "fbank_finish_stream: fmax")
    _hist_rows(umax, (b,), torch.float32, "fbank_finish_stream: umax")
    _hist_rows(feat_hist, (b, FRONT_HIST_FRAMES, m), torch.float32, "fbank_finish_stream: feat_hist")
    _hist_rows(feat_hist_out, (b, FRONT_HIST_FRAMES, m), torch.float32, "fbank_finish_stream: feat_hist_out")
    mean, std = _f32c(mean), _f32c(std)
    if mean is not None and (mean.numel() != m or std.numel() != m):
        raise RuntimeError(f"fbank_finish_stream: mean / std must have {m} elements")
    a = N.FbankStreamArgs()
    a.batch, a.n_mels, a.n_fft, a.f0, a.nf, a.total = b, m, int(n_fft), int(f0), nf, -1
    a.db, a.fmax, a.umax, a.top_db, a.mean, a.std = _ptr(db), _ptr(fmax), _ptr(umax), float(top_db), _ptr(mean), _ptr(std)
    a.feat_hist, a.feat_hist_out, a.stream = _ptr(feat_hist), _ptr(feat_hist_out), _stream()
    if plan is not None:
        ph, pd = _front_plan_ptrs(plan, b, db.device, "fbank_finish_stream")
        fn = N.lib().cm_fbank_finish_stream_slots
        _launch("cm_fbank_finish_stream_slots", lambda ref: fn(ref, ph, pd), a, units=b * nf)
        return db
    _launch("cm_fbank_finish_stream", N.lib().cm_fbank_finish_stream, a, units=b * nf)
    return db


def cnn_front_stream(feats, feat_hist, f0, r0, nr, w1, b1, ln1_w, ln1_b, eps1, w2_ohwi, b2, ln2_w, ln2_b, eps2, slope=0.01, t_total=-1,
                     out=None, plan=None):
    """The rows [r0, r0 + nr) of cnn_front for utterances whose features arrive in chunks (cm_cnn_front_stream): feats (batch, nf, 80)
    fp32 holds the frames from f0 on, feat_hist (batch, 8, 80) the 8 in front of them (None: there are none).  ``t_total``: the
    utterance's number of frames when this call ends it (the reflection at the end is taken), else -1.  -> (batch, nr, 640) bf16.
    ``plan`` (cm_cnn_front_stream_slots): per-slot f0 / nf / r0 / nr / T_total; ``nr`` and feats' frame axis are then the widest
    slot's, and rows of out past a slot's own nr are not written."""
    _dev_check(feats, feat_hist, w1, b1, ln1_w, ln1_b, w2_ohwi, b2, ln2_w, ln2_b, out)
    if feats.dtype != torch.float32 or not feats.is_contiguous() or feats.dim() != 3:
        raise RuntimeError("cnn_front_stream: feats must be contiguous fp32 (batch, frames, bins)")
    b, nf, f = feats.shape
    if not (tuple(w1.shape) == (64, 1, 3, 3) and tuple(w2_ohwi.shape) == (32, 3, 3, 64) and w2_ohwi.dtype == torch.bfloat16 and w2_ohwi.is_contiguous()):
        raise RuntimeError("cnn_front_stream: needs a (64, 1, 3, 3) first conv and a contiguous bf16 (32, 3, 3, 64) second conv")
    _hist_rows(feat_hist, (b, FRONT_HIST_FRAMES, f), torch.float32, "cnn_front_stream: feat_hist")
    w1f, b1f, g1, bt1 = _f32c(w1), _f32c(b1), _f32c(ln1_w).reshape(-1), _f32c(ln1_b).reshape(-1)
    b2f, g2, bt2 = _f32c(b2), _f32c(ln2_w).reshape(-1), _f32c(ln2_b).reshape(-1)
    if g1.numel() != 40 * 64 or g2.numel() != 20 * 32:
        raise RuntimeError("cnn_front_stream: LayerNorm parameters must have 40*64 and 20*32 elements")
    out = _out_rows(out, (b, nr, 640), torch.bfloat16, feats.device, "cnn_front_stream: out")
    a = N.CnnFrontStreamArgs()
    a.batch, a.F, a.C1, a.C2, a.f0, a.nf, a.r0, a.nr, a.T_total = b, f, 64, 32, int(f0), nf, int(r0), int(nr), int(t_total)
    a.feats, a.feat_hist, a.w1, a.b1, a.ln1_g, a.ln1_b = _ptr(feats), _ptr(feat_hist), _ptr(w1f), _ptr(b1f), _ptr(g1), _ptr(bt1)
    a.w2, a.b2, a.ln2_g, a.ln2_b = _ptr(w2_ohwi), _ptr(b2f), _ptr(g2), _ptr(bt2)
    a.eps1, a.eps2, a.slope, a.out, a.stream = float(eps1), float(eps2), float(slope), _ptr(out), _stream()
    if plan is not None:
        ph, pd = _front_plan_ptrs(plan, b, feats.device, "cnn_front_stream")
        fn = N.lib().cm_cnn_front_stream_slots
        _launch("cm_cnn_front_stream_slots", lambda ref: fn(ref, ph, pd), a, units=b * nr)
        return out
    _launch("cm_cnn_front_stream", N.lib().cm_cnn_front_stream, a, units=b * nr)
    return out


def spec_drop_(feats, start, length, dim, fill):
    """In-place SpecAugment masking (cm_spec_drop): feats (batch, frames, n_mels) fp32; start/length int32
    (batch, n_masks); dim 1 = time, 2 = frequency; fill = 0-dim device tensor."""
    _dev_check(feats, start, length, fill)
    if feats.dtype != torch.float32 or not feats.is_contiguous():
        raise RuntimeError("spec_drop_: feats must be contiguous fp32")
    start, length = start.to(torch.int32).contiguous(), length.to(torch.int32).contiguous()
    fill = fill.reshape(1).float()
    b, t, m = feats.shape
    a = N.SpecDropArgs()
    a.batch, a.frames, a.n_mels, a.n_masks, a.dim = b, t, m, start.shape[1], dim
    a.feats, a.start, a.length, a.fill = _ptr(feats), _ptr(start), _ptr(length), _ptr(fill)
    a.stream = _stream()
    _launch("cm_spec_drop", N.lib().cm_spec_drop, a, units=b * t)
    return feats
