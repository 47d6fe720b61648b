"""Per-slot streaming of the causal encoder, the host side: the three `_slots` entry points are declared in
include/conmamba_hip.h, exported, and refuse bad arguments before anything is launched; the Python layers refuse a malformed
``lens``.  Every native call here is made with HOST pointers and is refused by a host check, so nothing is launched."""
import ctypes as C
import inspect
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOTS = ("cm_conv_xproj_uni_slots", "cm_scan_cl_fwd_slots", "cm_glu_dwconv_ln_gelu_causal_slots")


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


class Host:
    """A zeroed host allocation handed out in 256-byte aligned pieces."""

    def __init__(self, nbytes=1 << 20):
        self.buf = C.create_string_buffer(nbytes + 256)
        self.at = (C.addressof(self.buf) + 255) // 256 * 256
        self.end = C.addressof(self.buf) + nbytes + 256

    def take(self, nbytes):
        p = self.at
        self.at = (p + nbytes + 255) // 256 * 256
        assert self.at <= self.end
        return p


def refused(native, rc, code, text):
    msg = native.lib().cm_last_error().decode()
    assert rc == code and text in msg, (rc, msg)


def test_symbols_declared_and_exported(native):
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12
    declared = {s[0]: s for s in native.SYMBOLS}
    handle = C.CDLL(native.LIB_PATH)
    for name, args in zip(SLOTS, (native.ConvXprojUniArgs, native.ScanClArgs, native.GluDwconvCausalArgs)):
        assert name in declared, f"{name} is not declared in conmamba_hip.h"
        assert hasattr(handle, name), f"{name} is not exported"
        _, res, argtypes = declared[name]
        assert res is C.c_int and argtypes == [C.POINTER(args), C.c_void_p]    # the lock-step struct + the per-slot array


def conv_args(native, h, batch=2, seqlen=8, dim=64):
    a = native.ConvXprojUniArgs()
    a.batch, a.seqlen, a.dim, a.width, a.dt_pad = batch, seqlen, dim, 4, 16
    a.x, a.y, a.xdbl = h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * 48 * 2)
    a.weight, a.wx = h.take(dim * 16), h.take(48 * dim * 2)
    a.x_hist, a.x_hist_out = h.take(batch * 3 * dim * 2), h.take(batch * 3 * dim * 2)
    a.x_bs, a.x_ts, a.y_bs, a.y_ts, a.xdbl_bs, a.xdbl_ts = seqlen * dim, dim, seqlen * dim, dim, seqlen * 48, 48
    return a


def test_conv_xproj_uni_slots_refusals(native):
    fn, h = native.lib().cm_conv_xproj_uni_slots, Host()
    lens = h.take(64)
    refused(native, fn(None, lens), native.CM_EINVAL, "args is NULL")
    a = conv_args(native, h)
    refused(native, fn(C.byref(a), None), native.CM_EINVAL, "lens is NULL")
    refused(native, fn(C.byref(a), lens + 2), native.CM_EALIGN, "lens must be 4-byte aligned")
    keep = a.x_hist_out
    a.x_hist_out = a.x_hist + 2 * 64 * 2                                        # one row into x_hist: the buffers overlap
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "must not overlap")
    a.x_hist_out = a.x_hist
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "must not overlap")
    a.x_hist_out, a.x = keep, a.x + 2
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "8-byte aligned")
    a.x, a.x_hist = a.x - 2, a.x_hist + 4
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "8-byte aligned")
    a.x_hist, a.seqlen = a.x_hist - 4, 0
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "bad sizes")


def scan_args(native, h, batch=2, seqlen=8, dim=64):
    a = native.ScanClArgs()
    a.batch, a.seqlen, a.dim, a.dstate, a.io_dtype, a.delta_softplus, a.ndir, a.time_chunks = batch, seqlen, dim, 16, native.CM_BF16, 1, 1, 1
    a.z, a.z_bs, a.z_ts = h.take(batch * seqlen * dim * 2), seqlen * dim, dim
    for d in a.dir:
        d.u, d.out, d.xdbl = h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * 48 * 2)
        d.A, d.dt_weight = h.take(dim * 64), h.take(dim * 64)
        d.h0 = d.h_last = h.take(batch * dim * 64)
        d.u_bs, d.u_ts, d.out_bs, d.out_ts, d.xdbl_bs, d.xdbl_ts, d.dt_rank = seqlen * dim, dim, seqlen * dim, dim, seqlen * 48, 48, 16
    return a


def test_scan_cl_fwd_slots_refusals(native):
    fn, h = native.lib().cm_scan_cl_fwd_slots, Host()
    lens = h.take(64)
    refused(native, fn(None, lens), native.CM_EINVAL, "args is NULL")
    a = scan_args(native, h)
    refused(native, fn(C.byref(a), None), native.CM_EINVAL, "lens is NULL")
    refused(native, fn(C.byref(a), lens + 2), native.CM_EALIGN, "lens must be 4-byte aligned")
    a.time_chunks = 2
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "time_chunks 2")
    a.time_chunks, a.ndir = 1, 2
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "two directions")
    a.ndir, a.time_chunks = 2, 4                                                # both at once: still nothing launched
    assert fn(C.byref(a), lens) == native.CM_EUNSUPPORTED
    a.ndir, a.time_chunks = 1, 0
    a.dir[0].u += 8
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "16-byte aligned")
    a.dir[0].u -= 8
    xdbl, a.dir[0].xdbl = a.dir[0].xdbl, None                                   # the state-split kernel has no per-slot form
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "xdbl mode")
    a.dir[0].xdbl, a.dir[0].reverse_time = xdbl, 1
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "forward time")
    a.dir[0].reverse_time, a.lanes_per_channel = 0, 8
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "lanes_per_channel 8")
    a.lanes_per_channel, a.seqlen = 0, 0
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "bad sizes")


def dw_args(native, h, batch=2, seqlen=8, dim=256):
    a = native.GluDwconvCausalArgs()
    a.batch, a.seqlen, a.dim, a.ksize, a.io_dtype, a.glu_done, a.eps = batch, seqlen, dim, 31, native.CM_BF16, 1, 1e-5
    a.in_, a.out = h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * dim * 2)
    a.weight, a.weight_t, a.bias, a.ln_g, a.ln_b = (h.take(dim * 31 * 4) for _ in range(5))
    a.hist, _, a.hist_out = h.take(batch * 30 * dim * 2), h.take(256), h.take(batch * 30 * dim * 2)      # a gap: moving hist by 4 bytes is no overlap
    return a


def test_glu_dwconv_causal_slots_refusals(native):
    fn, h = native.lib().cm_glu_dwconv_ln_gelu_causal_slots, Host()
    lens = h.take(64)
    refused(native, fn(None, lens), native.CM_EINVAL, "args is NULL")
    a = dw_args(native, h)
    refused(native, fn(C.byref(a), None), native.CM_EINVAL, "lens is NULL")
    refused(native, fn(C.byref(a), lens + 2), native.CM_EALIGN, "lens must be 4-byte aligned")
    keep = a.hist_out
    a.hist_out = a.hist + 29 * 256 * 2                                          # the last row of slot 0's history
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "must not overlap")
    a.hist_out = a.hist
    refused(native, fn(C.byref(a), lens), native.CM_EINVAL, "must not overlap")
    a.hist_out = keep + 2
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "4-byte aligned")
    a.hist_out, a.hist = keep, a.hist + 4
    refused(native, fn(C.byref(a), lens), native.CM_EALIGN, "hist must be 16-byte aligned")
    a.hist, a.ksize = a.hist - 4, 15
    refused(native, fn(C.byref(a), lens), native.CM_EUNSUPPORTED, "kernel size 15")


def test_python_layers_take_lens():
    """lens=None on every function the per-slot contract names, in that position, so existing calls are unchanged."""
    from mamba_asr_amd import fused
    from mamba_asr_amd.asr import ConMambaASR
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    from mamba_asr_amd.modules.TransformerASR import TransformerASR
    for fn in (fused.forward_streaming, ConmambaEncoder.forward_streaming, TransformerASR.encode_streaming,
               ConMambaASR.encode_streaming, ConMambaASR.log_probs_streaming):
        p = inspect.signature(fn).parameters
        assert "lens" in p and p["lens"].default is None and list(p)[-1] == "lens", fn.__qualname__


def test_ops_refuse_a_malformed_lens():
    """The wrappers check lens before they build a launch (CPU tensors are refused first, so the check is called directly)."""
    from mamba_asr_amd import ops
    dev = torch.device("cpu")
    good = torch.zeros(4, dtype=torch.int32)
    assert ops._slot_lens(good, 4, dev, "x") == good.data_ptr()
    checked = ops.slot_lens(good, 4, dev)                                       # checked once for the launches of a whole call
    assert ops._slot_lens(checked, 4, dev, "x") == good.data_ptr()
    with pytest.raises(RuntimeError, match="checked for batch 4"):
        ops._slot_lens(checked, 5, dev, "x")
    for bad in (torch.zeros(4, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(8, dtype=torch.int32)[::2], [0, 1, 2, 3]):
        with pytest.raises(RuntimeError, match="lens must be a contiguous int32"):
            ops._slot_lens(bad, 4, dev, "x")
    x = torch.zeros(2, 4, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.scan_cl_fwd([dict(u=x)], lens=torch.zeros(2, dtype=torch.int32))
