"""The folded scan, the host side: cm_scan_cl_fwd_fold, cm_scan_cl_fwd_fold_lens and cm_scan_cl_fwd_fold_workspace_bytes
are declared in include/conmamba_hip.h and exported with the ABI still 12; every configuration the fold is not built for is refused
before anything is launched (every native call here is made with HOST pointers and is refused by a host check); NULL and misaligned
``lens`` are refused; the workspace size is a pure function of the sizes; the Python switch and wrappers."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


class Host:
    """A zeroed host allocation handed out in 256-byte aligned pieces."""

    def __init__(self, nbytes=1 << 21):
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


def fold_args(native, h, batch=2, seqlen=40, dim=64):
    """A launch the fold accepts -- but for its pointers, which are host memory: every test below breaks exactly one requirement."""
    a = native.ScanClArgs()
    a.batch, a.seqlen, a.dim, a.dstate, a.io_dtype, a.delta_softplus, a.ndir, a.time_chunks = batch, seqlen, dim, 16, native.CM_BF16, 1, 2, 1
    a.z, a.z_bs, a.z_ts = h.take(batch * seqlen * dim * 2), seqlen * dim, dim
    out = h.take(batch * seqlen * dim * 2)
    for i, d in enumerate(a.dir):
        d.u, d.xdbl = h.take(batch * seqlen * dim * 2), h.take(batch * seqlen * 48 * 2)
        d.A, d.dt_weight = h.take(dim * 64), h.take(dim * 64)
        d.out = out if i == 0 else None
        d.u_bs, d.u_ts, d.out_bs, d.out_ts, d.xdbl_bs, d.xdbl_ts, d.dt_rank, d.reverse_time = seqlen * dim, dim, seqlen * dim, dim, seqlen * 48, 48, 16, i
    a.workspace_bytes = native.lib().cm_scan_cl_fwd_fold_workspace_bytes(C.byref(a))
    a.workspace = h.take(a.workspace_bytes)
    return a


def test_symbols_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    assert "#define CM_ABI_VERSION 12" in hdr
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12      # additive: the ABI stays
    declared = {s[0]: s for s in native.SYMBOLS}
    handle = C.CDLL(native.LIB_PATH)
    args = C.POINTER(native.ScanClArgs)
    for name, res, argtypes in (("cm_scan_cl_fwd_fold", C.c_int, [args]), ("cm_scan_cl_fwd_fold_lens", C.c_int, [args, C.c_void_p]),
                                ("cm_scan_cl_fwd_fold_workspace_bytes", C.c_int64, [args])):
        assert name in declared, f"{name} is not declared in conmamba_hip.h"
        assert hasattr(handle, name), f"{name} is not exported"
        assert declared[name][1] is res and declared[name][2] == argtypes, declared[name]


def test_null_and_misaligned_lens_are_refused(native):
    h = Host()
    lens = h.take(64)
    fn, a = native.lib().cm_scan_cl_fwd_fold_lens, fold_args(native, h)
    refused(native, fn(None, lens), native.CM_EINVAL, "args is NULL")
    refused(native, fn(C.byref(a), None), native.CM_EINVAL, "lens is NULL")
    refused(native, fn(C.byref(a), lens + 2), native.CM_EALIGN, "4-byte aligned")
    refused(native, native.lib().cm_scan_cl_fwd_fold(None), native.CM_EINVAL, "args is NULL")
    zero = native.ScanClArgs()
    assert fn(C.byref(zero), lens) == native.CM_EINVAL and native.lib().cm_scan_cl_fwd_fold(C.byref(zero)) == native.CM_EINVAL   # bad sizes


@pytest.mark.parametrize("with_lens", [False, True])
def test_every_refusal(native, with_lens):
    h = Host()
    lens = h.take(64)
    lib = native.lib()
    call = (lambda a: lib.cm_scan_cl_fwd_fold_lens(C.byref(a), lens)) if with_lens else (lambda a: lib.cm_scan_cl_fwd_fold(C.byref(a)))
    a = fold_args(native, h)
    U, I, A = native.CM_EUNSUPPORTED, native.CM_EINVAL, native.CM_EALIGN

    # xdbl mode
    xdbl, a.dir[1].xdbl = a.dir[1].xdbl, None
    refused(native, call(a), U, "xdbl mode")
    a.dir[1].xdbl = xdbl
    # two directions, of opposite time
    a.ndir = 1
    refused(native, call(a), U, "two directions")
    a.ndir = 3
    refused(native, call(a), I, "ndir must be 1 or 2")
    a.ndir = 2
    for r0, r1 in ((0, 0), (1, 1)):
        a.dir[0].reverse_time, a.dir[1].reverse_time = r0, r1
        refused(native, call(a), U, "opposite ways")
    a.dir[0].reverse_time, a.dir[1].reverse_time = 0, 1
    # z and softplus
    z, a.z = a.z, None
    refused(native, call(a), U, "z and softplus")
    a.z, a.delta_softplus = z, 0
    refused(native, call(a), U, "z and softplus")
    a.delta_softplus = 1
    # bf16 I/O
    a.io_dtype = native.CM_F32
    refused(native, call(a), U, "bf16 I/O only")
    a.io_dtype = native.CM_BF16
    # dt_rank <= 16
    a.dir[1].dt_rank = 32
    refused(native, call(a), U, "dt_rank 32")
    a.dir[1].dt_rank = 16
    # lanes_per_channel 0 or 4
    a.lanes_per_channel = 8
    refused(native, call(a), U, "lanes_per_channel 8")
    a.lanes_per_channel = 4
    # unchunked
    a.time_chunks = 2
    refused(native, call(a), U, "time_chunks 2")
    a.time_chunks = 1
    # no ckpt, ypre, h0, h_last or decay, in either direction
    state = h.take(2 * 64 * 64)
    for i in (0, 1):
        for field in ("h0", "h_last", "decay", "ckpt", "ypre"):
            setattr(a.dir[i], field, state)
            refused(native, call(a), U, "no carried state")
            setattr(a.dir[i], field, None)
    # dir[1].out NULL or equal to dir[0].out
    a.dir[1].out = state
    refused(native, call(a), U, "one output tensor")
    a.dir[1].out = None
    out, a.dir[0].out = a.dir[0].out, None
    refused(native, call(a), I, "NULL tensor")
    a.dir[0].out = out
    # the checks of the form without a fold
    a.dstate = 8
    refused(native, call(a), U, "dstate 8")
    a.dstate = 16
    a.dir[0].u += 8
    refused(native, call(a), A, "16-byte aligned")
    a.dir[0].u -= 8
    a.dim = 68
    refused(native, call(a), U, "multiple of 8")
    a.dim = 64
    # the workspace
    ws, a.workspace = a.workspace, None
    refused(native, call(a), I, "workspace")
    a.workspace, a.workspace_bytes = ws, a.workspace_bytes - 1
    refused(native, call(a), I, "workspace")
    a.workspace, a.workspace_bytes = ws + 4, a.workspace_bytes + 1
    refused(native, call(a), I, "workspace")
    a.workspace = ws
    a.seqlen = 0
    refused(native, call(a), I, "bad sizes")


def test_workspace_is_a_pure_function_of_the_sizes(native):
    fn = native.lib().cm_scan_cl_fwd_fold_workspace_bytes
    assert fn(None) == 0
    h = Host()
    for batch, seqlen, dim in ((1, 1, 8), (3, 70, 200), (64, 1000, 512), (64, 16, 512)):
        a = native.ScanClArgs()
        a.batch, a.seqlen, a.dim = batch, seqlen, dim
        want = 2 * batch * dim * 16 * 4 + batch * seqlen * dim * 2    # (2, batch, dim, 16) fp32 states + (batch, seqlen, dim) bf16 remainders
        assert fn(C.byref(a)) == want
        b = fold_args(native, h, batch=min(batch, 2), seqlen=8, dim=8)   # pointers, strides, flags: none of them enters
        b.batch, b.seqlen, b.dim, b.time_chunks, b.ndir, b.io_dtype = batch, seqlen, dim, 7, 1, native.CM_F32
        assert fn(C.byref(b)) == want == fn(C.byref(b))


def test_python_layers():
    """fold defaults to today's call; the switch exists and defaults on; mixer_tail still takes the 2E form (seqpar.py calls it)."""
    from mamba_asr_amd import fused, ops
    p = inspect.signature(ops.scan_cl_fwd).parameters
    assert "fold" in p and p["fold"].default is False
    assert inspect.signature(fused._scan).parameters["fold"].default is False
    assert isinstance(fused.USE_SCAN_FOLD, bool)
    assert fused.USE_SCAN_FOLD == (os.environ.get("CM_SCAN_FOLD", "1") == "1")
    assert list(inspect.signature(fused.mixer_tail).parameters) == ["c", "x", "ycat"]
    assert ops.scan_chunks_policy(4, 4000, 1024, 2, lens=object()) == 1
