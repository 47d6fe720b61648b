"""What the operator-route entry points (cm_selective_scan_fwd / _bwd, cm_causal_conv1d_fwd / _bwd) refuse, handed to the entry points
themselves with HOST pointers: each case returns its documented code and sets cm_last_error before anything is launched.  Only refused
values are ever passed -- an accepted one would launch on host pointers (tests/test_layer_config_gates_cpu.py works the same way).
Then cm_selective_scan_bwd_workspace_bytes against its formula for every lane split, the split rule restated here.
"""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, EUNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    assert (N.CM_OK, N.CM_EINVAL, N.CM_EUNSUPPORTED) == (OK, EINVAL, EUNSUPPORTED)
    return N


_HOST = C.create_string_buffer(1 << 16)
HOST = (C.addressof(_HOST) + 15) // 16 * 16            # a 16-byte aligned host address: never dereferenced by a refused call


def scan_fwd_args(N, **kw):
    a = N.ScanFwdArgs()
    a.batch, a.dim, a.seqlen, a.dstate = 2, 8, 16, 16
    a.io_dtype = a.bc_dtype = N.CM_F32
    for f in ("u", "delta", "A", "B", "C", "out"):
        setattr(a, f, HOST)
    a.u_bs = a.delta_bs = a.out_bs = 8 * 16
    a.u_ds = a.delta_ds = a.out_ds = 16
    a.B_bs = a.C_bs = 16 * 16
    a.B_ns = a.C_ns = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def scan_bwd_args(N, fwd=None, **kw):
    a = N.ScanBwdArgs()
    f = scan_fwd_args(N, **dict(dict(x=HOST), **(fwd or {})))
    C.memmove(C.addressof(a), C.addressof(f), C.sizeof(f))               # a.fwd is the struct's first member
    for f_ in ("dout", "du", "ddelta", "dA", "dB", "dC"):
        setattr(a, f_, HOST)
    a.dout_bs = a.du_bs = a.ddelta_bs = a.fwd.dim * a.fwd.seqlen
    a.dout_ds = a.du_ds = a.ddelta_ds = a.fwd.seqlen
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def conv_args(N, **kw):
    a = N.ConvArgs()
    a.batch, a.dim, a.seqlen, a.width = 2, 8, 16, 4
    a.io_dtype = N.CM_F32
    for f in ("x", "weight", "y", "dy", "dx", "dweight"):
        setattr(a, f, HOST)
    a.x_bs = a.y_bs = a.dy_bs = a.dx_bs = 8 * 16
    a.x_ds = a.y_ds = a.dy_ds = a.dx_ds = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def refused(N, fn, args, code, message):
    rc = fn(C.byref(args))
    err = N.lib().cm_last_error().decode()
    assert rc == code and message in err, (rc, code, err)


def test_first_member(native):
    assert native.ScanBwdArgs.fwd.offset == 0


@pytest.mark.parametrize("lanes", [3, 32, -1])
def test_lane_split_no_power_of_two_up_to_16(native, lanes):
    lib = native.lib()
    refused(native, lib.cm_selective_scan_fwd, scan_fwd_args(native, lanes_per_channel=lanes), EINVAL,
            f"scan_fwd: lanes_per_channel {lanes} (0, 1, 2, 4, 8 or 16)")
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(lanes_per_channel=lanes)), EINVAL,
            f"scan_bwd: lanes_per_channel {lanes} (0, 4, 8 or 16)")


def test_batch_beyond_the_grid_limit(native):
    lib = native.lib()
    refused(native, lib.cm_selective_scan_fwd, scan_fwd_args(native, batch=65536), EINVAL, "scan_fwd: batch 65536 exceeds the grid limit 65535")
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(batch=65536)), EINVAL, "scan_bwd: batch 65536 exceeds the grid limit 65535")
    refused(native, lib.cm_causal_conv1d_fwd, conv_args(native, batch=65536), EINVAL, "causal_conv1d_fwd: batch 65536 exceeds the grid limit 65535")
    refused(native, lib.cm_causal_conv1d_bwd, conv_args(native, batch=65536), EINVAL, "causal_conv1d_bwd: batch 65536 exceeds the grid limit 65535")


@pytest.mark.parametrize("dstate", [4, 32])
@pytest.mark.parametrize("lanes", [0, 4])
def test_dstate_without_a_kernel(native, dstate, lanes):
    lib = native.lib()
    refused(native, lib.cm_selective_scan_fwd, scan_fwd_args(native, dstate=dstate, lanes_per_channel=lanes), EUNSUPPORTED,
            f"scan_fwd: no kernel for dstate={dstate} with lane split S=")
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(dstate=dstate, lanes_per_channel=lanes)), EUNSUPPORTED,
            f"scan_bwd: no kernel for dstate={dstate} with lane split S=")
    assert "(supported dstate: 8, 16)" in lib.cm_last_error().decode()


def test_dtype_pairs_without_a_kernel(native):
    lib, N = native.lib(), native
    for io, bc in ((N.CM_F16, N.CM_F16), (N.CM_F16, N.CM_F32), (N.CM_F32, N.CM_BF16), (N.CM_F32, N.CM_F16), (N.CM_BF16, N.CM_F16)):
        tail = f"unsupported dtype pair io={io} bc={bc} (built: f32/f32, bf16/bf16, bf16/f32)"
        refused(N, lib.cm_selective_scan_fwd, scan_fwd_args(N, io_dtype=io, bc_dtype=bc), EUNSUPPORTED, "scan_fwd: " + tail)
        refused(N, lib.cm_selective_scan_bwd, scan_bwd_args(N, fwd=dict(io_dtype=io, bc_dtype=bc)), EUNSUPPORTED, "scan_bwd: " + tail)
    refused(N, lib.cm_causal_conv1d_fwd, conv_args(N, io_dtype=3), EUNSUPPORTED, "causal_conv1d: unsupported io dtype 3")
    refused(N, lib.cm_causal_conv1d_bwd, conv_args(N, io_dtype=3), EUNSUPPORTED, "causal_conv1d: unsupported io dtype 3")


def test_backward_takes_no_initial_state_and_wants_dz_with_z(native):
    lib = native.lib()
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(h0=HOST)), EUNSUPPORTED,
            "scan_bwd: an initial state (h0) is a forward-only feature")
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(z=HOST, z_bs=128, z_ds=16)), EINVAL,
            "scan_bwd: dz is NULL although z is given")
    refused(native, lib.cm_selective_scan_fwd, scan_fwd_args(native, z=HOST, z_bs=128, z_ds=16), EINVAL, "scan_fwd: out_z output pointer is NULL")
    refused(native, lib.cm_selective_scan_fwd, scan_fwd_args(native, out=None), EINVAL, "scan_fwd: out output pointer is NULL")
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, fwd=dict(x=None)), EINVAL, "scan_bwd: u/delta/A/B/C/x/dout must be non-NULL")


def test_workspace_pointer_and_size_go_together(native):
    lib = native.lib()
    msg = "scan_bwd: workspace must be 16-byte aligned with workspace_bytes > 0, or NULL with 0"
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, workspace=HOST, workspace_bytes=0), EINVAL, msg)
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, workspace=None, workspace_bytes=4096), EINVAL, msg)
    refused(native, lib.cm_selective_scan_bwd, scan_bwd_args(native, workspace=HOST + 4, workspace_bytes=1 << 20), EINVAL, msg)


@pytest.mark.parametrize("dstate,lanes", [(16, 0), (16, 4), (16, 8), (16, 16), (8, 4), (8, 8)])
def test_workspace_one_byte_short(native, dstate, lanes):
    lib = native.lib()
    a = scan_bwd_args(native, fwd=dict(dstate=dstate, lanes_per_channel=lanes, dim=70, batch=3, seqlen=65))
    need = lib.cm_selective_scan_bwd_workspace_bytes(C.byref(a))
    a.workspace, a.workspace_bytes = HOST, need - 1
    refused(native, lib.cm_selective_scan_bwd, a, EINVAL, f"scan_bwd: workspace of {need - 1} bytes is smaller than the {need} this launch needs")


@pytest.mark.parametrize("width", [1, 5, 0])
def test_conv_width(native, width):
    lib = native.lib()
    refused(native, lib.cm_causal_conv1d_fwd, conv_args(native, width=width), EUNSUPPORTED, f"causal_conv1d: width {width} unsupported (2..4)")
    refused(native, lib.cm_causal_conv1d_bwd, conv_args(native, width=width), EUNSUPPORTED, f"causal_conv1d: width {width} unsupported (2..4)")


def test_conv_null_outputs(native):
    lib = native.lib()
    refused(native, lib.cm_causal_conv1d_fwd, conv_args(native, y=None), EINVAL, "causal_conv1d_fwd: y is NULL")
    refused(native, lib.cm_causal_conv1d_bwd, conv_args(native, dweight=None), EINVAL, "causal_conv1d_bwd: dy/dx/dweight must be non-NULL")


def fwd_split(batch, dim, dstate, want):
    """csrc/selective_scan_fwd.hip, cm_scan_pick_split: a requested power of two is clamped to min(dstate, 16); otherwise the smallest
    split whose grid has 1024 waves of 64 / S channels, up to min(dstate, 16)."""
    smax = min(dstate, 16)
    if want >= 1 and want & (want - 1) == 0:
        return min(want, smax)
    s = 1
    while s < smax and batch * -(-dim // (64 // s)) < 1024:
        s *= 2
    return s


def bwd_split(batch, dim, dstate, want):
    """csrc/selective_scan_bwd.hip, bwd_split: the forward's pick, at least 4, at least 8 when the caller did not ask, at most dstate."""
    s = max(fwd_split(batch, dim, dstate, want), 4)
    if s < 8 and want == 0:
        s = 8
    return min(s, dstate)


@pytest.mark.parametrize("dstate", [16, 8])
@pytest.mark.parametrize("lanes", [0, 1, 2, 4, 8, 16])
def test_workspace_bytes_follow_the_lane_split(native, dstate, lanes):
    """2 gx batch dstate L + batch dim dstate + 2 batch dim floats, gx = ceil(dim / (4 x 64 / S)) for the split the launch will use."""
    lib = native.lib()
    for batch, dim, seqlen in ((3, 1, 1), (2, 64, 65), (2, 65, 64), (3, 17, 129), (32, 512, 1000), (64, 1024, 7)):
        a = scan_bwd_args(native, fwd=dict(batch=batch, dim=dim, seqlen=seqlen, dstate=dstate, lanes_per_channel=lanes))
        s = bwd_split(batch, dim, dstate, lanes)
        assert s in ((4, 8, 16) if dstate == 16 else (4, 8))
        gx = -(-dim // (4 * 64 // s))
        want = 4 * (2 * gx * batch * dstate * seqlen + batch * dim * dstate + 2 * batch * dim)
        assert lib.cm_selective_scan_bwd_workspace_bytes(C.byref(a)) == want, (batch, dim, seqlen, s)
    assert lib.cm_selective_scan_bwd_workspace_bytes(None) == 0
    assert lib.cm_selective_scan_bwd_workspace_bytes(C.byref(scan_bwd_args(native, fwd=dict(seqlen=0)))) == 0
