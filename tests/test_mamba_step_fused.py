"""cm_mamba_step (one launch for a mixer's decoding step between in_proj and out_proj), UniMamba.prefill, and their ABI.

  * the kernel against an fp64 restatement of its four formulas (include/conmamba_hip.h), four consecutive steps from
    random states, y and both states compared after every step; run-to-run bits; unsupported shapes            [GPU]
  * UniMamba.prefill(h) == the states T calls of UniMamba.step leave                                             [GPU]
  * the symbol, the ABI version, argument validation without a GPU, build()                                      [CPU]

Bounds.  fp32: the project's bound for fp32 module outputs against a reference (tests/test_hip_parity_r3.py `close`): rtol 2e-3,
atol 2e-4 x max(1, max|ref|).  bf16 I/O: the kernel computes in fp32 from the bf16 inputs, so its y is the bf16 rounding of an
fp32 value whose error is the fp32 bound's: against the fp64 result rounded to bf16 it can sit one bf16 ulp (2^-8 relative) off
-> rtol 2e-2, with the fp32 bound's atol for results near zero; its states are fp32 and keep the fp32 bound against the
restatement fed the same bf16-rounded inputs.
"""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def close(a, b, rtol=2e-3, atol=2e-4):
    scale = max(1.0, float(b.abs().max()))
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol * scale)


# ----------------------------------------------------------------------------------------------------------
# the kernel vs fp64
# ----------------------------------------------------------------------------------------------------------
def ref_step(xz, conv_state, ssm_state, w):
    """The four formulas of cm_mamba_step in fp64; returns (y, conv_state, ssm_state) as new tensors."""
    E, R = conv_state.shape[1], w["dt_proj"].shape[1]
    x_in, z = xz[:, :E], xz[:, E:]
    conv_state = torch.cat([conv_state[:, :, 1:], x_in[:, :, None]], dim=-1)                 # shift left, append
    x = (conv_state * w["conv_w"][None]).sum(-1) + w["conv_b"]
    x = x * torch.sigmoid(x)
    x_dbl = x @ w["x_proj"].t()                                                              # (batch, R + 32)
    dt = F.softplus(x_dbl[:, :R] @ w["dt_proj"].t() + w["dt_bias"])
    Bm, Cm = x_dbl[:, R:R + 16], x_dbl[:, R + 16:]
    ssm_state = ssm_state * torch.exp(dt[:, :, None] * w["A"][None]) + dt[:, :, None] * Bm[:, None, :] * x[:, :, None]
    y = ((ssm_state * Cm[:, None, :]).sum(-1) + w["D"] * x) * (z * torch.sigmoid(z))
    return y, conv_state, ssm_state


def _case(batch, E, R, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * E + 10 * R + batch + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = {"conv_w": rn(E, 4) * 0.5, "conv_b": rn(E) * 0.1, "x_proj": rn(R + 32, E) * E ** -0.5, "dt_proj": rn(E, R) * R ** -0.5,
         "dt_bias": rn(E) - 2.0, "A": -torch.exp(rn(E, 16) * 0.5), "D": rn(E)}
    xz = [rn(batch, 2 * E).to(dtype) for _ in range(4)]
    return w, xz, rn(batch, E, 4), rn(batch, E, 16)


def _run(w, xz, conv0, ssm0):
    from mamba_asr_amd import ops
    wd = {k: v.to(DEV) for k, v in w.items()}
    conv, ssm = conv0.to(DEV).clone(), ssm0.to(DEV).clone()
    trace = []
    for step in xz:
        y = ops.mamba_step(step.to(DEV), conv, ssm, wd["conv_w"], wd["conv_b"], wd["x_proj"], wd["dt_proj"], wd["dt_bias"], wd["A"], wd["D"])
        trace.append((y.clone(), conv.clone(), ssm.clone()))
    return trace


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("E,R", [(8, 1), (256, 8), (288, 9), (1024, 32), (4096, 32)])
def test_mamba_step_vs_fp64(E, R, batch, dtype):
    """Four consecutive steps from random non-zero states: the conv-state shift and the in-place carry of both states are
    exercised; 288 is no multiple of the 256 channels a wave's x_proj pass covers, and leaves the last pass of the
    512-thread channel loops partly empty; dt_rank 9 is no multiple of 4.  (8, 1): the smallest supported row, two lanes of one
    wave in the x_proj pass; (4096, 32): the largest, x fills its LDS array."""
    w, xz, conv0, ssm0 = _case(batch, E, R, dtype)
    got = _run(w, xz, conv0, ssm0)
    wr = {k: v.double() for k, v in w.items()}
    conv, ssm = conv0.double(), ssm0.double()
    for i, step in enumerate(xz):
        y, conv, ssm = ref_step(step.double(), conv, ssm, wr)                # the inputs as the kernel sees them (bf16-rounded)
        gy, gconv, gssm = got[i]
        assert gy.dtype == dtype and gconv.dtype == torch.float32 and gssm.dtype == torch.float32
        err = (gy.double().cpu() - y).abs().max().item()
        print(f"E {E} R {R} batch {batch} {dtype} step {i}: max|y err| {err:.3e}  max|ssm err| {(gssm.double().cpu() - ssm).abs().max().item():.3e}")
        if dtype == torch.float32:
            close(gy, y)
        else:
            close(gy, y.to(torch.bfloat16), rtol=2e-2)
        close(gconv, conv)
        close(gssm, ssm)
    again = _run(w, xz, conv0, ssm0)
    for a, b in zip(got, again):
        assert all(torch.equal(p, q) for p, q in zip(a, b)), "cm_mamba_step is not bit-identical from run to run"


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["d_state 8", "d_conv 3", "dt_rank 33"])
def test_mamba_step_rejects_unsupported_shapes(what):
    from mamba_asr_amd import ops
    E = 64
    N, K, R = (8 if what == "d_state 8" else 16), (3 if what == "d_conv 3" else 4), (33 if what == "dt_rank 33" else 8)
    z = lambda *s: torch.zeros(*s, device=DEV)
    conv, ssm = torch.ones(2, E, K, device=DEV), torch.ones(2, E, N, device=DEV)
    with pytest.raises(RuntimeError, match=r"cm_mamba_step failed \(code -2\)"):
        ops.mamba_step(z(2, 2 * E), conv, ssm, z(E, K), z(E), z(R + 2 * N, E), z(E, R), z(E), z(E, N), z(E))
    torch.cuda.synchronize()
    assert bool((conv == 1).all()) and bool((ssm == 1).all())               # nothing was launched
    assert not ops.mamba_step_supported(E, N, K, R, torch.float32)


# ----------------------------------------------------------------------------------------------------------
# prefill == stepping
# ----------------------------------------------------------------------------------------------------------
_MIXERS = {}


def _mixer(d_model):
    from mamba_asr_amd.modules.mamba.bimamba import UniMamba
    if d_model not in _MIXERS:
        torch.manual_seed(7 + d_model)
        _MIXERS[d_model] = UniMamba(d_model=d_model, d_state=16, d_conv=4, expand=2).to(DEV).eval()
    return _MIXERS[d_model]


def _stepped_states(m, h):
    conv, ssm = m.allocate_inference_cache(h.shape[0])
    for t in range(h.shape[1]):
        m.step(h[:, t:t + 1], conv, ssm)
    return conv, ssm


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 16, 37])
def test_prefill_equals_stepping_fp32(T):
    """E 256 / dt_rank 8, batch 2.  T = 3: the conv state is zero-filled on the left; T = 37: no multiple of the scan's
    16-step block."""
    m = _mixer(128)
    assert m.d_inner == 256 and m.dt_rank == 8
    h = torch.randn(2, T, 128, generator=torch.Generator().manual_seed(T)).to(DEV)
    with torch.no_grad():
        conv_p, ssm_p = m.prefill(h)
        conv_s, ssm_s = _stepped_states(m, h)
    assert conv_p.shape == (2, 256, 4) and ssm_p.shape == (2, 256, 16) and conv_p.dtype == ssm_p.dtype == torch.float32
    if T < 4:
        assert bool((conv_p[:, :, :4 - T] == 0).all())
    assert float(ssm_s.abs().max()) > 0
    close(conv_p, conv_s)
    close(ssm_p, ssm_s)


@pytest.mark.gpu
def test_prefill_equals_stepping_fp32_operator_route():
    """E 1024 / dt_rank 32 in fp32: the rows kernels are not built for dt_rank > 16 in fp32, so prefill takes the last checkpoint of
    cm_selective_scan_fwd; T = 70 crosses that kernel's 64-step chunk.  The fp32 bound."""
    from mamba_asr_amd.modules.mamba import mixer_rows
    m = _mixer(512)
    h = torch.randn(2, 70, 512, generator=torch.Generator().manual_seed(70)).to(DEV)
    assert not mixer_rows.supported(m, h)
    with torch.no_grad():
        conv_p, ssm_p = m.prefill(h)
        conv_s, ssm_s = _stepped_states(m, h)
    close(conv_p, conv_s)
    close(ssm_p, ssm_s)


@pytest.mark.gpu
def test_prefill_equals_stepping_bf16_large():
    """E 1024 / dt_rank 32 under bf16 autocast, T = 37.  The bound is bf16's: the two routes round different intermediates to
    bf16 (the sequence pass keeps the conv output and x_dbl in bf16 and hands bf16 weights to its GEMMs; the step kernel
    keeps them fp32), so every term dt B x of a state carries up to ~5 roundings of 2^-9 relative each, ~1e-2 -> rtol 2e-2,
    and the same fraction of the largest state for sums that cancel.  The conv states are in_proj outputs rounded to bf16
    by GEMMs of different shapes: at most one bf16 ulp (2^-8) apart."""
    m = _mixer(512)
    assert m.d_inner == 1024 and m.dt_rank == 32
    h = torch.randn(2, 37, 512, generator=torch.Generator().manual_seed(37)).to(DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        conv_p, ssm_p = m.prefill(h)
        conv_s, ssm_s = _stepped_states(m, h)
    print(f"bf16 prefill vs stepping: max|conv diff| {(conv_p - conv_s).abs().max().item():.3e} max|ssm diff| "
          f"{(ssm_p - ssm_s).abs().max().item():.3e} (max|ssm| {ssm_s.abs().max().item():.3e})")
    close(conv_p, conv_s, rtol=2e-2, atol=2e-2)
    close(ssm_p, ssm_s, rtol=2e-2, atol=2e-2)


# ----------------------------------------------------------------------------------------------------------
# ABI, without a GPU
# ----------------------------------------------------------------------------------------------------------
def test_mamba_step_symbol_and_abi_version():
    import mamba_asr_amd._native as N
    lib = N.lib()
    assert "cm_mamba_step" in {s[0] for s in N.SYMBOLS} and hasattr(lib, "cm_mamba_step")
    assert N.ABI_VERSION == 12 and lib.cm_abi_version() == N.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    assert "#define CM_ABI_VERSION 12" in hdr


def test_mamba_step_validates_without_launching():
    """NULL / bad sizes -> CM_EINVAL (-1); a shape the kernel is not built for -> CM_EUNSUPPORTED (-2) before anything is
    launched (the pointers here are host memory and there may be no GPU at all)."""
    import mamba_asr_amd._native as N
    lib = N.lib()
    assert lib.cm_mamba_step(None) == -1
    a = N.MambaStepArgs()
    assert lib.cm_mamba_step(C.byref(a)) == -1 and b"bad sizes" in lib.cm_last_error()
    a.batch, a.dim, a.dstate, a.dconv, a.dt_rank, a.io_dtype = 2, 64, 16, 4, 8, N.CM_F32
    assert lib.cm_mamba_step(C.byref(a)) == -1 and b"NULL" in lib.cm_last_error()
    host = (C.c_char * 256)()
    base = (C.addressof(host) + 63) // 64 * 64
    for f in ("xz", "conv_state", "ssm_state", "conv_weight", "x_proj_weight", "dt_proj_weight", "A", "out"):
        setattr(a, f, base)
    for field, bad in (("dstate", 8), ("dconv", 3), ("dt_rank", 33), ("dim", 60), ("dim", 4104), ("io_dtype", N.CM_F16)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.cm_mamba_step(C.byref(a)) == -2, (field, bad)
        setattr(a, field, good)


def test_build_entry_succeeds():
    subprocess.check_call([sys.executable, "-c", "import __graft_entry__ as g; g.build()"], cwd=ROOT)
