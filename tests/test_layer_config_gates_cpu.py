"""The layer-configuration gates, the parts that need no GPU (tests/layer_config_ref.py holds the reference and the table).

  * sensitivity: for every option the table turns on, the fp64 reference with that option REMOVED differs from the full reference by
    more than the bf16 allowance of the GPU file on at least 25 % of the output elements -- a fallback that drops a bias, keeps the
    0.5, ignores gamma, invents a conv bias, reads 16 dt columns of 24 or half the state columns cannot pass the GPU comparison;
  * the generalised reference equals oracle.conmamba_oracle.encoder to 1e-12 on every case the oracle can express;
  * gate mirrors: the first value every numeric limit refuses, handed to the entry point itself with host pointers, returns
    CM_EUNSUPPORTED / CM_EINVAL and sets cm_last_error before anything is launched, and the Python predicate that routes layers to
    that entry point says the same.  Only refused values are ever passed: an accepted one would launch on host pointers.
"""
import ctypes as C
import dataclasses
import types

import pytest
import torch

import layer_config_ref as R
from oracle import conmamba_oracle as O

BF16_TOL = R.INFER_TOL[torch.bfloat16]
CAP = 0.25


def _changed(alt, ref):
    return ((alt - ref).abs() > BF16_TOL["atol"] + BF16_TOL["rtol"] * ref.abs()).double().mean().item()


@pytest.fixture(scope="module")
def built():
    cache = {}

    def get(name):
        if name not in cache:
            case = R.CASES[name]
            enc, x = R.build(case)
            p = R.params64(enc)
            cache[name] = (case, enc, p, x, R.reference(case, p, x))
        return cache[name]
    return get


def _drop_bias(p, case):
    return {k: v for k, v in p.items() if not k.endswith(("in_proj.bias", "out_proj.bias"))}, case.if_devide_out


def _keep_half(p, case):
    return p, True


def _unit_gamma(p, case):
    return {k: (torch.ones_like(v) if k.endswith(".gamma") else v) for k, v in p.items()}, case.if_devide_out


def _zero_conv_bias(p, case):
    return {k: (torch.zeros_like(v) if ".mamba.conv1d" in k and k.endswith("bias") else v) for k, v in p.items()}, case.if_devide_out


def _a_conv_bias(p, case):
    """conv_bias=False removed = a layer that has one: N(0, 0.5), the draw every other case's conv bias comes from."""
    g = torch.Generator().manual_seed(77)
    q = dict(p)
    for k, v in p.items():
        if ".mamba.conv1d" in k and k.endswith("weight"):
            q[k[:-len("weight")] + "bias"] = torch.randn(v.shape[0], generator=g, dtype=torch.float64) * 0.5
    return q, case.if_devide_out


def _dt_first_16(p, case):
    q = {k: v.clone() for k, v in p.items()}
    for k in q:
        if ".mamba.x_proj" in k:
            q[k][16:case.dt_rank] = 0
    return q, case.if_devide_out


def _half_the_state(p, case):
    n = case.mamba_config()["d_state"]
    q = {k: v.clone() for k, v in p.items()}
    for k in q:
        if ".mamba.x_proj" in k:
            q[k][case.dt_rank + n // 2:case.dt_rank + n] = 0          # B's upper half: a scan that reads 16 columns where there are 8, or the reverse
    return q, case.if_devide_out


SENSITIVITY = [("opt_bias", _drop_bias), ("opt_no_devide", _keep_half), ("opt_layer_scale", _unit_gamma), ("opt_no_conv_bias", _a_conv_bias),
               ("opt_all", _drop_bias), ("opt_all", _keep_half), ("opt_all", _unit_gamma), ("opt_all", _a_conv_bias),
               ("expand2", _zero_conv_bias),
               ("dt_rank17", _dt_first_16), ("dt_rank24", _dt_first_16), ("dt_rank32", _dt_first_16), ("dt_rank33", _dt_first_16),
               ("dt_rank40", _dt_first_16), ("causal_dt_rank24", _dt_first_16), ("causal_dt_rank40", _dt_first_16),
               ("d_state8", _half_the_state), ("expand2", _half_the_state)]


@pytest.mark.parametrize("name,removed", SENSITIVITY, ids=[f"{n}-{f.__name__.strip('_')}" for n, f in SENSITIVITY])
def test_removing_the_option_moves_a_quarter_of_the_output(name, removed, built):
    case, _, p, x, ref = built(name)
    q, devide = removed(p, case)
    alt = R.encoder(q, x.double(), case.layers, "", case.kernel_size, case.causal, devide)
    frac = _changed(alt, ref)
    print(f"{name} {removed.__name__}: {frac:.3f} of the elements move by more than the bf16 allowance")
    assert frac >= CAP


ORACLE_CASES = [n for n, c in R.CASES.items() if not c.causal and not n.startswith("opt_")]


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_generalised_reference_equals_the_oracle(name, built):
    """Every case the oracle can express: two directions, conv bias, no projection bias, 0.5, no gamma, 'same' padding.  The oracle's
    mixer runs its inner op in fp32 (oracle.bimamba_v2 hands no work_dtype on); work_dtype=None is that arithmetic."""
    case, enc, _, x, _ = built(name)
    p32 = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    want = O.encoder(p32, x.double(), case.layers, kernel_size=case.kernel_size)
    got = R.reference(case, p32, x, work_dtype=None)
    assert (got - want).abs().max().item() <= 1e-12
    # and the fp64 mixer is the same function, 1e-5 away from the fp32 one at most
    assert (R.reference(case, p32, x) - want).abs().max().item() < 1e-4


def test_oracle_cannot_express_the_rest(built):
    """What the generalisation is for: the oracle raises on the unidirectional layer and on a missing conv bias."""
    for name in ("causal_expand1", "opt_no_conv_bias"):
        case, enc, _, x, _ = built(name)
        with pytest.raises(KeyError):
            O.encoder({k: v.detach() for k, v in enc.state_dict().items()}, x.double(), case.layers)


def test_reference_is_differentiable(built):
    case, enc, _, x, _ = built("opt_all")
    p = R.params64(enc, requires_grad=True)
    xg = x.double().requires_grad_(True)
    R.reference(case, p, xg).sum().backward()
    missing = [k for k, v in p.items() if v.grad is None]
    assert not missing and xg.grad is not None, missing


def test_table_agrees_with_fused_supports(built):
    from mamba_asr_amd import fused
    for name, case in R.CASES.items():
        _, enc, _, _, _ = built(name)
        assert all(fused.supports(l) for l in enc.layers) == case.supports, name


# ------------------------------------------------------------------------------------------------------------------------
# gate mirrors
# ------------------------------------------------------------------------------------------------------------------------
_HOST = (C.c_char * 4096)()
_BASE = (C.addressof(_HOST) + 255) // 256 * 256


def _filled(obj, skip=("stream",)):
    """Every pointer field of a ctypes argument struct (nested direction arrays included) -> one aligned host address."""
    for fname, ftype in obj._fields_:
        if ftype is C.c_void_p:
            if fname not in skip:
                setattr(obj, fname, _BASE)
        elif hasattr(ftype, "_length_"):
            for el in getattr(obj, fname):
                _filled(el, skip)
    return obj


def _refused(fn, args, code, word):
    import mamba_asr_amd._native as N
    lib = N.lib()
    rc = getattr(lib, fn)(C.byref(args))
    assert rc == code, (fn, rc, lib.cm_last_error())
    assert word.encode() in lib.cm_last_error(), lib.cm_last_error()


def _cuda_like(shape, dtype=torch.float32):
    """What the *_rows.supported predicates read of their input, with is_cuda set: the predicates can be asked without a GPU."""
    return types.SimpleNamespace(is_cuda=True, dim=lambda: len(shape), dtype=dtype, shape=tuple(shape))


def test_add_layernorm_width_limit_and_its_mirrors(built):
    """cm_add_layernorm: 1032 columns -> CM_EUNSUPPORTED.  fused.supports (every inference route off cm_ffn_fused goes through this
    kernel), ffn_rows, convmod_rows and mixer_rows.block_supported say the same at 1032 and admit 1024."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import fused
    from mamba_asr_amd.modules import convmod_rows, ffn_rows
    from mamba_asr_amd.modules.mamba import mixer_rows
    a = _filled(N.AddLnArgs())
    a.rows, a.dim, a.y_dtype, a.out_dtype, a.alpha = 38, 1032, N.CM_F32, N.CM_F32, 1.0
    _refused("cm_add_layernorm", a, N.CM_EUNSUPPORTED, "add_layernorm")
    for name, ok in (("d1024", True), ("d1032", False)):
        case, enc, _, _, _ = built(name)
        layer = enc.layers[0]
        x = _cuda_like((2, 19, case.d_model))
        pff = layer.ffn_module1[1]
        assert fused.supports(layer) == ok
        assert ffn_rows.supported(x, layer.ffn_module1[0], pff.ffn[0], pff.ffn[1], pff.ffn[3]) == ok
        assert convmod_rows.supported(layer.convolution_module, x) == ok
        # the table's wide layers have dt_rank = d_model / 16 = 64, outside the row-group scan; its width limit shows at dt_rank 16
        m16 = R.build(dataclasses.replace(case, mamba={"expand": 1, "dt_rank": 16}))[0].layers[0]
        assert not mixer_rows.supported(layer.mamba, x) and mixer_rows.supported(m16.mamba, x)
        assert mixer_rows.block_supported(m16.mamba, m16.norm1.norm, x) == ok


def test_ffn_fused_limits_and_ffn_supported():
    """cm_ffn_fused: hidden 2304 (the first multiple of 256 past 2048), 264 and d_model 264 -> CM_EUNSUPPORTED; a 4352-wide projection
    -> CM_EINVAL.  ops.ffn_supported admits exactly what the entry point takes."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    from mamba_asr_amd.modules import ffn_rows

    def args(dim=256, hidden=256, proj=0):
        a = _filled(N.FfnArgs(), skip=("stream", "addend", "n1_g", "n1_b", "n2_g", "n2_b", "h_out", "pre_out", "xn_out", "stats_out", "seed_epoch")
                    + (() if proj else ("proj_w", "proj_b", "proj_out")))
        a.rows, a.dim, a.hidden, a.alpha, a.proj_dim = 65, dim, hidden, 0.5, proj
        return a
    _refused("cm_ffn_fused", args(hidden=2304), N.CM_EUNSUPPORTED, "hidden")
    _refused("cm_ffn_fused", args(hidden=264), N.CM_EUNSUPPORTED, "hidden")
    _refused("cm_ffn_fused", args(dim=264), N.CM_EUNSUPPORTED, "d_model")
    _refused("cm_ffn_fused", args(proj=4352), N.CM_EINVAL, "projection")
    _refused("cm_ffn_fused", args(proj=384), N.CM_EINVAL, "projection")
    bf = torch.bfloat16
    assert ops.ffn_supported(256, 2048, bf) and ops.ffn_supported(256, 256, bf) and ops.ffn_supported(144, 256, bf)
    assert not ops.ffn_supported(256, 2304, bf) and not ops.ffn_supported(256, 264, bf) and not ops.ffn_supported(264, 256, bf)
    assert not ops.ffn_supported(256, 256, torch.float32)
    # the training pair: cm_ffn_bwd_fused has the same hidden limit and d_model 256 only
    b = _filled(N.FfnBwdArgs())
    b.rows, b.dim, b.hidden, b.alpha = 65, 256, 2304, 0.5
    _refused("cm_ffn_bwd_fused", b, N.CM_EUNSUPPORTED, "hidden")
    b.dim, b.hidden = 264, 256
    _refused("cm_ffn_bwd_fused", b, N.CM_EUNSUPPORTED, "d_model")
    assert ffn_rows._fused_ok(bf, 256, 2048, 111) and not ffn_rows._fused_ok(bf, 256, 2304, 111) and not ffn_rows._fused_ok(bf, 264, 256, 111)
    assert not ffn_rows._fused_ok(torch.float32, 256, 256, 111)


def test_mixer_tail_projection_limits():
    """cm_ln_pw_glu_mix: proj_k 8320 (past 8192), 192 and 64 (no multiple of 128 / below it), d_model 144 -> CM_EUNSUPPORTED."""
    import mamba_asr_amd._native as N
    for dim, k, word in ((256, 8320, "proj_k"), (256, 192, "proj_k"), (256, 64, "proj_k"), (144, 512, "d_model")):
        a = _filled(N.LnPwGluMixArgs())
        a.rows, a.dim, a.proj_k, a.alpha, a.eps = 65, dim, k, 1.0, 1e-5
        _refused("cm_ln_pw_glu_mix", a, N.CM_EUNSUPPORTED, word)


def test_conv_xproj_limits():
    """cm_conv_xproj / cm_conv_xproj_uni: E 2080 (past 2048), 304 and 300 (no multiple of 32), conv width 3, 48-wide dt padding."""
    import mamba_asr_amd._native as N
    for cls, fn in ((N.ConvXprojArgs, "cm_conv_xproj"), (N.ConvXprojUniArgs, "cm_conv_xproj_uni")):
        for dim, width, pad, word in ((2080, 4, 16, "dim"), (304, 4, 16, "dim"), (300, 4, 16, "dim"), (256, 3, 16, "width"), (256, 4, 48, "dt_pad")):
            a = _filled(cls(), skip=("stream", "x_hist", "x_hist_out"))
            a.batch, a.seqlen, a.dim, a.width, a.dt_pad = 2, 19, dim, width, pad
            _refused(fn, a, N.CM_EUNSUPPORTED, word)
    # both directions with 64-wide rows (16 < dt_rank <= 32): the LDS tile pair stops at 1248 channels; one direction goes on to 2048
    a = _filled(N.ConvXprojArgs())
    a.batch, a.seqlen, a.dim, a.width, a.dt_pad = 2, 19, 1280, 4, 32
    _refused("cm_conv_xproj", a, N.CM_EUNSUPPORTED, "too wide")
    from mamba_asr_amd import ops
    sup = ops.conv_xproj_supported
    assert sup(2048, 16) and sup(1248, 32) and not sup(1280, 32) and not sup(2048, 32) and sup(2048, 32, ndir=1) and sup(32, 32)
    assert not sup(2080, 16) and not sup(304, 16) and not sup(300, 16) and not sup(256, 16, d_conv=3) and not sup(2080, 32, ndir=1)


def test_scan_and_conv_gates_and_mixer_rows_supported(built):
    """The row-group scan (forward and backward) refuses d_state 8, 48-wide dt padding, 64-wide rows in fp32 and E = 300; the conv
    backward refuses width 3; mixer_rows.supported refuses the same layers (and every option its node does not carry)."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd.modules.mamba import mixer_rows

    def scan(cls, dim=512, dstate=16, dtype=N.CM_BF16, pad=16):
        a = _filled(cls(), skip=("stream",))
        a.batch, a.seqlen, a.dim, a.dstate, a.io_dtype, a.ndir, a.workspace_bytes = 2, 19, dim, dstate, dtype, 2, 1 << 30
        if hasattr(a, "delta_softplus"):
            a.delta_softplus = 1
        for i, d in enumerate(a.dir):
            d.dt_rank, d.reverse_time = pad, i
            for f in ("h0", "h_last", "decay", "ckpt", "ypre"):
                if cls is N.ScanClArgs and hasattr(d, f):
                    setattr(d, f, None)
        return a
    for cls, fn in ((N.ScanClArgs, "cm_scan_cl_fwd"), (N.ScanClBwdArgs, "cm_scan_cl_bwd")):
        _refused(fn, scan(cls, dstate=8), N.CM_EUNSUPPORTED, "dstate")
        _refused(fn, scan(cls, pad=48), N.CM_EUNSUPPORTED, "dt_rank")
        _refused(fn, scan(cls, dtype=N.CM_F32, pad=32), N.CM_EUNSUPPORTED, "bf16")
        _refused(fn, scan(cls, dim=300), N.CM_EUNSUPPORTED, "dim")
    cb = _filled(N.ConvClBwdArgs(), skip=("stream", "workspace"))
    cb.batch, cb.seqlen, cb.dim, cb.width, cb.io_dtype = 2, 19, 512, 3, N.CM_BF16
    _refused("cm_conv_cl_bwd", cb, N.CM_EUNSUPPORTED, "width")
    want = {"expand2": True, "dt_rank16": True, "dt_rank17": False, "dt_rank32": False, "dt_rank33": False, "expand1p5_d200": False,
            "d_state8": False, "d_conv3": False, "opt_bias": False, "opt_no_conv_bias": False, "opt_no_devide": True,
            "opt_layer_scale": False, "causal_expand1": True, "causal_dt_rank24": False}           # fp32: dt_rank <= 16 only
    for name, ok in want.items():
        case, enc, _, _, _ = built(name)
        x = _cuda_like((3, 37, case.d_model))
        assert mixer_rows.supported(enc.layers[0].mamba, x) == ok, name
        assert R.train_kernels(case, torch.float32)["cm_scan_cl_bwd"] == ok, name


def test_depthwise_conv_and_weight_gradient_limits(built):
    """cm_dwconv_cl_fwd: 33 taps -> CM_EUNSUPPORTED, and convmod_rows.supported stops at 32.  cm_wgrad_bf16: m 4224 (past 4096) and
    n 192 (no multiple of 128) -> CM_EUNSUPPORTED, as cm_wgrad_supported says."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd.modules import convmod_rows
    a = _filled(N.DwconvClArgs(), skip=("stream", "partial", "dy", "dx", "dweight", "dbias"))
    a.batch, a.dim, a.seqlen, a.ksize, a.pad_left, a.io_dtype = 3, 256, 37, 33, 16, N.CM_F32
    _refused("cm_dwconv_cl_fwd", a, N.CM_EUNSUPPORTED, "dwconv")
    for name, ok in (("k31", True), ("k15", True), ("k32_causal", True), ("k33", False)):
        case, enc, _, _, _ = built(name)
        assert convmod_rows.supported(enc.layers[0].convolution_module, _cuda_like((3, 37, 256))) == ok, name
    lib = N.lib()
    for m, n, ok in ((4096, 256, 1), (4224, 256, 0), (256, 192, 0), (128, 128, 1)):
        assert lib.cm_wgrad_supported(111, m, n) == ok
        if not ok:
            w = _filled(N.WgradArgs())
            w.rows, w.m, w.n, w.lda, w.ldb = 111, m, n, m, n
            _refused("cm_wgrad_bf16", w, N.CM_EUNSUPPORTED, "wgrad")


def test_native_gemm_limits_and_gemm_supported():
    """cm_gemm_bf16 (the opt-in CM_NATIVE_GEMM route): K 96 (no multiple of 64), N 264 (none of 256) and the residual epilogue at
    N 512 -> CM_EUNSUPPORTED; ops.gemm_supported says the same."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    for n, k, ep, word in ((256, 96, 0, "K"), (264, 256, 0, "N"), (512, 256, 2, "epilogue 2")):
        a = _filled(N.GemmArgs())
        a.M, a.N, a.K, a.epilogue, a.lda, a.ldw, a.ldo, a.alpha = 65, n, k, ep, k, k, n, 1.0
        _refused("cm_gemm_bf16", a, N.CM_EUNSUPPORTED, word)
        assert not ops.gemm_supported(65, n, k, ep)
    assert ops.gemm_supported(65, 256, 256, 2) and ops.gemm_supported(65, 512, 64, 0) and ops.gemm_supported(65, 1024, 256, 1)


def test_library_gemm_count_of_the_default_layer():
    """The table's GEMM arithmetic on the layers test_encoder_routes_gpu.py recorded on MI355X: none on the default layer."""
    bf = torch.bfloat16
    assert R.library_gemms(R.CASES["expand2"], bf) == 0 and R.library_gemms(R.CASES["expand8"], bf) == 0
    assert R.library_gemms(R.CASES["opt_bias"], bf) == 2 and R.library_gemms(R.CASES["opt_layer_scale"], bf) == 1
    assert R.library_gemms(R.CASES["dt_rank40"], bf) == 3 and R.library_gemms(R.CASES["expand2"], torch.float32) is None
