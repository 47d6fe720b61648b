"""The small row kernels against plain fp64 restatements, at the shapes where each takes another path.

  * cm_add_layernorm (csrc/elementwise_cl.hip): its NV = 1 / 2 / 4 instances, its four y / out dtype instances, the x-only and
    y-only forms, every norm form, out_act, want_out=False, x_out aliasing x, exact and ill-conditioned rows         [GPU]
    and its argument validation, fp16 included, without a launch                                                    [CPU]
  * cm_causal_conv1d_update, cm_selective_state_update (csrc/state_update.hip): four steps from random states, every
    optional input present and absent, widths and state sizes cm_mamba_step is not built for, and one cross-check of the
    two-kernel route against cm_mamba_step                                                                         [GPU]
  * cm_sum_leading (csrc/reduce_util.hip): the fixed order bit for bit, the four dtype instances                    [GPU]
  * the GLU forward / backward of cm_bias_act_dropout_* (csrc/ffn_train.hip) with its dbias column layout          [GPU]

Bounds: tests/test_mamba_step_fused.py's.  fp32 results: rtol 2e-3, atol 2e-4 x max(1, max|ref|).  bf16 results: against the fp64
result rounded to bf16, rtol 2e-2 and the same atol.  fp32 states keep the fp32 bound.  Every reference is torch in fp64 on the
CPU, fed the inputs as the kernel sees them (bf16 inputs are rounded first).  Each test prints its worst error and the largest
error / allowance ratio per kernel and result dtype.

The dbias bound of the GLU backward.  rows x 2^-24 x sum|da| per column bounds the error of SUMMING exact da's in fp32; it has no
room for the error of the da's themselves, and at rows = 1 it asks for |dbias - da| <= half an fp32 ulp of da: a correctly
rounded sigmoid.  The kernel's sigmoid is rcp(1 + exp2(-log2e t)): the exponent's rounding (|t| 2^-24 relative on e^-t), v_exp_f32
and v_rcp_f32 (one ulp = 2 x 2^-24 each) and the add give |sg error| <= [(|t| + 2) sg (1 - sg) + 3 sg] 2^-24 <= 3.8 x 2^-24, hence
|d1 error| <= 4.8 x 2^-24 |dy| and, with v = a1 + b1 and 1 - sg inheriting sg's absolute error, |d2 error| <= 5.8 x 2^-24 |dy v|.
Where the kernel sums da's rounded to bf16, each carries up to half a bf16 ulp = 2^-8 |da| (8 significant bits), not 2^-9: at
rows = 1 dbias IS one rounded da.  The test therefore holds dbias to
    rows 2^-24 sum|da|  +  8 x 2^-24 sum_rows |dy| (value half) or |dy v| (gate half)  (+ 2^-8 sum|da| in bf16)
and prints the error against the bound as first proposed (rows 2^-24 sum|da| (+ 2^-9 sum|da|)) as well.
"""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda"
gpu = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
WORST = {}                              # (kernel, result dtype) -> [max |err|, max err / allowance]


def check(kernel, got, ref64):
    """The project's bound (see the module docstring); records the worst error per kernel and result dtype."""
    bf = got.dtype == BF16
    want = (ref64.to(BF16) if bf else ref64).double()
    rtol, atol = (2e-2 if bf else 2e-3), 2e-4 * max(1.0, float(want.abs().max()))
    g = got.detach().double().cpu()
    assert g.shape == want.shape, (kernel, g.shape, want.shape)
    err = (g - want).abs()
    w = WORST.setdefault((kernel, "bf16" if bf else "fp32"), [0.0, 0.0])
    w[0], w[1] = max(w[0], float(err.max())), max(w[1], float((err / (atol + rtol * want.abs())).max()))
    torch.testing.assert_close(g, want, rtol=rtol, atol=atol, msg=lambda m: f"{kernel}: {m}")
    return float(err.max())


def report(kernel):
    for (k, dt), (e, r) in sorted(WORST.items()):
        if k.startswith(kernel):
            print(f"worst {k} [{dt} result]: max|err| {e:.3e}, max err / allowance {r:.3f} (allowance: rtol {2e-2 if dt == 'bf16' else 2e-3}, "
                  f"atol 2e-4 x max(1, max|ref|))")


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------
# cm_add_layernorm: validation without a GPU
# ----------------------------------------------------------------------------------------------------------
def _host_add_ln_args():
    import mamba_asr_amd._native as N
    host = (C.c_char * 256)()
    base = (C.addressof(host) + 63) // 64 * 64
    a = N.AddLnArgs()
    a.rows, a.dim, a.y_dtype, a.out_dtype, a.out_act = 2, 8, N.CM_BF16, N.CM_F32, 0
    for f in ("x", "y", "g1", "b1", "g2", "b2", "x_out", "out"):
        setattr(a, f, base)
    return a, base, host


def test_add_layernorm_rejects_dtypes_act_and_dims_without_launching():
    """CM_F16 y / out, out_act 2, dim 6 and dim 1028 -> CM_EUNSUPPORTED (-2) before anything is launched: the pointers are host
    memory and there may be no GPU at all."""
    import mamba_asr_amd._native as N
    lib = N.lib()
    a, _, _host = _host_add_ln_args()
    for field, bad in (("y_dtype", N.CM_F16), ("out_dtype", N.CM_F16), ("out_act", 2), ("dim", 6), ("dim", 1028), ("y_dtype", 7),
                       ("out_dtype", -1), ("out_act", -1)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert lib.cm_add_layernorm(C.byref(a)) == -2, (field, bad)
        assert b"add_layernorm" in lib.cm_last_error()
        setattr(a, field, good)
    # the dtype of an absent tensor is not read
    a.y, a.y_dtype, a.x, a.x_out = None, N.CM_F16, a.x + 4, None
    assert lib.cm_add_layernorm(C.byref(a)) == -3


def test_add_layernorm_rejects_misaligned_and_null_without_launching():
    import mamba_asr_amd._native as N
    lib = N.lib()
    assert lib.cm_add_layernorm(None) == -1
    a, base, _host = _host_add_ln_args()
    for field in ("x", "x_out"):
        for off in (4, 8):
            setattr(a, field, base + off)
            assert lib.cm_add_layernorm(C.byref(a)) == -3, (field, off)
            assert b"16-byte" in lib.cm_last_error()
        setattr(a, field, base)
    a.x, a.y = None, None
    assert lib.cm_add_layernorm(C.byref(a)) == -1
    a.x = base
    a.rows = 0
    assert lib.cm_add_layernorm(C.byref(a)) == -1
    a.rows, a.b2 = 2, None
    assert lib.cm_add_layernorm(C.byref(a)) == -1                            # LayerNorm weight without bias


def test_sum_leading_and_glu_reject_without_launching():
    """cm_sum_leading: an fp16 input -> -2, n no multiple of the 16-byte vector -> -3; the GLU form of cm_bias_act_dropout_*:
    dim 1032 (> 1024) and dim 12 (2 dim / 8 odd) -> -2.  Host pointers, nothing launched."""
    import mamba_asr_amd._native as N
    lib = N.lib()
    host = (C.c_char * 256)()
    base = (C.addressof(host) + 63) // 64 * 64
    assert lib.cm_sum_leading(base, base, 3, 8, N.CM_F16, N.CM_F32, None) == -2
    assert lib.cm_sum_leading(base, base, 3, 8, N.CM_F32, N.CM_F16, None) == -2
    assert lib.cm_sum_leading(base, base, 3, 6, N.CM_F32, N.CM_F32, None) == -3
    assert lib.cm_sum_leading(base, base, 3, 12, N.CM_BF16, N.CM_F32, None) == -3
    assert lib.cm_sum_leading(base + 4, base, 3, 8, N.CM_F32, N.CM_F32, None) == -3
    with pytest.raises(RuntimeError, match=r"cm_sum_leading failed \(code -2\)"):
        N.check(lib.cm_sum_leading(base, base, 3, 8, N.CM_F16, N.CM_F32, None), "cm_sum_leading")
    for dim in (1032, 12):
        a = N.FfnElemArgs()
        a.rows, a.dim, a.io_dtype, a.act, a.alpha = 3, dim, N.CM_F32, 2, 1.0
        a.a = a.y = a.dy = a.da = a.dbias = a.dbias_part = base
        assert lib.cm_bias_act_dropout_fwd(C.byref(a)) == -2, dim
        assert lib.cm_bias_act_dropout_bwd(C.byref(a)) == -2, dim


# ----------------------------------------------------------------------------------------------------------
# cm_add_layernorm vs fp64
# ----------------------------------------------------------------------------------------------------------
def ref_add_ln(x, y, alpha, n1, n2, act=0):
    """-> (x_out, out) in fp64.  norm = (weight, bias, eps) or None."""
    r = 0.0 if x is None else x.double()
    if y is not None:
        r = r + alpha * y.double()
    d = r.shape[-1]
    if n1 is not None:
        r = F.layer_norm(r, (d,), n1[0].double(), n1[1].double(), n1[2])
    out = r
    if n2 is not None:
        out = F.layer_norm(r, (d,), n2[0].double(), n2[1].double(), n2[2])
    if act == 1:
        out = torch.where(out > 0, out, 0.01 * out)
    return r, out


def _norms(d, g):
    mk = lambda eps: (1.0 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g), eps)
    return mk(1e-5), mk(1e-6)


def _dev_norm(n):
    return None if n is None else (n[0].to(DEV), n[1].to(DEV), n[2])


def _run_add_ln(x, y, alpha, n1, n2, odt, alias=False, **kw):
    from mamba_asr_amd import ops
    ref = x if x is not None else y
    xd = None if x is None else x.to(DEV).clone()                             # aliased calls overwrite it
    xo = xd if alias else torch.full(ref.shape, -7.0, device=DEV)
    return ops.add_layernorm(xd, None if y is None else y.to(DEV), alpha, norm1=_dev_norm(n1), norm2=_dev_norm(n2), x_out=xo,
                             out_dtype=odt, **kw)


ADD_LN_DIMS = [4, 144, 256, 260, 512, 640, 1024]     # NV 1: 4, 144, 256; NV 2: 260, 512; NV 4: 640, 1024


@gpu
@pytest.mark.parametrize("dim", ADD_LN_DIMS)
def test_add_layernorm_vs_fp64(dim):
    """Every (norm form) x (y dtype) x (out dtype) at every dim, the three input forms and the three row counts (none a multiple
    of the 4 rows of a workgroup) cycling underneath, plus the earlier direct case (x + 0.5 y, both norms, 35 rows) in both
    dtypes.  x_out and out are both compared."""
    g = gen(100 + dim)
    n1, n2 = _norms(dim, g)
    combos = [(nf, ydt, odt, i % 3, (1, 5, 35)[(i // 3) % 3])
              for i, (nf, ydt, odt) in enumerate(itertools.product(("n1", "both", "n2", "none"), (F32, BF16), (F32, BF16)))]
    combos += [("both", F32, F32, 0, 35), ("both", BF16, BF16, 0, 35)]
    for nf, ydt, odt, form, rows in combos:
        x = None if form == 2 else torch.randn(rows, dim, generator=g) * 1.5 + 0.3
        y = None if form == 1 else (torch.randn(rows, dim, generator=g) * 2.0 - 0.5).to(ydt)
        alpha = 0.5 if form == 0 else 1.0
        a1, a2 = (n1 if nf in ("n1", "both") else None), (n2 if nf in ("n2", "both") else None)
        xo, out = _run_add_ln(x, y, alpha, a1, a2, odt)
        rx, ro = ref_add_ln(x, y, alpha, a1, a2)
        assert xo.dtype == F32 and out.dtype == odt
        ex, eo = check("add_layernorm x_out", xo, rx), check("add_layernorm out", out, ro)
        print(f"add_ln dim {dim} rows {rows} form {('x+y', 'x', 'y')[form]} norms {nf} y {ydt} out {odt}: max|x_out err| {ex:.3e} max|out err| {eo:.3e}")
    report("add_layernorm")


@gpu
@pytest.mark.parametrize("dim", [144, 512, 1024])
def test_add_layernorm_alias_want_out_and_repeat(dim):
    """x_out aliasing x (every seam of the encoder) == the non-aliased call, bit for bit; want_out=False writes x_out and returns
    None; two calls give the same bits."""
    g = gen(200 + dim)
    n1, n2 = _norms(dim, g)
    x, y = torch.randn(35, dim, generator=g), torch.randn(35, dim, generator=g).to(BF16)
    xo, out = _run_add_ln(x, y, 0.5, n1, n2, BF16)
    xo_a, out_a = _run_add_ln(x, y, 0.5, n1, n2, BF16, alias=True)
    assert torch.equal(xo, xo_a) and torch.equal(out, out_a), "x_out aliasing x changes the result"
    xo_b, out_b = _run_add_ln(x, y, 0.5, n1, n2, BF16)
    assert torch.equal(xo, xo_b) and torch.equal(out, out_b), "cm_add_layernorm is not bit-identical from run to run"
    xo_n, none = _run_add_ln(x, y, 0.5, n1, None, BF16, want_out=False)
    assert none is None
    check("add_layernorm x_out", xo_n, ref_add_ln(x, y, 0.5, n1, None)[0])
    assert torch.equal(xo_n, xo)                                             # x_out does not depend on what follows it


@gpu
@pytest.mark.parametrize("ydt,odt", [(BF16, BF16), (F32, F32), (BF16, F32)], ids=["bf16", "fp32", "bf16-fp32"])
def test_add_layernorm_leaky_relu_front_end_call(ydt, odt):
    """The CNN front end's call: x=None, dim 640, out_act=1 = LeakyReLU(0.01) after LN2."""
    from mamba_asr_amd import ops
    g = gen(300)
    _, n2 = _norms(640, g)
    y = (torch.randn(5, 640, generator=g) * 2.0).to(ydt)
    _, ro = ref_add_ln(None, y, 1.0, None, n2, act=1)
    assert float((ro > 0.05).double().mean()) > 0.3 and float((ro < -0.0005).double().mean()) > 0.3     # both branches
    _, out = ops.add_layernorm(None, y.to(DEV), norm2=_dev_norm(n2), out_dtype=odt, out_act=1)
    print(f"add_ln LeakyReLU y {ydt} out {odt}: max|err| {check('add_layernorm out', out, ro):.3e}")
    _, plain = ops.add_layernorm(None, y.to(DEV), norm2=_dev_norm(n2), out_dtype=odt, out_act=0)
    check("add_layernorm out", plain, ref_add_ln(None, y, 1.0, None, n2)[1])


@gpu
@pytest.mark.parametrize("dim", [144, 260, 640])
def test_add_layernorm_constant_rows_give_the_bias_exactly(dim):
    """Rows whose entries are one small integer: the mean is exact, every deviation is 0, so LN(r) == bias to the bit (bf16 out:
    the bias rounded), whatever the weight.  A one-pass variance, or padding lanes counted into the statistics, break this."""
    g = gen(400 + dim)
    n1, n2 = _norms(dim, g)
    vals = torch.tensor([-3.0, -1.0, 0.0, 2.0, 5.0])
    x = vals[:, None].expand(5, dim).contiguous()
    y = (2.0 * vals.flip(0))[:, None].expand(5, dim).contiguous().to(BF16)   # x + 0.5 y: constant rows again
    for yy in (None, y):
        xo, out = _run_add_ln(x, yy, 0.5, None, n2, F32)
        assert torch.equal(out.cpu(), n2[1].expand(5, dim)), "LN2 of constant rows is not the bias"
        assert torch.equal(xo.cpu(), ref_add_ln(x, yy, 0.5, None, None)[0].float())
        xo, out = _run_add_ln(x, yy, 0.5, n1, None, BF16)
        assert torch.equal(xo.cpu(), n1[1].expand(5, dim)), "LN1 of constant rows is not the bias"
        assert torch.equal(out.cpu(), n1[1].to(BF16).expand(5, dim))


@gpu
@pytest.mark.parametrize("dim", [144, 512, 1024])
def test_add_layernorm_large_mean_rows(dim):
    """Rows of 1000 + randn: the two-pass variance keeps the fp32 bound (E[x^2] - mean^2 in fp32 would lose the variance: 1e6 x 2^-24
    is 6 % of it)."""
    g = gen(500 + dim)
    _, n2 = _norms(dim, g)
    x = 1000.0 + torch.randn(5, dim, generator=g)
    xo, out = _run_add_ln(x, None, 1.0, None, n2, F32)
    assert torch.equal(xo.cpu(), x)
    print(f"add_ln 1000 + randn dim {dim}: max|err| {check('add_layernorm out (1000 + randn)', out, ref_add_ln(x, None, 1.0, None, n2)[1]):.3e}")
    report("add_layernorm out (1000")


@gpu
def test_add_layernorm_refuses_fp16():
    """An fp16 y or out_dtype raises before the native call; x_out keeps its sentinel (nothing ran)."""
    from mamba_asr_amd import ops
    x = torch.randn(5, 144, generator=gen(600)).to(DEV)
    ln = (torch.ones(144, device=DEV), torch.zeros(144, device=DEV), 1e-5)
    for kw in (dict(y=x.to(torch.float16), out_dtype=BF16), dict(y=x.to(BF16), out_dtype=torch.float16), dict(y=None, out_dtype=torch.float16)):
        xo = torch.full_like(x, -7.0)
        with pytest.raises(RuntimeError, match="must be fp32 or bf16"):
            ops.add_layernorm(x, kw["y"], 0.5, norm2=ln, x_out=xo, out_dtype=kw["out_dtype"])
        torch.cuda.synchronize()
        assert bool((xo == -7.0).all())
    with pytest.raises(RuntimeError, match=r"cm_add_layernorm failed \(code -2\)"):
        ops.add_layernorm(x, None, norm2=ln, out_dtype=BF16, out_act=2)


# ----------------------------------------------------------------------------------------------------------
# cm_causal_conv1d_update vs fp64
# ----------------------------------------------------------------------------------------------------------
def ref_conv_update(state, x, w, bias, silu):
    state = torch.cat([state[:, :, 1:], x[:, :, None]], dim=-1)                  # shift left, append
    out = (state * w[None]).sum(-1)
    if bias is not None:
        out = out + bias
    return (out * torch.sigmoid(out) if silu else out), state


@gpu
@pytest.mark.parametrize("batch,dim,width", [(1, 8, 4), (3, 100, 2), (2, 288, 3), (5, 130, 4), (2, 24, 1)])
def test_causal_conv1d_update_vs_fp64(batch, dim, width):
    """Four consecutive steps from a random non-zero state; out and the whole state after every step.  The state is data
    movement only: it equals "shift left, append x" exactly.  5 x 130 = 650 threads: no multiple of the 256-thread workgroup."""
    from mamba_asr_amd import ops
    g = gen(1000 * dim + 10 * width + batch)
    w, b = torch.randn(dim, width, generator=g) * 0.5, torch.randn(dim, generator=g) * 0.3
    for dtype, has_bias, silu in itertools.product((F32, BF16), (True, False), (True, False)):
        st0 = torch.randn(batch, dim, width, generator=g)
        xs = [(torch.randn(batch, dim, generator=g) * 1.5).to(dtype) for _ in range(4)]
        bias = b if has_bias else None
        st, rst = st0.to(DEV).clone(), st0.double()
        for i, x in enumerate(xs):
            out = ops.causal_conv1d_update(x.to(DEV), st, w.to(DEV), None if bias is None else bias.to(DEV), silu=silu)
            rout, rst = ref_conv_update(rst, x.double(), w.double(), None if bias is None else bias.double(), silu)
            assert out.dtype == dtype and out.shape == (batch, dim)
            e = check("causal_conv1d_update out", out, rout)
            assert torch.equal(st.cpu(), rst.float()), f"conv state after step {i} is not shift-left-append"
            print(f"conv_update ({batch}, {dim}, {width}) {dtype} bias {has_bias} silu {silu} step {i}: max|out err| {e:.3e}")
    report("causal_conv1d_update")


# ----------------------------------------------------------------------------------------------------------
# cm_selective_state_update vs fp64
# ----------------------------------------------------------------------------------------------------------
def ref_state_update(state, x, dt, A, B, Cm, D, z, dt_bias, softplus):
    if dt_bias is not None:
        dt = dt + dt_bias
    if softplus:
        dt = F.softplus(dt)
    state = state * torch.exp(dt[:, :, None] * A[None]) + dt[:, :, None] * B[:, None, :] * x[:, :, None]
    y = (state * Cm[:, None, :]).sum(-1)
    if D is not None:
        y = y + D * x
    if z is not None:
        y = y * (z * torch.sigmoid(z))
    return y, state


@gpu
@pytest.mark.parametrize("batch,dim,dstate", [(1, 8, 16), (3, 100, 8), (2, 288, 1), (5, 130, 64)])
def test_selective_state_update_vs_fp64(batch, dim, dstate):
    """Four consecutive steps with the state updated in place; y and the state after every step, for every subset of D / z / dt_bias,
    dt_softplus on and off, both dtypes.  With softplus, dt + dt_bias spans -30 .. +30: cm_softplus's three branches (exp below
    -15, the identity above 20, log(1 + exp) between)."""
    from mamba_asr_amd import ops
    g = gen(1000 * dim + 10 * dstate + batch)
    A = -torch.exp(torch.randn(dim, dstate, generator=g) * 0.5)
    Dw = torch.randn(dim, generator=g)
    dv = lambda t: None if t is None else t.to(DEV)
    for dtype, has_D, has_z, has_b, sp in itertools.product((F32, BF16), (True, False), (True, False), (True, False), (True, False)):
        st0 = torch.randn(batch, dim, dstate, generator=g)
        st, rst = st0.to(DEV).clone(), st0.double()
        db = None if not has_b else ((torch.rand(dim, generator=g) - 0.5) if sp else torch.rand(dim, generator=g) * 0.2)
        worst_y = worst_s = 0.0
        for i in range(4):
            rn = lambda *s: torch.randn(*s, generator=g).to(dtype)
            x, B, Cm, z = rn(batch, dim), rn(batch, dstate), rn(batch, dstate), (rn(batch, dim) if has_z else None)
            u = torch.rand(batch, dim, generator=g)
            dt = (u * 59.0 - 29.5 if sp else u * 0.5 + 0.01).to(dtype)
            if sp:
                t = dt.float() + (db if db is not None else 0.0)
                assert float(t.min()) < -15.0 and float(t.max()) > 20.0 or batch * dim < 64
            y = ops.selective_state_update(st, dv(x), dv(dt), dv(A), dv(B), dv(Cm), dv(Dw if has_D else None), dv(z), dv(db), dt_softplus=sp)
            d64 = lambda t: None if t is None else t.double()
            ry, rst = ref_state_update(rst, d64(x), d64(dt), d64(A), d64(B), d64(Cm), d64(Dw if has_D else None), d64(z), d64(db), sp)
            assert y.dtype == dtype and y.shape == (batch, dim) and st.dtype == F32
            worst_y, worst_s = max(worst_y, check("selective_state_update y", y, ry)), max(worst_s, check("selective_state_update state", st, rst))
        print(f"state_update ({batch}, {dim}, {dstate}) {dtype} D {has_D} z {has_z} dt_bias {has_b} softplus {sp}: max|y err| {worst_y:.3e} "
              f"max|state err| {worst_s:.3e}")
    report("selective_state_update")


@gpu
def test_two_kernel_step_matches_mamba_step():
    """(3, 256, 16), width 4, dt_rank 8, fp32: cm_causal_conv1d_update + the two projections (torch, fp32, as plain sums) +
    cm_selective_state_update give the y and the states of ops.mamba_step, four steps, the fp32 bound."""
    from mamba_asr_amd import ops
    batch, E, R, N = 3, 256, 8, 16
    g = gen(77)
    rn = lambda *s: torch.randn(*s, generator=g)
    w = {"conv_w": rn(E, 4) * 0.5, "conv_b": rn(E) * 0.1, "x_proj": rn(R + 2 * N, E) * E ** -0.5, "dt_proj": rn(E, R) * R ** -0.5,
         "dt_bias": rn(E) - 2.0, "A": -torch.exp(rn(E, N) * 0.5), "D": rn(E)}
    w = {k: v.to(DEV) for k, v in w.items()}
    conv0, ssm0 = rn(batch, E, 4).to(DEV), rn(batch, E, N).to(DEV)
    conv_a, ssm_a, conv_b, ssm_b = conv0.clone(), ssm0.clone(), conv0.clone(), ssm0.clone()
    for i in range(4):
        xz = rn(batch, 2 * E).to(DEV)
        ya = ops.mamba_step(xz, conv_a, ssm_a, w["conv_w"], w["conv_b"], w["x_proj"], w["dt_proj"], w["dt_bias"], w["A"], w["D"])
        x = ops.causal_conv1d_update(xz[:, :E], conv_b, w["conv_w"], w["conv_b"], silu=True)
        x_dbl = (x[:, None, :] * w["x_proj"][None]).sum(-1)                    # (batch, R + 2 N)
        dt = (x_dbl[:, None, :R] * w["dt_proj"][None]).sum(-1)                  # (batch, E)
        yb = ops.selective_state_update(ssm_b, x, dt, w["A"], x_dbl[:, R:R + N], x_dbl[:, R + N:], w["D"], xz[:, E:], w["dt_bias"], dt_softplus=True)
        e = check("two-kernel step vs mamba_step y", yb, ya.double().cpu())
        check("two-kernel step vs mamba_step state", conv_b, conv_a.double().cpu())
        es = check("two-kernel step vs mamba_step state", ssm_b, ssm_a.double().cpu())
        print(f"two-kernel step vs mamba_step, step {i}: max|y diff| {e:.3e} max|ssm diff| {es:.3e}")
    report("two-kernel")


# ----------------------------------------------------------------------------------------------------------
# cm_sum_leading
# ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("nbatch,n", [(1, 8), (3, 24), (7, 2056), (64, 256 * 48), (33, 1024 * 256)])
def test_sum_leading_fixed_order_and_fp64(nbatch, n):
    """fp32 out == the sequential fp32 sum acc = in[0]; acc = acc + in[b] bit for bit (the "fixed order" of the kernel's header);
    bf16 out within one bf16 ulp of it; against fp64, |err| <= nbatch 2^-24 sum_b |in| (any order of fp32 adds), plus the output
    rounding for bf16 out: 2^-8 |sum| (bf16 keeps 8 significant bits: half an ulp is at most 2^-8 relative).  Signs and magnitudes over 2^-6 .. 2^6 so that the order shows in the last bits.
    2056 / 8 = 257 threads: one past a workgroup; (33, 1024 x 256): the training step's largest fold."""
    from mamba_asr_amd import ops
    g = gen(nbatch * 7 + n)
    base = torch.randn(nbatch, n, generator=g) * torch.exp2(torch.randint(-6, 7, (nbatch, n), generator=g).float())
    for idt, odt in itertools.product((F32, BF16), (F32, BF16)):
        t = base.to(idt)
        seq = t[0].float().clone()
        for b in range(1, nbatch):
            seq = seq + t[b].float()
        r64, sumabs = t.double().sum(0), t.double().abs().sum(0)
        td = t.to(DEV)
        out = ops.sum_leading(td, odt)
        assert out.dtype == odt and out.shape == (n,)
        o = out.cpu()
        bound = nbatch * 2.0 ** -24 * sumabs
        if odt == F32:
            assert torch.equal(o, seq), f"cm_sum_leading {idt} -> fp32 is not the sequential fp32 sum ({int((o != seq).sum())} of {n} differ)"
        else:
            assert bool(((o.double() - seq.double()).abs() <= 2.0 ** -8 * seq.double().abs()).all()), "bf16 out is more than one bf16 ulp off"
            bound = bound + 2.0 ** -8 * (r64.abs() + bound)
        err = (o.double() - r64).abs()
        print(f"sum_leading ({nbatch}, {n}) {idt} -> {odt}: max|err vs fp64| {float(err.max()):.3e}, max err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())
        assert torch.equal(ops.sum_leading(td, odt), out), "cm_sum_leading is not bit-identical from run to run"
    # a leading axis of a higher-rank tensor (how the weight gradients arrive)
    t3 = base.view(nbatch, -1, 4).to(DEV)
    assert torch.equal(ops.sum_leading(t3).reshape(-1), ops.sum_leading(t3.view(nbatch, n)))


# ----------------------------------------------------------------------------------------------------------
# GLU forward / backward
# ----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rows,dim", [(1, 8), (17, 24), (37, 144), (33, 1024), (529, 256)])
def test_bias_glu_fwd_bwd_vs_fp64(rows, dim):
    """y = (a1 + b1) sigmoid(a2 + b2), da = [dy sg, dy (a1 + b1) sg (1 - sg)], dbias = column sums of da (2 dim, fp32), both
    dtypes, with and without bias.  The value half is 4 x the gate half, so halves that trade places (in y, da or dbias's
    column layout) cannot pass.  (33, 1024): 128 threads per row, 2 rows per pass; 529 rows = 34 partial rows: the second trip of
    colsum_partials_kernel's loop over its 32 row groups.  The dbias bound: the module docstring."""
    from mamba_asr_amd import ops
    g = gen(rows * 3 + dim)
    bias = torch.cat([torch.randn(dim, generator=g) * 2.0, torch.randn(dim, generator=g) * 0.5])
    for dtype, has_bias in itertools.product((F32, BF16), (True, False)):
        a = torch.cat([torch.randn(rows, dim, generator=g) * 4.0, torch.randn(rows, dim, generator=g)], dim=1).to(dtype)
        dy = (torch.randn(rows, dim, generator=g) * 1.5).to(dtype)
        b = bias if has_bias else None
        bd = None if b is None else b.to(DEV)
        a64, dy64, b64 = a.double(), dy.double(), (bias.double() if has_bias else torch.zeros(2 * dim, dtype=torch.float64))
        v, sg = a64[:, :dim] + b64[:dim], torch.sigmoid(a64[:, dim:] + b64[dim:])
        ry, rda = v * sg, torch.cat([dy64 * sg, dy64 * v * sg * (1 - sg)], dim=1)
        y = ops.bias_glu_fwd(a.to(DEV), bd)
        da, dbias = ops.bias_glu_bwd(dy.to(DEV), a.to(DEV), bd)
        assert y.dtype == dtype and y.shape == (rows, dim) and da.dtype == dtype and da.shape == (rows, 2 * dim)
        assert dbias.dtype == F32 and dbias.shape == (2 * dim,)
        ey, eda = check("bias_glu_fwd y", y, ry), check("bias_glu_bwd da", da, rda)
        sumabs = rda.abs().sum(0)
        issue = rows * 2.0 ** -24 * sumabs + (2.0 ** -9 * sumabs if dtype == BF16 else 0.0)       # the bound as first proposed
        summing = rows * 2.0 ** -24 * sumabs + (2.0 ** -8 * sumabs if dtype == BF16 else 0.0)
        elems = 8 * 2.0 ** -24 * torch.cat([dy64.abs().sum(0), (dy64 * v).abs().sum(0)])
        err = (dbias.double().cpu() - rda.sum(0)).abs()
        for half, sl in (("value", slice(0, dim)), ("gate", slice(dim, 2 * dim))):
            print(f"glu ({rows}, {dim}) {dtype} bias {has_bias} dbias {half} half: max|err| {float(err[sl].max()):.3e}, max err / (bound as first proposed) "
                  f"{float((err[sl] / issue[sl]).max()):.3f}, max err / (summing + element bound) {float((err[sl] / (summing + elems)[sl]).max()):.3f}")
            assert bool((err[sl] <= (summing + elems)[sl]).all()), f"dbias {half} half"
        print(f"glu ({rows}, {dim}) {dtype} bias {has_bias}: max|y err| {ey:.3e} max|da err| {eda:.3e}")
        y2 = ops.bias_glu_fwd(a.to(DEV), bd)
        da2, dbias2 = ops.bias_glu_bwd(dy.to(DEV), a.to(DEV), bd)
        assert torch.equal(y, y2) and torch.equal(da, da2) and torch.equal(dbias, dbias2), "the GLU kernels are not bit-identical from run to run"
    report("bias_glu")


@gpu
def test_bias_glu_rejects_unsupported_dims():
    """dim 1032 (> 1024) and 2 dim / 8 odd (dim 12) raise; nothing is launched."""
    from mamba_asr_amd import ops
    for dim in (1032, 12):
        a, dy = torch.zeros(3, 2 * dim, device=DEV), torch.zeros(3, dim, device=DEV)
        with pytest.raises(RuntimeError):
            ops.bias_glu_fwd(a, None)
        with pytest.raises(RuntimeError, match=r"cm_bias_act_dropout_bwd failed \(code -2\)"):
            ops.bias_glu_bwd(dy, a, None)
    torch.cuda.synchronize()
