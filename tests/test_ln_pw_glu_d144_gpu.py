"""cm_ln_pw_glu at d_model 144 (csrc/fused_d144.hip): x_out = x + y; g = GLU(LayerNorm(x_out) @ W^T + b), W (288, 144).

  * against fp64 torch on the CPU with the same bf16 operands, beside the route it replaces (cm_add_layernorm + library addmm + GLU
    in torch, as fused._tail / layer_forward run it): within 1.5 x that route's max abs error;
  * bit-for-bit: a token's outputs depend neither on its position nor on the launch's row count; x_out may alias x;
  * widths other than 256 and 144 are refused without a launch (CPU).
"""
import ctypes as C

import pytest
import torch

DEV = "cuda"
D = 144
ROWS = (1, 63, 64, 65, 200)


def _case(rows, seed=0):
    g = torch.Generator().manual_seed(4100 + seed + rows)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(rows, D), y=r(rows, D).bfloat16(), w=(r(2 * D, D) * 0.05).bfloat16(), bias=r(2 * D) * 0.1,
                ln_g=1.0 + 0.1 * r(D), ln_b=0.1 * r(D), eps=1e-5)


def _reference(c, with_y):
    xo = c["x"].double() + (c["y"].double() if with_y else 0.0)
    h = torch.nn.functional.layer_norm(xo, (D,), c["ln_g"].double(), c["ln_b"].double(), c["eps"])
    pw = h @ c["w"].double().t() + c["bias"].double()
    return xo, pw[:, :D] * torch.sigmoid(pw[:, D:])


class _Dev:
    def __init__(self, c):
        from mamba_asr_amd import ops
        self.x, self.y, self.w, self.bias = c["x"].to(DEV), c["y"].to(DEV), c["w"].to(DEV), c["bias"].to(DEV)
        self.ln = (c["ln_g"].to(DEV), c["ln_b"].to(DEV), c["eps"])
        self.wp = ops.PackedWeight(self.w, pad=(2 * D, 160))

    def kernel(self, x=None, y="own", x_out="new"):
        from mamba_asr_amd import ops
        x = self.x if x is None else x
        y = self.y if isinstance(y, str) else y
        xo = torch.empty_like(x) if isinstance(x_out, str) else x_out
        return xo, ops.ln_pw_glu(x, y, 1.0, self.ln, self.wp, self.bias, x_out=xo)

    def library(self, with_y):
        from mamba_asr_amd import ops
        xo, h = ops.add_layernorm(self.x, self.y if with_y else None, 1.0, x_out=torch.empty_like(self.x), norm2=self.ln,
                                  out_dtype=torch.bfloat16)
        pw = torch.addmm(self.bias.bfloat16(), h, self.w.t())
        return xo, torch.nn.functional.glu(pw, dim=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("with_y", [True, False], ids=["y", "no-y"])
@pytest.mark.parametrize("rows", ROWS)
def test_kernel_vs_fp64_beside_the_library_route(rows, with_y):
    """Max abs error against fp64 measured on MI355X, library route / kernel:
        rows   1    y: x_out 1.192e-07 / 1.192e-07, gated 3.269e-03 / 3.209e-03
        rows   1 no y: x_out 0.000e+00 / 0.000e+00, gated 4.464e-03 / 2.711e-03
        rows  63    y: x_out 2.384e-07 / 2.384e-07, gated 5.660e-03 / 4.905e-03
        rows  63 no y: x_out 0.000e+00 / 0.000e+00, gated 7.317e-03 / 5.286e-03
        rows  64    y: x_out 2.384e-07 / 2.384e-07, gated 8.762e-03 / 4.523e-03
        rows  64 no y: x_out 0.000e+00 / 0.000e+00, gated 6.741e-03 / 5.142e-03
        rows  65    y: x_out 2.384e-07 / 2.384e-07, gated 6.337e-03 / 4.389e-03
        rows  65 no y: x_out 0.000e+00 / 0.000e+00, gated 6.737e-03 / 4.496e-03
        rows 200    y: x_out 2.384e-07 / 2.384e-07, gated 7.896e-03 / 5.222e-03
        rows 200 no y: x_out 0.000e+00 / 0.000e+00, gated 7.597e-03 / 5.710e-03
    (the library route rounds the 288-wide pointwise output to bf16 before the GLU; the kernel gates in fp32)"""
    c = _case(rows)
    want_x, want_g = _reference(c, with_y)
    d = _Dev(c)
    xo, g = d.kernel(y="own" if with_y else None)
    xl, gl = d.library(with_y)
    torch.cuda.synchronize()
    assert torch.isfinite(xo).all() and torch.isfinite(g.float()).all() and g.shape == (rows, D) and g.dtype == torch.bfloat16
    err = lambda a, b: (a.cpu().double() - b).abs().max().item()
    e, el = (err(xo, want_x), err(g, want_g)), (err(xl, want_x), err(gl, want_g))
    print(f"rows {rows} {'y' if with_y else 'no y'}: max|err| vs fp64  x_out: library {el[0]:.3e}, kernel {e[0]:.3e};  "
          f"gated: library {el[1]:.3e}, kernel {e[1]:.3e}")
    assert e[0] <= 1.5 * el[0]
    assert e[1] <= 1.5 * el[1]


@pytest.mark.gpu
def test_token_outputs_do_not_depend_on_position_or_row_count():
    d = _Dev(_case(200, seed=1))
    xo, g = d.kernel()
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(5)).to(DEV)
    xo_p, g_p = d.kernel(x=d.x[perm].contiguous(), y=d.y[perm].contiguous())
    assert torch.equal(xo_p, xo[perm]) and torch.equal(g_p, g[perm])
    for n in (1, 63, 65):                                            # another launch size, another tile position for most rows
        xo_n, g_n = d.kernel(x=d.x[200 - n:].contiguous(), y=d.y[200 - n:].contiguous())
        assert torch.equal(xo_n, xo[200 - n:]) and torch.equal(g_n, g[200 - n:])


@pytest.mark.gpu
def test_x_out_may_alias_x():
    d = _Dev(_case(200, seed=2))
    xo, g = d.kernel()
    x2 = d.x.clone()
    xo2, g2 = d.kernel(x=x2, x_out=x2)
    assert xo2.data_ptr() == x2.data_ptr() and torch.equal(xo2, xo) and torch.equal(g2, g)


@pytest.mark.gpu
def test_python_layer_wants_the_padded_image():
    from mamba_asr_amd import ops
    d = _Dev(_case(8, seed=3))
    with pytest.raises(RuntimeError, match="padded"):
        ops.ln_pw_glu(d.x, d.y, 1.0, d.ln, ops.PackedWeight(torch.zeros(288, 160, dtype=torch.bfloat16, device=DEV)), d.bias)
    with pytest.raises(RuntimeError, match="256"):
        ops.ln_pw_glu(torch.zeros(8, 128, device=DEV), None, 1.0, d.ln, d.wp, d.bias)


# ---- argument refusal: no GPU, no launch -------------------------------------------------------------------------------
def test_entry_point_refuses_other_widths_without_a_launch():
    import mamba_asr_amd._native as N
    lib = N.lib()
    fields = dict(N.LnPwGluArgs._fields_)
    for dim in (128, 160, 0):
        a = N.LnPwGluArgs()
        a.rows, a.dim, a.alpha, a.eps = 64, dim, 1.0, 1e-5
        for i, k in enumerate(("x", "ln_g", "ln_b", "w", "bias", "x_out", "out")):      # never dereferenced
            setattr(a, k, C.cast(C.c_void_p(0x10000000 * (i + 1)), fields[k]))
        assert lib.cm_ln_pw_glu(C.byref(a)) == -2, dim                                   # CM_EUNSUPPORTED
    assert b"ln_pw_glu" in lib.cm_last_error()
