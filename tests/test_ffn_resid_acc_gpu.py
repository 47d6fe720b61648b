"""cm_ffn_fused with the residual carried in the second GEMM's accumulators (ops.ffn_fused(..., resid_acc=), cm_ffn_args.flags).

  * against fp64 torch on the CPU with the same bf16 weights and no intermediate rounding, beside the route it replaces (the same call
    with the reload path selected): both round the normalised tokens and the hidden slab to bf16 at the same points and differ only in
    the fp32 order of the residual add, so the new path must stay within 1.5 x the reload path's max abs error (the factor covers the
    fluctuation of a maximum over elements);
  * an alpha that is no power of two takes the reload path by itself;
  * bit-for-bit: a token's outputs depend neither on its position nor on the launch's row count; x_out may alias x; repeats give
    the same bits;
  * the switch is an argument field, mirrored in _native (CPU).
"""
import os
import re

import pytest
import torch

DEV = "cuda"
D = 256
ROWS = (1, 63, 64, 65, 200)
HIDDEN = (256, 1024)
F = torch.nn.functional


def _module(r, hidden):
    return dict(pre=(1.0 + 0.1 * r(D), 0.1 * r(D), 1e-5), w1=(r(hidden, D) * D ** -0.5).bfloat16(), b1=r(hidden) * 0.1,
                w2=(r(D, hidden) * hidden ** -0.5).bfloat16(), b2=r(D) * 0.1)


def _case(rows, hidden, seed=0):
    """Inputs scaled as in test_hip_modules.py::test_ffn_fused_kernel; module a closes a layer, module b opens the next."""
    g = torch.Generator().manual_seed(2000 + seed + rows + hidden)
    r = lambda *s: torch.randn(*s, generator=g)
    ln = lambda: (1.0 + 0.1 * r(D), 0.1 * r(D), 1e-5)
    return dict(x=r(rows, D) * 2.0 + 0.5, add=r(rows, D).bfloat16(), a=_module(r, hidden), b=_module(r, hidden), n1=ln(), n2=ln())


def _ln64(t, p):
    return F.layer_norm(t, (D,), p[0].double(), p[1].double(), p[2])


def _ffn64(xin, m, alpha):
    hid = F.gelu(_ln64(xin, m["pre"]) @ m["w1"].double().t() + m["b1"].double())
    return xin + alpha * (hid @ m["w2"].double().t() + m["b2"].double())


class _Dev:
    def __init__(self, c):
        from mamba_asr_amd import ops
        d = lambda t: t.to(DEV)
        dn = lambda p: (p[0].to(DEV), p[1].to(DEV), p[2])
        self.x, self.add, self.n1, self.n2 = d(c["x"]), d(c["add"]), dn(c["n1"]), dn(c["n2"])
        self.m = {k: dict(pre=dn(c[k]["pre"]), w1=ops.PackedWeight(d(c[k]["w1"])), b1=d(c[k]["b1"]), w2=ops.PackedWeight(d(c[k]["w2"])),
                          b2=d(c[k]["b2"])) for k in ("a", "b")}

    def one(self, k, x, alpha=0.5, **kw):
        """One module, x_out a new tensor -> (x_out, h or projection)."""
        from mamba_asr_amd import ops
        m = self.m[k]
        if kw.get("x_out") is None:
            kw["x_out"] = torch.empty_like(x)
        return ops.ffn_fused(x, m["pre"], m["w1"], m["b1"], m["w2"], m["b2"], alpha=alpha, **kw)


def _err(got, want):
    assert torch.isfinite(got.float()).all()
    return (got.cpu().double() - want).abs().max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True], ids=["bare", "addend-n1-n2"])
@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_residual_in_accumulators_vs_fp64_beside_the_reload_path(rows, hidden, full):
    """Max abs error against fp64 measured on MI355X, reload path / residual in the accumulators (x_out; h):
    rows 1 hidden 1024 bare: x_out: 2.660e-03 / 2.660e-03;  h: 2.660e-03 / 2.660e-03
        rows 1 hidden 1024 full: x_out: 9.447e-04 / 9.447e-04;  h: 9.589e-04 / 9.587e-04
        rows 63 hidden 1024 bare: x_out: 3.249e-03 / 3.249e-03;  h: 3.249e-03 / 3.249e-03
        rows 63 hidden 1024 full: x_out: 1.666e-03 / 1.666e-03;  h: 1.712e-03 / 1.712e-03
        rows 64 hidden 1024 bare: x_out: 3.632e-03 / 3.632e-03;  h: 3.632e-03 / 3.632e-03
        rows 64 hidden 1024 full: x_out: 1.665e-03 / 1.665e-03;  h: 1.810e-03 / 1.810e-03
        rows 65 hidden 1024 bare: x_out: 3.425e-03 / 3.425e-03;  h: 3.425e-03 / 3.425e-03
        rows 65 hidden 1024 full: x_out: 1.912e-03 / 1.912e-03;  h: 1.772e-03 / 1.772e-03
        rows 200 hidden 1024 bare: x_out: 3.481e-03 / 3.481e-03;  h: 3.481e-03 / 3.481e-03
        rows 200 hidden 1024 full: x_out: 1.800e-03 / 1.801e-03;  h: 2.152e-03 / 2.152e-03
    (hidden 256: the same picture, 1.3e-03 .. 3.7e-03, the two paths equal to three digits)"""
    c = _case(rows, hidden)
    xin = c["x"].double() + (0.7 * c["add"].double() if full else 0.0)
    want_x = _ffn64(xin, c["a"], 0.5)
    if full:
        want_x = _ln64(want_x, c["n1"])
    want_h = _ln64(want_x, c["n2"]) if full else want_x
    d = _Dev(c)
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2) if full else {}
    err = {}
    for name, racc in (("reload", False), ("acc", True)):
        xo, h = d.one("a", d.x, h_dtype=torch.float32, resid_acc=racc, **kw)
        torch.cuda.synchronize()
        err[name] = (_err(xo, want_x), _err(h, want_h))
    print(f"rows {rows} hidden {hidden} {'full' if full else 'bare'}: max|err| vs fp64  x_out: reload {err['reload'][0]:.3e}, "
          f"accumulators {err['acc'][0]:.3e};  h: reload {err['reload'][1]:.3e}, accumulators {err['acc'][1]:.3e}")
    assert err["acc"][0] <= 1.5 * err["reload"][0]
    assert err["acc"][1] <= 1.5 * err["reload"][1]


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", HIDDEN)
def test_an_alpha_that_is_no_power_of_two_takes_the_reload_path(hidden):
    c = _case(200, hidden, seed=1)
    want_x = _ln64(_ffn64(c["x"].double() + 0.7 * c["add"].double(), c["a"], 0.3), c["n1"])
    d = _Dev(c)
    kw = dict(alpha=0.3, addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2, h_dtype=torch.float32)
    xo, h = d.one("a", d.x, **kw)
    xo_r, h_r = d.one("a", d.x, resid_acc=False, **kw)
    torch.cuda.synchronize()
    e, e_r = _err(xo, want_x), _err(xo_r, want_x)
    print(f"hidden {hidden} alpha 0.3: max|err| vs fp64  x_out: default {e:.3e}, reload {e_r:.3e}")
    assert e <= 1.5 * e_r and _err(h, _ln64(want_x, c["n2"])) <= 1.5 * _err(h_r, _ln64(want_x, c["n2"]))
    assert torch.equal(xo, xo_r) and torch.equal(h, h_r)             # the same path: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", HIDDEN)
def test_token_outputs_do_not_depend_on_position_or_row_count(hidden):
    d = _Dev(_case(200, hidden, seed=3))
    kw = dict(add_scale=0.7, norm1=d.n1, norm2=d.n2, h_dtype=torch.float32)
    xo, h = d.one("a", d.x, addend=d.add, **kw)
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(5)).to(DEV)
    xo_p, h_p = d.one("a", d.x[perm].contiguous(), addend=d.add[perm].contiguous(), **kw)
    assert torch.equal(xo_p, xo[perm]) and torch.equal(h_p, h[perm])
    for n in (1, 63, 65):                                            # another launch size, another tile position for most rows
        xo_n, h_n = d.one("a", d.x[200 - n:].contiguous(), addend=d.add[200 - n:].contiguous(), **kw)
        assert torch.equal(xo_n, xo[200 - n:]) and torch.equal(h_n, h[200 - n:])


@pytest.mark.gpu
def test_x_out_may_alias_x():
    d = _Dev(_case(200, 1024, seed=4))
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2)
    xo, h = d.one("a", d.x, **kw)
    x2 = d.x.clone()
    xo2, h2 = d.one("a", x2, x_out=x2, **kw)
    assert xo2.data_ptr() == x2.data_ptr() and torch.equal(xo2, xo) and torch.equal(h2, h)


@pytest.mark.gpu
def test_repeats_give_the_same_bits_at_32000_rows():
    g_ = torch.Generator(device=DEV).manual_seed(3)
    d = _Dev(_case(1, 1024, seed=5))
    x = torch.randn(32000, D, device=DEV, generator=g_) * 2.0 + 0.5
    add = torch.randn(32000, D, device=DEV, generator=g_).bfloat16()
    kw = dict(add_scale=0.7, norm1=d.n1, norm2=d.n2)
    first = d.one("a", x, addend=add, **kw)
    for _ in range(5):
        again = d.one("a", x, addend=add, **kw)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    tail = d.one("a", x[31936:].contiguous(), addend=add[31936:].contiguous(), **kw)
    assert torch.equal(tail[0], first[0][31936:]) and torch.equal(tail[1], first[1][31936:])


# ---- no GPU ------------------------------------------------------------------------------------------------------------
def test_the_switch_is_an_argument_field_mirrored_in_native():
    import mamba_asr_amd._native as N
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "conmamba_hip.h")).read()
    assert int(re.search(r"^#define CM_FFN_RELOAD_RESIDUAL (\d+)$", hdr, re.M).group(1)) == N.CM_FFN_RELOAD_RESIDUAL == 1
    body = hdr[hdr.index("typedef struct cm_ffn_args {"):hdr.index("} cm_ffn_args;")]
    assert re.search(r"seed_epoch;.*\n\s*int32_t flags;.*\n\s*int32_t reserved_;\s*$", body)        # appended behind the last field
    assert [f[0] for f in N.FfnArgs._fields_][-3:] == ["seed_epoch", "flags", "reserved_"]
    assert N.ABI_VERSION == N.lib().cm_abi_version()
