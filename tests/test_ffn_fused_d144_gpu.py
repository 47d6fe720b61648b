"""cm_ffn_fused at d_model 144 (csrc/fused_d144.hip; ops.ffn_fused on (rows, 144) rows, images padded to 160 columns / rows).

  * against fp64 torch on the CPU with the same bf16 weights and no intermediate rounding, beside the route the encoder took at this
    width before (fused.layer_forward: cm_add_layernorm -> library Linear + GELU -> library Linear -> cm_add_layernorm): the kernel
    must stay within 1.5 x that route's max abs error (the factor covers the fluctuation of a maximum over elements; the library
    route rounds the module output to bf16 once more than the kernel, so the bound is not tight from above);
  * the projection epilogue at proj_dim 576 (2 d_inner of the recipe, no multiple of 256) and 64 (the smallest accepted);
  * an alpha that is no power of two takes the reload path by itself;
  * bit-for-bit: a token's outputs depend neither on its position nor on the launch's row count; x_out may alias x; repeats give
    the same bits at 32000 rows;
  * LayerNorm statistics count the 144 real features only (inputs offset by +50);
  * the entry point's refusals, without a launch (CPU).
"""
import ctypes as C

import pytest
import torch

DEV = "cuda"
D = 144
ROWS = (1, 63, 64, 65, 200)
HIDDEN = (256, 1024)
F = torch.nn.functional


def _module(r, hidden):
    return dict(pre=(1.0 + 0.1 * r(D), 0.1 * r(D), 1e-5), w1=(r(hidden, D) * D ** -0.5).bfloat16(), b1=r(hidden) * 0.1,
                w2=(r(D, hidden) * hidden ** -0.5).bfloat16(), b2=r(D) * 0.1)


def _case(rows, hidden, seed=0, offset=0.5):
    """test_ffn_resid_acc_gpu.py's inputs, restated for D = 144."""
    g = torch.Generator().manual_seed(2000 + seed + rows + hidden)
    r = lambda *s: torch.randn(*s, generator=g)
    ln = lambda: (1.0 + 0.1 * r(D), 0.1 * r(D), 1e-5)
    return dict(x=r(rows, D) * 2.0 + offset, add=r(rows, D).bfloat16(), a=_module(r, hidden), n1=ln(), n2=ln(),
                wp=(r(576, D) * D ** -0.5).bfloat16(), bp=r(576) * 0.1)


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
        m = c["a"]
        hidden = m["w1"].shape[0]
        self.x, self.add, self.n1, self.n2 = d(c["x"]), d(c["add"]), dn(c["n1"]), dn(c["n2"])
        self.raw = dict(pre=dn(m["pre"]), w1=d(m["w1"]), b1=d(m["b1"]).bfloat16(), w2=d(m["w2"]), b2=d(m["b2"]).bfloat16())
        self.m = dict(pre=dn(m["pre"]), w1=ops.PackedWeight(d(m["w1"]), pad=(hidden, 160)), b1=d(m["b1"]),
                      w2=ops.PackedWeight(d(m["w2"]), pad=(160, hidden)), b2=d(m["b2"]))
        self.wp_raw, self.bp = d(c["wp"]), d(c["bp"])

    def proj(self, pdim):
        from mamba_asr_amd import ops
        return ops.PackedWeight(self.wp_raw[:pdim].contiguous(), pad=(pdim, 160))

    def one(self, x, alpha=0.5, **kw):
        """The kernel, x_out a new tensor -> (x_out, h or projection)."""
        from mamba_asr_amd import ops
        m = self.m
        if kw.get("x_out") is None:
            kw["x_out"] = torch.empty_like(x)
        return ops.ffn_fused(x, m["pre"], m["w1"], m["b1"], m["w2"], m["b2"], alpha=alpha, **kw)

    def library(self, x, full, alpha=0.5, h_dtype=torch.float32):
        """fused.layer_forward's sequence around one feed-forward module -> (x_out, h)."""
        from mamba_asr_amd import ops
        m = self.raw
        if full:
            xin, h = ops.add_layernorm(x, self.add, 0.7, x_out=torch.empty_like(x), norm2=m["pre"], out_dtype=torch.bfloat16)
        else:
            xin, h = x, ops.add_layernorm(x, None, norm2=m["pre"], out_dtype=torch.bfloat16)[1]
        hid = torch._addmm_activation(m["b1"], h, m["w1"].t(), use_gelu=True)
        y = torch.addmm(m["b2"], hid, m["w2"].t())
        return ops.add_layernorm(xin, y, alpha, x_out=torch.empty_like(x), norm1=self.n1 if full else None,
                                 norm2=self.n2 if full else None, out_dtype=h_dtype)


def _err(got, want):
    assert torch.isfinite(got.float()).all()
    return (got.cpu().double() - want).abs().max().item()


def _want(c, full, alpha=0.5):
    xin = c["x"].double() + (0.7 * c["add"].double() if full else 0.0)
    want_x = _ffn64(xin, c["a"], alpha)
    if full:
        want_x = _ln64(want_x, c["n1"])
    return want_x, (_ln64(want_x, c["n2"]) if full else want_x)


@pytest.mark.gpu
@pytest.mark.parametrize("racc", [True, False], ids=["accumulators", "reload"])
@pytest.mark.parametrize("full", [False, True], ids=["bare", "addend-n1-n2"])
@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("rows", ROWS)
def test_kernel_vs_fp64_beside_the_library_route(rows, hidden, full, racc):
    """Max abs error against fp64 measured on MI355X, library route / kernel (x_out; h), residual in the accumulators:
        rows   1 hidden  256 bare: x_out: 3.804e-03 / 2.509e-03;  h: 3.804e-03 / 2.509e-03
        rows   1 hidden  256 full: x_out: 1.958e-03 / 1.006e-03;  h: 2.177e-03 / 1.121e-03
        rows  63 hidden  256 bare: x_out: 4.718e-03 / 3.152e-03;  h: 4.718e-03 / 3.152e-03
        rows  63 hidden  256 full: x_out: 2.206e-03 / 1.521e-03;  h: 2.511e-03 / 1.588e-03
        rows  64 hidden  256 bare: x_out: 5.556e-03 / 3.131e-03;  h: 5.556e-03 / 3.131e-03
        rows  64 hidden  256 full: x_out: 2.703e-03 / 1.521e-03;  h: 2.887e-03 / 1.653e-03
        rows  65 hidden  256 bare: x_out: 4.992e-03 / 3.181e-03;  h: 4.992e-03 / 3.181e-03
        rows  65 hidden  256 full: x_out: 2.326e-03 / 1.562e-03;  h: 2.320e-03 / 1.900e-03
        rows 200 hidden  256 bare: x_out: 5.109e-03 / 3.676e-03;  h: 5.109e-03 / 3.676e-03
        rows 200 hidden  256 full: x_out: 2.837e-03 / 1.684e-03;  h: 2.613e-03 / 1.683e-03
        rows   1 hidden 1024 bare: x_out: 4.550e-03 / 2.354e-03;  h: 4.550e-03 / 2.354e-03
        rows   1 hidden 1024 full: x_out: 1.663e-03 / 1.245e-03;  h: 1.778e-03 / 1.200e-03
        rows  63 hidden 1024 bare: x_out: 4.546e-03 / 3.320e-03;  h: 4.546e-03 / 3.320e-03
        rows  63 hidden 1024 full: x_out: 2.126e-03 / 1.717e-03;  h: 2.273e-03 / 1.571e-03
        rows  64 hidden 1024 bare: x_out: 3.868e-03 / 3.467e-03;  h: 3.868e-03 / 3.467e-03
        rows  64 hidden 1024 full: x_out: 2.081e-03 / 1.769e-03;  h: 2.375e-03 / 1.462e-03
        rows  65 hidden 1024 bare: x_out: 4.312e-03 / 3.375e-03;  h: 4.312e-03 / 3.375e-03
        rows  65 hidden 1024 full: x_out: 2.262e-03 / 1.481e-03;  h: 2.195e-03 / 1.584e-03
        rows 200 hidden 1024 bare: x_out: 5.396e-03 / 3.203e-03;  h: 5.396e-03 / 3.203e-03
        rows 200 hidden 1024 full: x_out: 2.794e-03 / 1.512e-03;  h: 2.818e-03 / 1.731e-03
    (the reload path, all 20 cases measured in the same run: the library column is the same launch sequence, the kernel column
    differs from the one above in 5 cases, by at most 2e-06)"""
    c = _case(rows, hidden)
    want_x, want_h = _want(c, full)
    d = _Dev(c)
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2) if full else {}
    xo, h = d.one(d.x, h_dtype=torch.float32, resid_acc=racc, **kw)
    xl, hl = d.library(d.x, full)
    torch.cuda.synchronize()
    e, el = (_err(xo, want_x), _err(h, want_h)), (_err(xl, want_x), _err(hl, want_h))
    print(f"rows {rows} hidden {hidden} {'full' if full else 'bare'} {'acc' if racc else 'reload'}: max|err| vs fp64  "
          f"x_out: library {el[0]:.3e}, kernel {e[0]:.3e};  h: library {el[1]:.3e}, kernel {e[1]:.3e}")
    assert e[0] <= 1.5 * el[0]
    assert e[1] <= 1.5 * el[1]


@pytest.mark.gpu
@pytest.mark.parametrize("bias", [False, True], ids=["no-bias", "bias"])
@pytest.mark.parametrize("rows", (1, 65, 200))
def test_projection_epilogue_vs_fp64_beside_h_and_a_library_gemm(rows, bias):
    """proj_dim 576: max abs error against fp64 LN2(r) @ Wp^T (+ b), h_out bf16 + torch.mm / the epilogue, measured on MI355X:
        rows   1 no bias: 9.204e-03 / 9.204e-03
        rows   1    bias: 1.165e-02 / 8.330e-03
        rows  65 no bias: 1.412e-02 / 1.412e-02
        rows  65    bias: 1.779e-02 / 1.359e-02
        rows 200 no bias: 1.330e-02 / 1.330e-02
        rows 200    bias: 2.754e-02 / 1.491e-02
    (without a bias the two agree to the digits shown: the bf16 rounding of h dominates both)"""
    c = _case(rows, 1024, seed=7)
    want_x, want_h = _want(c, True)
    want_p = want_h @ c["wp"].double().t() + (c["bp"].double() if bias else 0.0)
    d = _Dev(c)
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2)
    xo, p = d.one(d.x, proj_w=d.proj(576), proj_b=d.bp if bias else None, **kw)
    xo2, h = d.one(d.x, h_dtype=torch.bfloat16, **kw)
    pl = torch.mm(h, d.wp_raw.t())
    if bias:
        pl = (pl.float() + d.bp).bfloat16()
    torch.cuda.synchronize()
    assert p.shape == (rows, 576) and p.dtype == torch.bfloat16 and torch.equal(xo, xo2)
    e, el = _err(p, want_p), _err(pl, want_p)
    print(f"rows {rows} proj 576 {'bias' if bias else 'no bias'}: max|err| vs fp64  h + library GEMM {el:.3e}, epilogue {e:.3e}")
    assert e <= 1.5 * el
    assert _err(xo, want_x) <= 1.5 * _err(d.library(d.x, True)[0], want_x)


@pytest.mark.gpu
def test_projection_epilogue_at_the_smallest_width():
    c = _case(200, 256, seed=8)
    want_h = _want(c, True)[1]
    d = _Dev(c)
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2)
    _, p = d.one(d.x, proj_w=d.proj(64), proj_b=d.bp[:64].contiguous(), **kw)
    _, h = d.one(d.x, h_dtype=torch.bfloat16, **kw)
    pl = (torch.mm(h, d.wp_raw[:64].t()).float() + d.bp[:64]).bfloat16()
    want_p = want_h @ c["wp"][:64].double().t() + c["bp"][:64].double()
    assert p.shape == (200, 64)
    assert _err(p, want_p) <= 1.5 * _err(pl, want_p)
    # the epilogue's bands are the wide projection's: the same 64 columns, the same bits
    _, p576 = d.one(d.x, proj_w=d.proj(576), proj_b=d.bp, **kw)
    assert torch.equal(p576[:, :64], p)


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", HIDDEN)
def test_an_alpha_that_is_no_power_of_two_takes_the_reload_path(hidden):
    c = _case(200, hidden, seed=1)
    want_x, want_h = _want(c, True, alpha=0.3)
    d = _Dev(c)
    kw = dict(alpha=0.3, addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2, h_dtype=torch.float32)
    xo, h = d.one(d.x, **kw)
    xo_r, h_r = d.one(d.x, resid_acc=False, **kw)
    xl, hl = d.library(d.x, True, alpha=0.3)
    torch.cuda.synchronize()
    assert _err(xo, want_x) <= 1.5 * _err(xl, want_x) and _err(h, want_h) <= 1.5 * _err(hl, want_h)
    assert torch.equal(xo, xo_r) and torch.equal(h, h_r)             # the same path: the same bits


@pytest.mark.gpu
@pytest.mark.parametrize("racc", [True, False], ids=["accumulators", "reload"])
@pytest.mark.parametrize("hidden", HIDDEN)
def test_token_outputs_do_not_depend_on_position_or_row_count(hidden, racc):
    d = _Dev(_case(200, hidden, seed=3))
    kw = dict(add_scale=0.7, norm1=d.n1, norm2=d.n2, h_dtype=torch.float32, resid_acc=racc)
    xo, h = d.one(d.x, addend=d.add, **kw)
    _, p = d.one(d.x, addend=d.add, proj_w=d.proj(576), **{k: v for k, v in kw.items() if k != "h_dtype"})
    perm = torch.randperm(200, generator=torch.Generator().manual_seed(5)).to(DEV)
    xo_p, h_p = d.one(d.x[perm].contiguous(), addend=d.add[perm].contiguous(), **kw)
    assert torch.equal(xo_p, xo[perm]) and torch.equal(h_p, h[perm])
    for n in (1, 63, 65):                                            # another launch size, another tile position for most rows
        xo_n, h_n = d.one(d.x[200 - n:].contiguous(), addend=d.add[200 - n:].contiguous(), **kw)
        assert torch.equal(xo_n, xo[200 - n:]) and torch.equal(h_n, h[200 - n:])
        _, p_n = d.one(d.x[200 - n:].contiguous(), addend=d.add[200 - n:].contiguous(), proj_w=d.proj(576),
                       **{k: v for k, v in kw.items() if k != "h_dtype"})
        assert torch.equal(p_n, p[200 - n:])


@pytest.mark.gpu
def test_x_out_may_alias_x():
    d = _Dev(_case(200, 1024, seed=4))
    kw = dict(addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2)
    for racc in (True, False):
        xo, h = d.one(d.x, resid_acc=racc, **kw)
        x2 = d.x.clone()
        xo2, h2 = d.one(x2, x_out=x2, resid_acc=racc, **kw)
        assert xo2.data_ptr() == x2.data_ptr() and torch.equal(xo2, xo) and torch.equal(h2, h)


@pytest.mark.gpu
def test_repeats_give_the_same_bits_at_32000_rows():
    g_ = torch.Generator(device=DEV).manual_seed(3)
    d = _Dev(_case(1, 1024, seed=5))
    x = torch.randn(32000, D, device=DEV, generator=g_) * 2.0 + 0.5
    add = torch.randn(32000, D, device=DEV, generator=g_).bfloat16()
    kw = dict(add_scale=0.7, norm1=d.n1, norm2=d.n2)
    first = d.one(x, addend=add, **kw)
    for _ in range(5):
        again = d.one(x, addend=add, **kw)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1])
    tail = d.one(x[31936:].contiguous(), addend=add[31936:].contiguous(), **kw)
    assert torch.equal(tail[0], first[0][31936:]) and torch.equal(tail[1], first[1][31936:])


@pytest.mark.gpu
@pytest.mark.parametrize("racc", [True, False], ids=["accumulators", "reload"])
def test_layernorm_statistics_count_the_real_features_only(racc):
    """Inputs offset by +50: a mean over 160 columns would be 45 instead of 50, far outside any rounding.  The offset costs the fp32
    rows log2(50 / 0.5) ~ 7 bits against the other cases, on both routes alike; the bound stays the library route's error."""
    c = _case(200, 1024, seed=6, offset=50.0)
    want_x, want_h = _want(c, True)
    d = _Dev(c)
    xo, h = d.one(d.x, addend=d.add, add_scale=0.7, norm1=d.n1, norm2=d.n2, h_dtype=torch.float32, resid_acc=racc)
    xl, hl = d.library(d.x, True)
    torch.cuda.synchronize()
    e, el = (_err(xo, want_x), _err(h, want_h)), (_err(xl, want_x), _err(hl, want_h))
    print(f"offset 50 {'acc' if racc else 'reload'}: max|err| vs fp64  x_out: library {el[0]:.3e}, kernel {e[0]:.3e};  "
          f"h: library {el[1]:.3e}, kernel {e[1]:.3e}")
    assert e[0] <= 1.5 * el[0] and e[1] <= 1.5 * el[1]
    # bare: r = x + 0.5 ffn(LN(x)) around 50; a wrong pre-LN mean shows in the feed-forward term
    want_b = _want(c, False)[0]
    assert _err(d.one(d.x, resid_acc=racc)[0], want_b) <= 1.5 * _err(d.library(d.x, False)[0], want_b)


@pytest.mark.gpu
def test_packed_weight_zero_padding():
    """The image of a (1024, 144) matrix padded to 160 columns is the image of the explicitly zero-padded matrix; repack_ rewrites it
    in place; an unpadded image is what it was.  (On the GPU: the image is made by cm_ffn_pack_weights.)"""
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(1)
    w = torch.randn(1024, 144, generator=g).bfloat16().to(DEV)
    pw = ops.PackedWeight(w, pad=(1024, 160))
    explicit = ops.PackedWeight(F.pad(w, (0, 16)))
    assert pw.shape == (1024, 144) and pw.padded == (1024, 160) and explicit.padded == explicit.shape == (1024, 160)
    assert pw.data.numel() == 1024 * 160 and torch.equal(pw.data, explicit.data)
    wt = w.t().contiguous()                                          # rows padded: W2's image
    assert torch.equal(ops.PackedWeight(wt, pad=(160, 1024)).data, ops.PackedWeight(F.pad(wt, (0, 0, 0, 16))).data)
    ptr = pw.data.data_ptr()
    w2 = torch.randn(1024, 144, generator=g).bfloat16().to(DEV)
    pw.repack_(w2)
    assert pw.data.data_ptr() == ptr and torch.equal(pw.data, ops.PackedWeight(F.pad(w2, (0, 16))).data)
    with pytest.raises(RuntimeError):
        ops.PackedWeight(w, pad=(1024, 128))
    # the image of one fragment tile: lane L = 16 lq + l15 owns row l15, columns 8 lq .. 8 lq + 7
    w256 = torch.randn(512, 256, generator=g).bfloat16().to(DEV)
    img = ops.PackedWeight(w256).data.view(512 // 16, 256 // 32, 4, 16, 8)
    assert torch.equal(img.permute(0, 3, 1, 2, 4).reshape(512, 256), w256)


# ---- argument refusal: no GPU, no launch -------------------------------------------------------------------------------
def test_entry_point_refuses_bad_arguments_without_a_launch():
    import mamba_asr_amd._native as N
    lib = N.lib()
    fields = dict(N.FfnArgs._fields_)

    def args(**over):
        a = N.FfnArgs()
        a.rows, a.dim, a.hidden, a.alpha, a.pre_eps = 64, 144, 1024, 0.5, 1e-5
        # distinct, 16-byte aligned; never dereferenced: every case below is refused before a launch
        for i, k in enumerate(("x", "pre_g", "pre_b", "w1", "b1", "w2", "b2", "x_out")):
            setattr(a, k, C.cast(C.c_void_p(0x10000000 * (i + 1)), fields[k]))
        for k, v in over.items():
            if k in ("proj_w", "proj_out", "pre_out", "h_out"):
                v = C.cast(C.c_void_p(v), fields[k])
            setattr(a, k, v)
        return a

    proj = dict(proj_w=0xa0000000, proj_out=0xb0000000)
    for bad in (dict(dim=128), dict(dim=160), dict(layout=1), dict(pre_out=0xc0000000)):
        assert lib.cm_ffn_fused(C.byref(args(**bad))) == -2, bad                         # CM_EUNSUPPORTED
    assert b"ffn_fused" in lib.cm_last_error()
    for bad in (dict(proj_dim=100, **proj), dict(proj_dim=0, **proj), dict(dim=256, proj_dim=576, **proj)):
        assert lib.cm_ffn_fused(C.byref(args(**bad))) == -1, bad                         # CM_EINVAL
    assert lib.cm_ffn_fused(C.byref(args(hidden=1000))) == -2


def test_python_layer_accepts_144_only_while_the_16x16x32_kernel_is_selected(monkeypatch):
    from mamba_asr_amd import ops
    assert ops.ffn_supported(256, 1024, torch.bfloat16)
    assert ops.ffn_supported(144, 1024, torch.bfloat16) == (ops.FFN_LAYOUT == 16)
    monkeypatch.setattr(ops, "FFN_LAYOUT", 32)
    assert not ops.ffn_supported(144, 1024, torch.bfloat16) and ops.ffn_supported(256, 1024, torch.bfloat16)
    monkeypatch.setattr(ops, "FFN_LAYOUT", 16)
    assert ops.ffn_supported(144, 1024, torch.bfloat16) and not ops.ffn_supported(144, 1000, torch.bfloat16)
    assert not ops.ffn_supported(128, 1024, torch.bfloat16) and not ops.ffn_supported(144, 1024, torch.float32)
