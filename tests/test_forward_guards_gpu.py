"""Guard bands around the fused forward kernels (tests/guard_bands.py; tests/test_guard_bands_cpu.py shows the checker catches what it
is for).  Every case is two launches: (a) on ordinary tensors, (b) with every input a view of a NaN-filled buffer and every output a
view of a sentinel-filled one.  Then: (b)'s outputs have (a)'s bits, nothing outside an output view is written, every output is finite,
and (a)'s outputs are far from the sentinel.  Where the shape is new to the suite, (a) is also held to the fp64 reference with the
tolerance of the kernel's existing test (restated and named at each use).

Guards: 64 rows around the tensors of the row kernels (their workgroup tile), 32 time steps behind every utterance of the time-tiled
ones plus one whole guard utterance in front of and behind the batch, 8 columns left and 16 right of column slices.  An output that
aliases an input (x_out = x, the residual x of cm_gemm_bf16's epilogue 2) lies in a sentinel buffer: a read of its surroundings
brings -65536 into the result, which then has other bits than (a)'s.  Packed weight images are opaque to the tests and stay plain.
Halves of a wider buffer that the kernel under test has no business reading ([x | z]: z for the convs, x for the scan) are NaN in (b).
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import conmamba_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
RT, TT = G.ROW_TILE, G.TIME_TILE
COLS = dict(rows=TT, left=G.LEFT, right=G.RIGHT)
NAN = float("nan")


def close(a, b, rtol, atol):
    torch.testing.assert_close(a.detach().double().cpu(), b.detach().double().cpu(), rtol=rtol, atol=atol)


def dev(t):
    return None if t is None else t.to(DEV)


def Launch(guard):
    """guard_bands.Launch on the GPU: plain (guard=False) or poisoned inputs / guarded outputs (guard=True)."""
    return G.Launch(guard, DEV)


def two_step(run):
    """run(Launch) launches the kernel on the Launch's tensors.  -> the plain launch's outputs by name."""
    return G.two_step(run, DEV)


# ------------------------------------------------------------------------------------------------------------------------
# cm_ffn_fused
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ffn_case(d, hidden, pdim, layout):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(d + hidden + pdim)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    ln = lambda: (dev(1.0 + 0.1 * rn(d)), dev(0.1 * rn(d)))
    kp = 160 if d == 144 else d                                              # d_model 144: images padded to whole 32-column tiles
    pw = lambda t, pad: ops.PackedWeight(dev(t.bfloat16()), layout, pad=pad)
    return dict(d=d, hidden=hidden, pdim=pdim, x=dev(rn(129, d, scale=2.0) + 0.5), addend=dev(rn(129, d).bfloat16()),
                w1=pw(rn(hidden, d, scale=d ** -0.5), (hidden, kp)), b1=dev(rn(hidden, scale=0.1)),
                w2=pw(rn(d, hidden, scale=hidden ** -0.5), (kp, hidden)), b2=dev(rn(d, scale=0.1)), pre=ln(), n1=ln(), n2=ln(),
                wp=pw(rn(pdim, d, scale=1 / 16), (pdim, kp)), bp=dev(rn(pdim, scale=0.1)))


def _ffn_run(c, rows, form, tokens, alias, racc, train=None):
    from mamba_asr_amd import ops
    d = c["d"]

    def run(L):
        norm = lambda k: (L.vec(c[k][0]), L.vec(c[k][1]), 1e-5)
        x = c["x"][:rows]
        if alias:
            xin, xo = L.out("x_out", (rows, d), F32, fill=x), None
        else:
            xin, xo = L.rows(x), L.out("x_out", (rows, d), F32)
        kw = dict(alpha=0.5, x_out=xo, resid_acc=racc)
        if train is not None:
            outs = (L.out("pre", (rows, c["hidden"]), BF16), L.out("xn", (rows, d), BF16), L.out("stats", (2, rows), F32))
            kw.update(train=train, train_out=outs)
        elif form == "proj":
            kw.update(norm2=norm("n2"), proj_w=c["wp"], proj_b=L.vec(c["bp"]), proj_out=L.out("proj_out", (rows, c["pdim"]), BF16), tokens=tokens)
        else:
            hdt = F32 if form == "bare_f32" else BF16
            kw.update(h_dtype=hdt, h_out=L.out("h", (rows, d), hdt), tokens=tokens)
            if form == "full":
                kw.update(addend=L.rows(c["addend"][:rows]), add_scale=0.7, norm1=norm("n1"), norm2=norm("n2"))
        ret = ops.ffn_fused(xin, norm("pre"), c["w1"], L.vec(c["b1"]), c["w2"], L.vec(c["b2"]), **kw)
        assert ret[0].data_ptr() == L.outs["x_out"].data_ptr()
    return run


@pytest.mark.parametrize("form", ["bare_bf16", "bare_f32", "full", "proj"])
@pytest.mark.parametrize("rows", [1, 31, 33, 63, 65, 129])
@pytest.mark.parametrize("layout,tokens", [(16, None), (32, 64), (32, 32)])
def test_ffn_fused_d256(layout, tokens, rows, form):
    """Inference forward, D 256, hidden 256: both weight layouts, 64- and 32-token workgroups; h in bf16 / fp32, addend + norm1 + norm2,
    the projection epilogue (P = 256) into a guarded proj_out; x_out aliasing x and apart; the residual in accumulators and reloaded."""
    c = _ffn_case(256, 256, 256, layout)
    for alias in (False, True):
        for racc in (True, False):
            two_step(_ffn_run(c, rows, form, tokens, alias, racc))


@pytest.mark.parametrize("form", ["bare_bf16", "full", "proj"])
@pytest.mark.parametrize("rows", [1, 63, 65])
def test_ffn_fused_d144(rows, form):
    """D 144 (csrc/fused_d144.hip), hidden 256: the bare and the full form, the projection with P = 64."""
    c = _ffn_case(144, 256, 64, 16)
    for alias in (False, True):
        for racc in (True, False):
            two_step(_ffn_run(c, rows, form, None, alias, racc))


@pytest.mark.parametrize("p", [(0.0, 0.0), (0.1, 0.2)])
@pytest.mark.parametrize("rows", [1, 63, 65, 129])
@pytest.mark.parametrize("hidden", [256, 1024])
def test_ffn_fused_training_forward(hidden, rows, p):
    """The training forward's stored outputs: pre goes out through raw buffer stores whose descriptor range drops the rows of a ragged
    last tile, xn / stats / x_out behind row tests.  stats is (2, rows): a mean stored past ``rows`` would land in the 1/std row, inside
    the view, so the statistics are also held to fp64 (test_ffn_fused_training_forward in tests/test_scan_rows_bwd.py: mean rtol 1e-5 /
    atol 1e-5, 1/std rtol 1e-4 / atol 1e-5)."""
    c = _ffn_case(256, hidden, 256, 16)
    for alias in (False, True):
        outs = two_step(_ffn_run(c, rows, "train", None, alias, True, train=(p[0], p[1], 1234567 + rows, 7654321 + hidden)))
        x = c["x"][:rows].double()
        close(outs["stats"][0], x.mean(1), 1e-5, 1e-5)
        close(outs["stats"][1], (x.var(1, unbiased=False) + 1e-5).rsqrt(), 1e-4, 1e-5)


# ------------------------------------------------------------------------------------------------------------------------
# cm_ln_pw_glu / cm_ln_pw_glu_mix
# ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lnpw_case(d, k):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(d + k)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    c = dict(d=d, x=dev(rn(65, d)), y=dev(rn(65, d, scale=0.5).bfloat16()), ln=(dev(1.0 + 0.1 * rn(d)), dev(0.1 * rn(d))),
             w=ops.PackedWeight(dev(rn(2 * d, d, scale=1 / 16).bfloat16()), pad=(2 * d, 160 if d == 144 else d)), bias=dev(rn(2 * d, scale=0.1)))
    if k:
        c.update(ycat=dev(rn(65, k).bfloat16()), wo=ops.PackedWeight(dev(rn(256, k, scale=0.05).bfloat16())))
    return c


@pytest.mark.parametrize("rows", [1, 15, 17, 63, 65])
@pytest.mark.parametrize("d,k", [(256, 0), (256, 128), (256, 512), (144, 0)])
def test_ln_pw_glu(d, k, rows):
    """x_out and out behind their row tests, with y (k = 0) or with ycat @ out_w^T formed in the kernel (K = 128, 512; D 256 only);
    x, y and ycat inside NaN rows; x_out apart from x and aliasing it."""
    from mamba_asr_amd import ops
    c = _lnpw_case(d, k)

    def make(alias):
        def run(L):
            x = c["x"][:rows]
            if alias:
                xin, xo = L.out("x_out", (rows, d), F32, fill=x), None
            else:
                xin, xo = L.rows(x), L.out("x_out", (rows, d), F32)
            kw = dict(ycat=L.rows(c["ycat"][:rows]), out_w=c["wo"]) if k else {}
            y = None if k else L.rows(c["y"][:rows])
            ret = ops.ln_pw_glu(xin, y, 1.0, (L.vec(c["ln"][0]), L.vec(c["ln"][1]), 1e-5), c["w"], L.vec(c["bias"]), x_out=xo,
                                out=L.out("out", (rows, d), BF16), **kw)
            assert ret.data_ptr() == L.outs["out"].data_ptr()
        return run
    for alias in (False, True):
        two_step(make(alias))


# ------------------------------------------------------------------------------------------------------------------------
# cm_conv_xproj / cm_conv_xproj_uni
# ------------------------------------------------------------------------------------------------------------------------
CONV_TOL = (1.6e-2, 1e-2)          # test_conv_xproj (tests/test_hip_ops.py): the conv against O.causal_conv1d
XDBL_TOL = (1.6e-2, 2e-2)          # test_conv_xproj: the x_dbl rows against the kernel's own u through an fp32 matmul


@functools.lru_cache(maxsize=None)
def _xproj_case(b, l, e, rw):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(1000 * l + e + rw + b)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    c = dict(xz=dev(rn(b, l, 2 * e).bfloat16()), hist=dev(rn(b, 3, e).bfloat16()), w=[dev(rn(e, 4, scale=0.5)) for _ in range(2)],
             bias=[dev(rn(e, scale=0.1)) for _ in range(2)], wx=[dev(rn(rw, e, scale=0.1).bfloat16()) for _ in range(2)])
    c["wxp"] = [ops.PackedWeight(w, pad=(rw, (e + 31) // 32 * 32)) for w in c["wx"]]     # dim 72: an image exists, the entry point refuses
    return c


def _refused(run, match):
    """A launch the entry point must refuse (a missing kernel is an error, not another route): RuntimeError, and no output touched."""
    L = Launch(True)
    with pytest.raises(RuntimeError, match=match):
        run(L)
    torch.cuda.synchronize()
    for name, (buf, view, outside) in L.g.items.items():
        G.assert_untouched(buf, outside, name)
        assert bool((view == G.SENTINEL).all()), f"{name}: written by a refused launch"


def _conv_ref(x, w, bias, reverse=False, hist=None):
    """fp64 causal conv + SiLU of (b, l, e) rows (reverse: anti-causal, the backward direction); hist: the three rows in front."""
    xt = x.double().cpu().transpose(1, 2)
    n = 0
    if hist is not None:
        xt, n = torch.cat([hist.double().cpu().transpose(1, 2), xt], dim=2), 3
    if reverse:
        xt = xt.flip(-1)
    y = O.causal_conv1d(xt, w.double().cpu(), bias.double().cpu(), True, work_dtype=torch.float64)
    return (y.flip(-1) if reverse else y)[:, :, n:].transpose(1, 2)


def _xproj_bi(b, l, e, rw, variant=0):
    from mamba_asr_amd import ops
    c = _xproj_case(b, l, e, rw)

    def run(L):
        xz = L.cols(c["xz"], dead=(e, 2 * e))
        ucat = L.out("ucat", (b, l, 2 * e), BF16, **COLS)
        xdbl = L.out("xdbl", (b, l, 2 * rw), BF16, **COLS)
        ret = ops.conv_xproj(xz[:, :, :e], L.vec(c["w"][0]), L.vec(c["bias"][0]), L.vec(c["w"][1]), L.vec(c["bias"][1]), c["wxp"][0], c["wxp"][1],
                             out_f=ucat[:, :, :e], out_b=ucat[:, :, e:], xdbl=xdbl, variant=variant)
        assert ret.data_ptr() == xdbl.data_ptr()
    if e % 32:
        return _refused(run, "multiple of 32")
    outs = two_step(run)
    x = c["xz"][:, :, :e]
    for i in range(2):
        u = outs["ucat"][:, :, e * i:e * (i + 1)]
        close(u, _conv_ref(x, c["w"][i], c["bias"][i], reverse=i == 1), *CONV_TOL)
        close(outs["xdbl"][:, :, rw * i:rw * (i + 1)], u.double() @ c["wx"][i].double().t(), *XDBL_TOL)
    return outs


@pytest.mark.parametrize("l", [1, 2, 3, 15, 16, 17, 33])
@pytest.mark.parametrize("e", [64, 72, 96])
@pytest.mark.parametrize("rw", [48, 64])
def test_conv_xproj(rw, e, l):
    """x a column slice of a NaN-surrounded [x | z] whose z half is NaN, out_f / out_b the halves of one guarded ucat, xdbl guarded;
    sequences shorter than the window, on and next to the 16-step tile.  The kernel takes dims that are multiples of 32 (its k-tiles):
    dim 72 must be refused with every output untouched; dim 96 is the smallest width that is no multiple of 64."""
    _xproj_bi(2, l, e, rw)


@pytest.mark.parametrize("rw", [48, 64])
def test_conv_xproj_32_step_tiles(rw):
    """batch x ceil(seqlen / 32) >= 512 picks the 32-step tiles (ragged second tile of one step); the 16-step tiles give the same bits."""
    wide, narrow = _xproj_bi(512, 33, 64, rw), _xproj_bi(512, 33, 64, rw, variant=1)
    assert torch.equal(wide["ucat"], narrow["ucat"]) and torch.equal(wide["xdbl"], narrow["xdbl"])


def _xproj_uni(b, l, e, rw, with_hist, variant=0):
    from mamba_asr_amd import ops
    c = _xproj_case(b, l, e, rw)

    def run(L):
        xz = L.cols(c["xz"], dead=(e, 2 * e))
        hist = L.flat(c["hist"], 3) if with_hist else None
        ret = ops.conv_xproj_uni(xz[:, :, :e], L.vec(c["w"][0]), L.vec(c["bias"][0]), c["wxp"][0], out=L.out("u", (b, l, e), BF16, **COLS),
                                 xdbl=L.out("xdbl", (b, l, rw), BF16, **COLS), x_hist=hist,
                                 x_hist_out=L.out("x_hist_out", (b, 3, e), BF16, rows=RT, contiguous=True), variant=variant)
        assert ret.data_ptr() == L.outs["xdbl"].data_ptr()
    if e % 32:
        return _refused(run, "multiple of 32")
    outs = two_step(run)
    x = c["xz"][:, :, :e]
    hist = c["hist"] if with_hist else torch.zeros_like(c["hist"])
    close(outs["u"], _conv_ref(x, c["w"][0], c["bias"][0], hist=hist), *CONV_TOL)
    close(outs["xdbl"], outs["u"].double() @ c["wx"][0].double().t(), *XDBL_TOL)
    assert torch.equal(outs["x_hist_out"], torch.cat([hist, x], dim=1)[:, -3:]), "x_hist_out: the last three rows of [x_hist | x]"
    return outs


@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("l", [1, 2, 3, 15, 16, 17, 33])
@pytest.mark.parametrize("e", [64, 72, 96])
@pytest.mark.parametrize("rw", [48, 64])
def test_conv_xproj_uni(rw, e, l, with_hist):
    """The causal form; with a NaN-surrounded x_hist and a guarded x_hist_out (seqlen 1 and 2: shorter than the history, so x_hist_out
    keeps rows of x_hist)."""
    _xproj_uni(2, l, e, rw, with_hist)


def test_conv_xproj_uni_32_step_tiles():
    wide, narrow = _xproj_uni(512, 33, 64, 48, True), _xproj_uni(512, 33, 64, 48, True, variant=1)
    for k in wide:
        assert torch.equal(wide[k], narrow[k]), k


# ------------------------------------------------------------------------------------------------------------------------
# cm_scan_cl_fwd
# ------------------------------------------------------------------------------------------------------------------------
SCAN_TOL = {F32: (2e-4, 5e-5), BF16: (1.6e-2, 1e-2)}       # test_scan_rows_two_directions / test_scan_channels_last_two_directions (tests/test_hip_ops.py)


@functools.lru_cache(maxsize=None)
def _scan_case(b, l, e, rank, dtype):
    """test_scan_rows_two_directions' recipe and reference: x_dbl rows [dt P | B | C], both directions, the fp64 oracle on the
    dtype-rounded inputs and the dtype-rounded dt_proj weight."""
    from mamba_asr_amd import ops
    P = 16 if rank <= 16 else 32
    RW = P + 32
    gen = torch.Generator().manual_seed(l * 11 + e + rank)
    xz = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    ucat = torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    xcat = torch.randn(b, l, 2 * RW, generator=gen)
    tr = lambda t: t.double().transpose(1, 2)
    par, refs = [], []
    for i, rev in enumerate((False, True)):
        xcat[:, :, RW * i + rank:RW * i + P] = 0.0
        A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
        Wdt = torch.randn(e, rank, generator=gen) * 0.3
        D, bias = torch.randn(e, generator=gen), torch.randn(e, generator=gen) - 1
        par.append(dict(A=dev(A), D=dev(D), bias=dev(bias), W=ops.pad_dt_weight(dev(Wdt)), rev=rev, host=(A, Wdt, D, bias)))
    xq = xcat.to(dtype)
    for i, p in enumerate(par):
        A, Wdt, D, bias = p["host"]
        xd = xq[:, :, RW * i:RW * (i + 1)].double()
        delta = torch.einsum("er,blr->bel", Wdt.to(dtype).double(), xd[:, :, :rank])
        f = (lambda t: t.flip(-1)) if p["rev"] else (lambda t: t)
        ref = O.selective_scan(f(tr(ucat[:, :, e * i:e * (i + 1)])), f(delta), A, f(xd[:, :, P:P + 16].transpose(1, 2)), f(xd[:, :, P + 16:].transpose(1, 2)),
                               D, f(tr(xz[:, :, e:])), bias, True, work_dtype=torch.float64)
        refs.append(f(ref).transpose(1, 2))
    h0 = [dev(torch.randn(b, e, 16, generator=gen)) for _ in range(2)]
    return dict(b=b, l=l, e=e, RW=RW, dtype=dtype, xz=dev(xz), ucat=dev(ucat), xcat=dev(xq), par=par, ref=torch.cat(refs, dim=2), h0=h0)


def _scan_rows(c, split, chunks=1, carry=False, train=False):
    from mamba_asr_amd import ops
    b, l, e, RW, dtype = c["b"], c["l"], c["e"], c["RW"], c["dtype"]

    def run(L):
        xz, ucat, xcat = L.cols(c["xz"], dead=(0, e)), L.cols(c["ucat"]), L.cols(c["xcat"])
        ycat = L.out("ycat", (b, l, 2 * e), dtype, **COLS)
        pcat = L.out("pcat", (b, l, 2 * e), dtype, **COLS) if train else None
        dirs = []
        for i, p in enumerate(c["par"]):
            sl = slice(e * i, e * (i + 1))
            dd = dict(u=ucat[:, :, sl], xdbl=xcat[:, :, RW * i:RW * (i + 1)], A=L.vec(p["A"]), D=L.vec(p["D"]), delta_bias=L.vec(p["bias"]),
                      dt_weight=L.vec(p["W"]), out=ycat[:, :, sl], reverse=p["rev"])
            if carry:                                       # (batch, dim, 16) fp32: one utterance's plane of guard on each side
                dd.update(h0=L.flat(c["h0"][i], e), h_last=L.out(f"h_last{i}", (b, e, 16), F32, rows=e, contiguous=True),
                          decay=L.out(f"decay{i}", (b, e, 16), F32, rows=e, contiguous=True))
            if train:                                       # ckpt: two (dim, 16) planes of guard; zero-filled, a ragged last block need not fill its planes
                dd.update(ypre=pcat[:, :, sl], ckpt=L.out(f"ckpt{i}", ops.scan_ckpt_shape(b, l, e), F32, fill=0.0, rows=2 * e))
            dirs.append(dd)
        ret = ops.scan_cl_fwd(dirs, z=xz[:, :, e:], delta_softplus=True, split=split, time_chunks=chunks)
        assert [r.data_ptr() for r in ret] == [d_["out"].data_ptr() for d_ in dirs]
    return two_step(run)


@pytest.mark.parametrize("l", [1, 7, 8, 9, 15, 16, 17, 33])
@pytest.mark.parametrize("e", [64, 72])
@pytest.mark.parametrize("dtype,rank,split", [(F32, 9, 4), (F32, 9, 8), (BF16, 9, 4), (BF16, 9, 8), (BF16, 32, 4)])
def test_scan_rows(dtype, rank, split, e, l):
    """xdbl mode, both directions: the outputs are the halves of one guarded ycat, z the second half of a NaN-surrounded [x | z] whose x
    half is NaN, u the halves of a NaN-surrounded ucat, xdbl the halves of a NaN-surrounded xcat.  (The 2-states-per-lane kernel,
    split 8, is built for dt_rank <= 16.)"""
    c = _scan_case(2, l, e, rank, dtype)
    outs = _scan_rows(c, split)
    close(outs["ycat"], c["ref"], *SCAN_TOL[dtype])


@pytest.mark.parametrize("dtype,rank", [(F32, 9), (BF16, 9), (BF16, 32)])
@pytest.mark.parametrize("e", [64, 72])
def test_scan_rows_time_chunks_and_carry(dtype, rank, e):
    """time_chunks 3 at seqlen 50 (a ragged last chunk), then the same with a NaN-surrounded h0 and guarded h_last / decay."""
    c = _scan_case(2, 50, e, rank, dtype)
    outs = _scan_rows(c, 4, chunks=3)
    close(outs["ycat"], c["ref"], *SCAN_TOL[dtype])
    _scan_rows(c, 4, chunks=3, carry=True)


@pytest.mark.parametrize("l", [17, 33])
@pytest.mark.parametrize("dtype,rank", [(F32, 9), (BF16, 9), (BF16, 32)])
@pytest.mark.parametrize("e", [64, 72])
def test_scan_rows_training_outputs(dtype, rank, e, l):
    """The checkpoints and ypre the training forward stores for cm_scan_cl_bwd, guarded."""
    c = _scan_case(2, l, e, rank, dtype)
    outs = _scan_rows(c, 4, train=True)
    close(outs["ycat"], c["ref"], *SCAN_TOL[dtype])


def _bc(L, t):
    """Channel-mode B / C (16, batch, seqlen): read 16 steps past their end by contract (ops.alloc_bc) -- that tail stays finite (0),
    NaN only in front and beyond it."""
    if not L.guard:
        from mamba_asr_amd import ops
        v = ops.alloc_bc(*t.shape, DEV)
        v.copy_(t)
        return v
    n, pad = t.numel(), 64
    flat = torch.full((pad + n + 16 + pad,), NAN, dtype=F32, device=DEV)
    flat[pad + n:pad + n + 16] = 0.0
    v = flat[pad:pad + n].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("split", [4, 16])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_scan_channel_mode(dtype, split):
    """Channel mode (delta given) at (2, 17, 70): test_scan_channels_last_two_directions' recipe; u / delta / z / out column slices at
    widths that keep 4-byte alignment only."""
    from mamba_asr_amd import ops
    b, l, e = 2, 17, 70
    gen = torch.Generator().manual_seed(l * 7 + e)
    xz, ucat = torch.randn(b, l, 2 * e, generator=gen).to(dtype), torch.randn(b, l, 2 * e, generator=gen).to(dtype)
    dcat = (torch.randn(b, l, 2 * e, generator=gen) * 0.5).to(dtype)
    tr = lambda t: t.double().transpose(1, 2)
    par, refs = [], []
    for i, rev in enumerate((False, True)):
        sl = slice(e * i, e * (i + 1))
        A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
        Bm, Cm = torch.randn(16, b, l, generator=gen), torch.randn(16, b, l, generator=gen)
        D, bias = torch.randn(e, generator=gen), torch.randn(e, generator=gen) - 1
        f = (lambda t: t.flip(-1)) if rev else (lambda t: t)
        ref = O.selective_scan(f(tr(ucat[:, :, sl])), f(tr(dcat[:, :, sl])), A, f(Bm.permute(1, 0, 2)), f(Cm.permute(1, 0, 2)), D, f(tr(xz[:, :, e:])),
                               bias, True, work_dtype=torch.float64)
        refs.append(f(ref).transpose(1, 2))
        par.append(dict(A=dev(A), B=dev(Bm), C=dev(Cm), D=dev(D), bias=dev(bias), rev=rev))
    gxz, gu, gd = dev(xz), dev(ucat), dev(dcat)

    def run(L):
        vxz, vu, vd = L.cols(gxz, dead=(0, e), align=4), L.cols(gu, align=4), L.cols(gd, align=4)
        ycat = L.out("ycat", (b, l, 2 * e), dtype, align=4, **COLS)
        dirs = [dict(u=vu[:, :, e * i:e * (i + 1)], delta=vd[:, :, e * i:e * (i + 1)], A=L.vec(p["A"]), B=_bc(L, p["B"]), C=_bc(L, p["C"]),
                     D=L.vec(p["D"]), delta_bias=L.vec(p["bias"]), out=ycat[:, :, e * i:e * (i + 1)], reverse=p["rev"]) for i, p in enumerate(par)]
        ops.scan_cl_fwd(dirs, z=vxz[:, :, e:], delta_softplus=True, split=split)
    outs = two_step(run)
    close(outs["ycat"], torch.cat(refs, dim=2), *SCAN_TOL[dtype])


# ------------------------------------------------------------------------------------------------------------------------
# cm_glu_dwconv_ln_gelu / cm_glu_dwconv_ln_gelu_causal
# ------------------------------------------------------------------------------------------------------------------------
# bf16: test_dwconv_rows_kernel (tests/test_hip_modules.py) rtol 1.6e-2 / atol 1e-2; the closing Linear against the kernel's own bf16
# activations through a matmul: rtol 8e-3 / atol 4e-3 (same test).  fp32 (generic kernel only; test_dwconv_rows_kernel is bf16):
# test_channels_last_elementwise_ops' dim-80 check, rtol 1e-4 / atol 1e-4.
DW_TOL = {BF16: (1.6e-2, 1e-2), F32: (1e-4, 1e-4)}
DW_LIN_TOL = (8e-3, 4e-3)
KS = 31


def _ln64(t, g, b, eps):
    mu = t.mean(-1, keepdim=True)
    return (t - mu) / torch.sqrt(((t - mu) ** 2).mean(-1, keepdim=True) + eps) * g + b


@functools.lru_cache(maxsize=None)
def _dw_case(dtype, d, glu_done, lin, l, causal):
    from mamba_asr_amd import ops
    b = 3
    g = torch.Generator().manual_seed(31 * l + d + 2 * glu_done + lin)
    inp = torch.randn(b, l, d if glu_done else 2 * d, generator=g).to(dtype)
    hist = torch.randn(b, KS - 1, d, generator=g).to(dtype)
    w, bs = torch.randn(d, KS, generator=g) / 6, torch.randn(d, generator=g) * 0.1
    lg, lb = 1.0 + 0.1 * torch.randn(d, generator=g), 0.1 * torch.randn(d, generator=g)
    lw, lbias = (torch.randn(d, d, generator=g) / 16).bfloat16(), torch.randn(d, generator=g) * 0.1
    i64 = inp.double()
    gated = i64 if glu_done else (i64[..., :d] * torch.sigmoid(i64[..., d:])).to(dtype).double()     # the conv's operand is rounded to the I/O dtype
    seq = torch.cat([hist.double(), gated], dim=1) if causal else F.pad(gated, (0, 0, KS // 2, KS // 2))
    conv = bs.double() + sum(w.double()[:, k] * seq[:, k:k + l] for k in range(KS))
    act = _ln64(conv, lg.double(), lb.double(), 1e-5)
    act = 0.5 * act * (1.0 + torch.erf(act / 2 ** 0.5))
    c = dict(b=b, l=l, d=d, dtype=dtype, inp=dev(inp), hist=dev(hist), w=dev(w), wt=dev(w.t().contiguous()), bs=dev(bs), lg=dev(lg), lb=dev(lb),
             act=act, hist_ref=torch.cat([hist.double(), gated], dim=1)[:, -(KS - 1):], lw=dev(lw), lbias=dev(lbias))
    if lin:
        c["lwp"] = ops.PackedWeight(c["lw"])
    return c


def _dw_run(c, glu_done, lin, variant, causal, poison_neighbours=False):
    from mamba_asr_amd import ops
    b, l, d, dtype = c["b"], c["l"], c["d"], c["dtype"]

    def run(L):
        inp, hist = c["inp"], c["hist"]
        if poison_neighbours and L.guard:
            inp, hist = inp.clone(), hist.clone()
            inp[0], inp[2], hist[0], hist[2] = NAN, NAN, NAN, NAN
        kw = dict(lin_w=c["lwp"], lin_b=L.vec(c["lbias"])) if lin else {}
        if causal:
            kw.update(causal=True, hist=L.flat(hist, TT), hist_out=L.out("hist_out", (b, KS - 1, d), dtype, rows=TT, contiguous=True))
        ret = ops.glu_dwconv_ln_gelu(L.flat(inp, TT), L.vec(c["w"]), L.vec(c["bs"]), L.vec(c["lg"]), L.vec(c["lb"]), 1e-5, weight_t=L.vec(c["wt"]),
                                     glu_done=glu_done, variant=variant, out=L.out("out", (b, l, d), dtype, rows=TT, contiguous=True), **kw)
        assert ret.data_ptr() == L.outs["out"].data_ptr()
    return run


def _dw_check(c, glu_done, lin, variant, causal):
    """(1) all three utterances finite, NaN around the batch; (2) the middle utterance between two NaN utterances: the wrapper takes
    contiguous batches only, so there is no room for guard rows between utterances -- the neighbours themselves are the poison.  A
    halo that crosses an utterance end turns rows of the middle utterance into NaN."""
    outs = two_step(_dw_run(c, glu_done, lin, variant, causal))
    plain, guarded = Launch(False), Launch(True)
    _dw_run(c, glu_done, lin, variant, causal)(plain)
    _dw_run(c, glu_done, lin, variant, causal, poison_neighbours=True)(guarded)
    torch.cuda.synchronize()
    for name, (buf, view, outside) in guarded.g.items.items():
        G.assert_untouched(buf, outside, name)
        G.assert_finite(view[1], f"{name}[middle utterance]")
        G.assert_same_bits(view[1], plain.outs[name][1], f"{name}[middle utterance]")
    return outs


def _dw_reference_checks(c, outs, glu_done, lin, variant, causal):
    from mamba_asr_amd import ops
    dtype = c["dtype"]
    if lin:     # the Linear's operand is the bf16 activation tile the same launch stores without the epilogue (itself held to fp64)
        kw = dict(causal=True, hist=c["hist"]) if causal else {}
        act_k = ops.glu_dwconv_ln_gelu(c["inp"], c["w"], c["bs"], c["lg"], c["lb"], 1e-5, weight_t=c["wt"], glu_done=glu_done, variant=variant, **kw)
        close(act_k, c["act"], *DW_TOL[dtype])
        close(outs["out"], act_k.double() @ c["lw"].double().t() + c["lbias"].double(), *DW_LIN_TOL)
    else:
        close(outs["out"], c["act"], *DW_TOL[dtype])
    if causal:
        close(outs["hist_out"], c["hist_ref"], *DW_TOL[dtype])
        if glu_done:
            assert torch.equal(outs["hist_out"].double().cpu(), c["hist_ref"]), "hist_out: the last k - 1 rows of [hist | inp]"


DW_FORMS = [(BF16, 256, False, False, 0), (BF16, 256, True, False, 0), (BF16, 256, True, True, 0), (BF16, 256, False, False, 1), (BF16, 256, True, False, 1),
            (BF16, 512, False, False, 0), (BF16, 512, True, False, 0), (BF16, 512, True, False, 1),
            (BF16, 80, False, False, 0), (BF16, 80, True, False, 0), (F32, 80, False, False, 0), (F32, 80, True, False, 0)]
DW_IDS = [f"{'bf16' if t == BF16 else 'fp32'}_d{d}_{'gated' if gd else 'glu'}{'_lin' if ln_ else ''}{'_v1' if v else ''}" for t, d, gd, ln_, v in DW_FORMS]


@pytest.mark.parametrize("l", [1, 15, 16, 17, 31, 32, 33, 65])
@pytest.mark.parametrize("dtype,d,glu_done,lin,variant", DW_FORMS, ids=DW_IDS)
def test_glu_dwconv_ln_gelu(dtype, d, glu_done, lin, variant, l):
    """bf16 at dim 256 / 512: the 32-step row kernel, and variant 1 (the generic 16-step kernel) on the same input; dim 80: the generic
    kernel in both dtypes; pre-gated input and not; the closing Linear at dim 256.  Batch 3: the halo of the middle utterance ends at
    both neighbours."""
    c = _dw_case(dtype, d, glu_done, lin, l, False)
    outs = _dw_check(c, glu_done, lin, variant, False)
    _dw_reference_checks(c, outs, glu_done, lin, variant, False)


@pytest.mark.parametrize("l", [1, 5, 33])
@pytest.mark.parametrize("dtype,d,glu_done,lin,variant", DW_FORMS, ids=DW_IDS)
def test_glu_dwconv_ln_gelu_causal(dtype, d, glu_done, lin, variant, l):
    """The causal form with a NaN-surrounded hist and a guarded hist_out; seqlen 1 and 5 are shorter than the k - 1 = 30 history rows,
    so hist_out keeps rows of hist."""
    c = _dw_case(dtype, d, glu_done, lin, l, True)
    outs = _dw_check(c, glu_done, lin, variant, True)
    _dw_reference_checks(c, outs, glu_done, lin, variant, True)


# ------------------------------------------------------------------------------------------------------------------------
# the fallback routes: cm_add_layernorm, cm_conv_cl_fwd, cm_gemm_bf16
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", [BF16, F32])
@pytest.mark.parametrize("rows", [1, 65])
@pytest.mark.parametrize("d", [144, 256])
def test_add_layernorm(d, rows, odt):
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(d + rows)
    x, y = dev(torch.randn(rows, d, generator=g)), dev(torch.randn(rows, d, generator=g).bfloat16())
    par = [dev(torch.randn(d, generator=g)) for _ in range(4)]

    def make(alias):
        def run(L):
            if alias:
                xin = xo = L.out("x_out", (rows, d), F32, fill=x)
            else:
                xin, xo = L.rows(x), L.out("x_out", (rows, d), F32)
            ops.add_layernorm(xin, L.rows(y), 0.5, norm1=(L.vec(par[0]), L.vec(par[1]), 1e-5), norm2=(L.vec(par[2]), L.vec(par[3]), 1e-6), x_out=xo,
                              out_dtype=odt, out=L.out("out", (rows, d), odt))
        return run
    for alias in (False, True):
        two_step(make(alias))


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_cl_fwd(dtype):
    """(2, 17, 72), both directions: x the first half of a NaN-surrounded [x | z] whose z half is NaN, the outputs the halves of one
    guarded ucat."""
    from mamba_asr_amd import ops
    b, l, e = 2, 17, 72
    g = torch.Generator().manual_seed(1772)
    xz = dev(torch.randn(b, l, 2 * e, generator=g).to(dtype))
    w, bias = [dev(torch.randn(e, 4, generator=g) * 0.5) for _ in range(2)], [dev(torch.randn(e, generator=g) * 0.1) for _ in range(2)]

    def run(L):
        v = L.cols(xz, dead=(e, 2 * e))
        ucat = L.out("ucat", (b, l, 2 * e), dtype, **COLS)
        ops.conv_cl_fwd(v[:, :, :e], L.vec(w[0]), L.vec(bias[0]), L.vec(w[1]), L.vec(bias[1]), True, out_f=ucat[:, :, :e], out_b=ucat[:, :, e:])
    outs = two_step(run)
    # test_channels_last_elementwise_ops (tests/test_hip_modules.py): fp32 rtol 1e-4 / atol 1e-4, bf16 rtol 2e-2 / atol 2e-2
    tol = (1e-4, 1e-4) if dtype == F32 else (2e-2, 2e-2)
    for i in range(2):
        close(outs["ucat"][:, :, e * i:e * (i + 1)], _conv_ref(xz[:, :, :e], w[i], bias[i], reverse=i == 1), *tol)


@pytest.mark.parametrize("epilogue", [0, 1, 2])
@pytest.mark.parametrize("m,n,k", [(1, 256, 64), (65, 256, 256), (129, 512, 64)])
def test_gemm_bf16(m, n, k, epilogue):
    """a: a row-strided view (8 NaN columns in front of every row, 16 behind, NaN rows around); out guarded; epilogue 2: the residual
    x is read and written in place, inside a guarded buffer.  Epilogue 2 exists at N = 256 only: at N = 512 the entry point must refuse
    without touching out or x."""
    from mamba_asr_amd import ops
    g = torch.Generator().manual_seed(m + n + k)
    a = dev((torch.randn(1, m, k, generator=g) * 0.5).bfloat16())
    w, bias = dev((torch.randn(n, k, generator=g) * 0.1).bfloat16()), dev(torch.randn(n, generator=g))
    x = dev(torch.randn(m, n, generator=g))
    par = [dev(torch.randn(n, generator=g)) for _ in range(4)]

    def run(L):
        kw = {}
        if epilogue == 2:
            kw = dict(x=L.out("x", (m, n), F32, fill=x), alpha=0.5, norm1=(L.vec(par[0]), L.vec(par[1]), 1e-5), norm2=(L.vec(par[2]), L.vec(par[3]), 1e-6))
        av = (G.poisoned(a, rows=RT, left=G.LEFT, right=G.RIGHT) if L.guard else a.clone())[0]
        ret = ops.gemm_bf16(av, L.rows(w), L.vec(bias), epilogue=epilogue, out=L.out("out", (m, n), BF16), **kw)
        assert ret.data_ptr() == L.outs["out"].data_ptr()
    if epilogue == 2 and n != 256:
        L = Launch(True)
        with pytest.raises(RuntimeError, match="epilogue 2"):
            run(L)
        torch.cuda.synchronize()
        for name, (buf, view, outside) in L.g.items.items():
            G.assert_untouched(buf, outside, name)
        assert bool((L.outs["out"] == G.SENTINEL).all()) and torch.equal(L.outs["x"], x), "written by a refused launch"
        return
    two_step(run)


# ------------------------------------------------------------------------------------------------------------------------
# the output parameters themselves
# ------------------------------------------------------------------------------------------------------------------------
def test_output_parameters_are_checked_before_any_launch():
    """A caller's out / h_out / train_out of the wrong shape, dtype or layout is refused in Python; nothing is launched, nothing written."""
    from mamba_asr_amd import ops
    c, lp = _ffn_case(256, 256, 256, 16), _lnpw_case(256, 0)
    rows = 5
    x = c["x"][:rows].clone()
    pre = (c["pre"][0], c["pre"][1], 1e-5)
    t = lambda *s, dtype=BF16: torch.full(s, G.SENTINEL, dtype=dtype, device=DEV)
    ffn = lambda **kw: ops.ffn_fused(x, pre, c["w1"], c["b1"], c["w2"], c["b2"], **kw)
    dw = _dw_case(BF16, 80, True, False, 5, False)
    a, w = torch.zeros(rows, 64, dtype=BF16, device=DEV), torch.zeros(256, 64, dtype=BF16, device=DEV)
    bad = [
        (lambda o: ffn(h_out=o), [t(rows, 256, dtype=F32), t(rows + 1, 256), t(rows, 512)[:, :256]]),
        (lambda o: ffn(h_out=o, want_h=False), [t(rows, 256)]),
        (lambda o: ffn(h_out=o, norm2=pre, proj_w=c["wp"]), [t(rows, 256)]),
        (lambda o: ffn(train_out=(o, t(rows, 256), t(2, rows, dtype=F32))), [t(rows, 256)]),                       # no training forward asked for
        (lambda o: ffn(train=(0.0, 0.0, 1, 2), train_out=(o, t(rows, 256), t(2, rows, dtype=F32))), [t(rows, 512), t(rows, 256, dtype=F32)]),
        (lambda o: ffn(train=(0.0, 0.0, 1, 2), train_out=(t(rows, 256), t(rows, 256), o)), [t(rows, 2, dtype=F32), t(2, rows)]),
        (lambda o: ffn(train=(0.0, 0.0, 1, 2), h_out=o), [t(rows, 256)]),
        (lambda o: ops.ln_pw_glu(x, None, 1.0, (lp["ln"][0], lp["ln"][1], 1e-5), lp["w"], lp["bias"], out=o), [t(rows, 256, dtype=F32), t(rows, 144), t(rows, 512)[:, ::2]]),
        (lambda o: ops.glu_dwconv_ln_gelu(dw["inp"], dw["w"], dw["bs"], dw["lg"], dw["lb"], 1e-5, glu_done=True, out=o), [t(3, 5, 80, dtype=F32), t(3, 6, 80), t(3, 5, 160)[:, :, :80]]),
        (lambda o: ops.add_layernorm(x, out=o), [t(rows, 256, dtype=F32), t(rows, 128), t(rows, 512)[:, :256]]),
        (lambda o: ops.add_layernorm(x, out=o, want_out=False), [t(rows, 256)]),
        (lambda o: ops.gemm_bf16(a, w, out=o), [t(rows, 256, dtype=F32), t(rows, 512), t(rows, 512)[:, :256]]),
    ]
    keep = x.clone()
    ops.LAUNCH_LOG = log = []
    try:
        for call, outs in bad:
            for o in outs:
                with pytest.raises(RuntimeError):
                    call(o)
                assert bool((o == G.SENTINEL).all())
    finally:
        ops.LAUNCH_LOG = None
    torch.cuda.synchronize()
    assert log == [] and torch.equal(x, keep)
