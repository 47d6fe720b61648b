"""Guard bands (tests/guard_bands.py) around the decoding kernels: cm_mamba_step, cm_causal_conv1d_update, cm_selective_state_update,
cm_attn_step, cm_xattn_step, cm_beam_select, cm_ctc_prefix_score / _advance and the whole-utterance cm_ctc_beam_search /
cm_ctc_beam_lm_search.  Every case is G.two_step: a plain launch, then the same launch with its float inputs inside NaN, its integer
inputs inside guard values that name poison, its outputs and in-place states inside sentinels and its workspace a scratch.  The
guarded launch must have the plain launch's bits (finite where the plain one is) and write nothing outside an output, a state or a
workspace; the plain launch is held to the fp64 restatement and the bound of the kernel's own test file, which is imported:
    cm_mamba_step, the two update kernels     tests/test_row_kernels_fp64.check (tests/test_mamba_step_fused's bound), .ref_*
    cm_attn_step / cm_xattn_step              4 x |ops.*_torch - fp64|, at least one ulp (tests/test_attn_step_gpu, test_xattn_step_gpu)
    cm_beam_select                            torch.equal with tests/s2s_beam_ref.select (tests/test_beam_select_gpu)
    cm_ctc_prefix_*                           4 x |fp32 restatement - fp64| (tests/test_ctc_prefix_gpu._Err, tests/ctc_prefix_ref)
    the beam searches                         the bits of the call without bufs (tests/test_ctc_beam_stream_gpu._whole / _lm_ ...)
Each test prints the largest error / allowance ratio of its plain launches.

The guards are at least one workgroup's reach of the kernel under test (a whole batch row of cm_mamba_step's states, 256 channels of
the update kernels, a cache position of cm_attn_step, ...); a weight a workgroup reads whole has its own size of NaN either side.
_Spy reads the addresses each launch was really given: a wrapper that copied a guarded view would defeat the guard silently.
"""
import ctypes as ct
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_data as D  # noqa: E402
import ctc_prefix_ref as PR  # noqa: E402
import guard_bands as G  # noqa: E402
import s2s_beam_ref as SR  # noqa: E402
import test_attn_step_gpu as TA  # noqa: E402
import test_beam_select_gpu as TB  # noqa: E402
import test_ctc_beam_stream_gpu as BS  # noqa: E402
import test_ctc_lm_stream_gpu as LS  # noqa: E402
import test_ctc_prefix_gpu as TP  # noqa: E402
import test_mamba_step_fused as MS  # noqa: E402
import test_row_kernels_fp64 as RK  # noqa: E402
import test_xattn_step_gpu as TX  # noqa: E402
from test_ctc_lm_stream_gpu import arpa  # noqa: E402,F401  (the module-scoped fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
NEG = -math.inf
DTYPES = pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])


class _Spy:
    """ops._launch wrapped: the argument struct of every native launch, to compare the addresses a kernel was given with the tensors
    the test placed."""

    def __init__(self, monkeypatch):
        from mamba_asr_amd import ops
        self.calls = []
        real = ops._launch

        def launch(name, fn, args, units=0):
            self.calls.append((name, args))
            return real(name, fn, args, units)
        monkeypatch.setattr(ops, "_launch", launch)

    def given(self, kernel, **fields):
        """The last launch was ``kernel`` and got exactly these tensors (None: a NULL pointer)."""
        name, a = self.calls[-1]
        assert name == kernel, (name, kernel)
        for f, t in fields.items():
            got, want = getattr(a, f) or None, None if t is None else t.data_ptr()
            assert got == want, f"{kernel}: {f} is {got}, the test placed {want}: the wrapper copied it"


def _whole(L, t):
    """An input a workgroup reads whole (a weight): its own size of NaN in front and behind."""
    return None if t is None else L.around(t, rows=1 if t.dim() == 1 else t.shape[0])


def _dev(t):
    return None if t is None else t.to(DEV)


# ----------------------------------------------------------------------------------------------------------
# cm_mamba_step
# ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optional", [True, False], ids=["bias_D", "no_bias_D"])
@DTYPES
@pytest.mark.parametrize("batch,E,R", [(1, 8, 1), (3, 520, 9), (2, 4096, 32)])
def test_mamba_step(batch, E, R, dtype, optional, monkeypatch):
    """(1, 8, 1): the smallest supported row; (3, 520, 9): one 512-thread pass plus 8 channels, lanes 0 and 1 alone in the x_proj
    loop's third pass; (2, 4096, 32): the maximum, s_x full.  Two consecutive steps: the second starts from the states the first left.
    A workgroup owns one batch row: the states' guards are a whole row (E x 4, E x 16 floats) either side."""
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    w, xz, conv0, ssm0 = MS._case(batch, E, R, dtype)
    if not optional:
        w = dict(w, conv_b=None, dt_bias=None, D=None)
    wd = {k: _dev(v) for k, v in w.items()}
    wr = {k: torch.zeros(E, dtype=torch.float64) if v is None else v.double() for k, v in w.items()}
    conv, ssm, rconv, rssm = conv0.to(DEV), ssm0.to(DEV), conv0.double(), ssm0.double()
    for i in range(2):
        def run(L, x_dev=xz[i].to(DEV), conv=conv, ssm=ssm):
            x = L.rows(x_dev, rows=4)
            cs = L.out("conv_state", conv.shape, F32, fill=conv, contiguous=True, rows=E)
            ss = L.out("ssm_state", ssm.shape, F32, fill=ssm, contiguous=True, rows=E)
            wt = {k: _whole(L, v) for k, v in wd.items()}
            out = L.out("out", (batch, E), dtype, rows=4)
            got = ops.mamba_step(x, cs, ss, wt["conv_w"], wt["conv_b"], wt["x_proj"], wt["dt_proj"], wt["dt_bias"], wt["A"], wt["D"],
                                 bufs={"out": out})
            assert got is out
            spy.given("cm_mamba_step", xz=x, conv_state=cs, ssm_state=ss, out=out, conv_weight=wt["conv_w"], conv_bias=wt["conv_b"],
                      x_proj_weight=wt["x_proj"], dt_proj_weight=wt["dt_proj"], dt_bias=wt["dt_bias"], A=wt["A"], D=wt["D"])
        outs = G.two_step(run, DEV)
        y, rconv, rssm = MS.ref_step(xz[i].double(), rconv, rssm, wr)
        ey = RK.check("mamba_step y", outs["out"], y)
        ec, es = RK.check("mamba_step conv_state", outs["conv_state"], rconv), RK.check("mamba_step ssm_state", outs["ssm_state"], rssm)
        print(f"mamba_step ({batch}, {E}, {R}) {dtype} optional {optional} step {i}: max|y err| {ey:.3e} max|conv err| {ec:.3e} "
              f"max|ssm err| {es:.3e}")
        conv, ssm = outs["conv_state"], outs["ssm_state"]
    assert len(spy.calls) == 4                                      # one launch per call
    RK.report("mamba_step")


# ----------------------------------------------------------------------------------------------------------
# cm_causal_conv1d_update / cm_selective_state_update: 256 (batch, channel) threads per workgroup, the last one partial
# ----------------------------------------------------------------------------------------------------------
@DTYPES
@pytest.mark.parametrize("batch,dim,width", [(1, 8, 4), (3, 100, 2)])
def test_causal_conv1d_update(batch, dim, width, dtype, monkeypatch):
    from mamba_asr_amd import ops
    assert (batch * dim) % 256
    spy = _Spy(monkeypatch)
    g = RK.gen(1000 * dim + 10 * width + batch + 7)
    w, b = torch.randn(dim, width, generator=g) * 0.5, torch.randn(dim, generator=g) * 0.3
    st0 = torch.randn(batch, dim, width, generator=g)
    x0 = (torch.randn(batch, dim, generator=g) * 1.5).to(dtype)
    for has_bias, silu in ((True, True), (False, False)):
        bias = b if has_bias else None

        def run(L):
            x = L.rows(x0.to(DEV))                                   # 64 rows: at least 256 elements
            st = L.out("conv_state", st0.shape, F32, fill=st0.to(DEV), contiguous=True, rows=256)
            wv, bv = _whole(L, w.to(DEV)), _whole(L, _dev(bias))
            out = L.out("out", (batch, dim), dtype)
            assert ops.causal_conv1d_update(x, st, wv, bv, silu=silu, bufs={"out": out}) is out
            spy.given("cm_causal_conv1d_update", x=x, conv_state=st, weight=wv, bias=bv, out=out)
        outs = G.two_step(run, DEV)
        rout, rst = RK.ref_conv_update(st0.double(), x0.double(), w.double(), None if bias is None else bias.double(), silu)
        e = RK.check("causal_conv1d_update out", outs["out"], rout)
        assert torch.equal(outs["conv_state"].cpu(), rst.float()), "the conv state is not shift-left-append"
        print(f"conv_update ({batch}, {dim}, {width}) {dtype} bias {has_bias} silu {silu}: max|out err| {e:.3e}")
    RK.report("causal_conv1d_update")


@DTYPES
@pytest.mark.parametrize("batch,dim,dstate", [(1, 8, 16), (5, 130, 64)])
def test_selective_state_update(batch, dim, dstate, dtype, monkeypatch):
    from mamba_asr_amd import ops
    assert (batch * dim) % 256
    spy = _Spy(monkeypatch)
    g = RK.gen(1000 * dim + 10 * dstate + batch + 7)
    A = -torch.exp(torch.randn(dim, dstate, generator=g) * 0.5)
    Dw, st0 = torch.randn(dim, generator=g), torch.randn(batch, dim, dstate, generator=g)
    rn = lambda *s: torch.randn(*s, generator=g).to(dtype)  # noqa: E731
    x, B, Cm, z0 = rn(batch, dim), rn(batch, dstate), rn(batch, dstate), rn(batch, dim)
    u = torch.rand(batch, dim, generator=g)
    for full in (True, False):                                       # every optional input and softplus, or none of them
        dt = (u * 59.0 - 29.5 if full else u * 0.5 + 0.01).to(dtype)
        db = (torch.rand(dim, generator=g) - 0.5) if full else None
        Dv, z = (Dw, z0) if full else (None, None)

        def run(L):
            st = L.out("state", st0.shape, F32, fill=st0.to(DEV), contiguous=True, rows=256)
            xv, dtv, zv, Bv, Cv = (L.rows(_dev(t)) for t in (x, dt, z, B, Cm))
            Av, Dg, dbv = _whole(L, A.to(DEV)), _whole(L, _dev(Dv)), _whole(L, _dev(db))
            out = L.out("out", (batch, dim), dtype)
            assert ops.selective_state_update(st, xv, dtv, Av, Bv, Cv, Dg, zv, dbv, dt_softplus=full, bufs={"out": out}) is out
            spy.given("cm_selective_state_update", state=st, x=xv, dt=dtv, A=Av, B=Bv, C=Cv, D=Dg, z=zv, dt_bias=dbv, out=out)
        outs = G.two_step(run, DEV)
        d64 = lambda t: None if t is None else t.double()  # noqa: E731
        ry, rst = RK.ref_state_update(st0.double(), d64(x), d64(dt), d64(A), d64(B), d64(Cm), d64(Dv), d64(z), d64(db), full)
        ey, es = RK.check("selective_state_update y", outs["out"], ry), RK.check("selective_state_update state", outs["state"], rst)
        print(f"state_update ({batch}, {dim}, {dstate}) {dtype} optional {full}: max|y err| {ey:.3e} max|state err| {es:.3e}")
    RK.report("selective_state_update")


# ----------------------------------------------------------------------------------------------------------
# cm_attn_step
# ----------------------------------------------------------------------------------------------------------
RATIO = {}


def _note(kernel, err, tol):
    RATIO[kernel] = max(RATIO.get(kernel, 0.0), err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
    print(f"worst {kernel} so far: max err / allowance {RATIO[kernel]:.3f}")


GAP, PAD_POS = 16, 2              # sentinel columns between cache positions; sentinel positions in front of and behind a cache


def _cache(L, c, dead, t):
    """A (Lcap, R, D) cache as attn_step takes it, position stride R * D + GAP.  Guarded: the gaps and PAD_POS whole positions either
    side hold the sentinel, the lines ``dead`` (Lcap, R) no ancestry names hold NaN.  Line t is NaN in both launches: the kernel writes
    it.  -> (buffer, view, outside mask)"""
    Lcap, R, Dm = c.shape
    buf = torch.full((PAD_POS + Lcap + PAD_POS, R * Dm + GAP), G.SENTINEL if L.guard else 0.0, dtype=c.dtype, device=DEV)
    view = buf[PAD_POS:PAD_POS + Lcap, :R * Dm].view(Lcap, R, Dm)
    view.copy_(c)
    if L.guard:
        view[dead] = float("nan")
    view[t] = float("nan")
    outside = torch.ones(buf.shape, dtype=torch.bool, device=DEV)
    outside[PAD_POS:PAD_POS + Lcap, :R * Dm] = False
    assert (Lcap == 1 or view.stride(0) == R * Dm + GAP) and view.stride()[1:] == (Dm, 1) and view.data_ptr() % 16 == 0
    return buf, view, outside


def _attn(H, dh, t, R, dtype, monkeypatch):
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    g = torch.Generator().manual_seed(H * 100000 + t * 10 + R)
    Dm, Lcap = H * dh, t + 1
    qkv = torch.randn(R, 3 * Dm, generator=g).to(dtype).to(DEV)
    kc, vc = (torch.randn(Lcap, R, Dm, generator=g).to(dtype).to(DEV) for _ in range(2))
    spare = R - 1                                                    # R > 1: the row no hypothesis' ancestry names
    anc = torch.randint(0, max(R - 1, 1), (Lcap, R), generator=g).int()
    named = torch.zeros(Lcap, R, dtype=torch.bool).scatter_(1, anc.long(), True)
    anc[t] = spare                                                   # rows >= t are not read: a valid row whose cached lines are NaN
    named[t] = False
    anc, dead = anc.to(DEV), (~named).to(DEV)
    assert R == 1 or bool(dead[:t, spare].all())
    bits = torch.int32 if dtype == F32 else torch.int16

    def run(L):
        q = L.rows(qkv, rows=4)
        (kbuf, k1, kout), (vbuf, v1, vout) = _cache(L, kc, dead, t), _cache(L, vc, dead, t)
        before = k1.clone().view(bits), v1.clone().view(bits)
        a = L.ints(anc, spare, rows=2, unique=False)
        out = L.out("out", (R, Dm), dtype, rows=4)
        assert ops.attn_step(q, k1, v1, a, t, H, bufs={"out": out}) is out
        spy.given("cm_attn_step", qkv=q, kc=k1, vc=v1, anc=a, out=out)
        torch.cuda.synchronize()
        # line t holds the bits of this step's k and v; nothing else in the caches, their gaps or around them changed
        assert torch.equal(k1[t].view(bits), q[:, Dm:2 * Dm].contiguous().view(bits))
        assert torch.equal(v1[t].view(bits), q[:, 2 * Dm:].contiguous().view(bits))
        keep = [s for s in range(Lcap) if s != t]
        assert torch.equal(k1.clone().view(bits)[keep], before[0][keep]) and torch.equal(v1.clone().view(bits)[keep], before[1][keep])
        if L.guard:
            G.assert_untouched(kbuf, kout, "kc")
            G.assert_untouched(vbuf, vout, "vc")
        else:
            assert not bool(kbuf[:, R * Dm:].any()) and not bool(vbuf[:, R * Dm:].any())
    outs = G.two_step(run, DEV)
    ref = TA._ref64(qkv, kc, vc, anc, t, H)
    base = ops.attn_step_torch(qkv, kc.clone(), vc.clone(), anc, t, H)
    d_torch, d_native = float((base.double().cpu() - ref).abs().max()), float((outs["out"].double().cpu() - ref).abs().max())
    tol = max(4.0 * d_torch, TA._ulp(dtype, float(ref.abs().max())))
    print(f"attn_step R {R} H {H} dh {dh} t {t} {str(dtype)[6:]}: |native - fp64| {d_native:.3e}, |torch - fp64| {d_torch:.3e}, "
          f"tolerance {tol:.3e}")
    assert d_native <= tol
    _note("attn_step", d_native, tol)


@DTYPES
@pytest.mark.parametrize("t", [0, 1, 64, 65])
@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("H,dh", [(2, 32), (3, 64)])
def test_attn_step(H, dh, R, t, dtype, monkeypatch):
    """Lcap = t + 1: the line written is the cache's last, the sentinel positions lie directly behind it.  R * H = 15: the last
    workgroup has 3 of its 4 waves; t = 64, 65: the second pass of a lane over the positions."""
    _attn(H, dh, t, R, dtype, monkeypatch)


@DTYPES
def test_attn_step_two_waves_per_workgroup(dtype, monkeypatch):
    """t = 1024: 1088 score slots, two waves per workgroup; R * H = 9 units: the last workgroup has one."""
    _attn(3, 32, 1024, 3, dtype, monkeypatch)


# ----------------------------------------------------------------------------------------------------------
# cm_xattn_step
# ----------------------------------------------------------------------------------------------------------
XROWS = [2, 0, 1, 1, 0, 2, 7]                                       # 7: no utterance; it gives zeros and loads nothing


@DTYPES
@pytest.mark.parametrize("T", [1, 64, 65])
@pytest.mark.parametrize("H,dh", TX.HEADS)
def test_xattn_step(H, dh, T, dtype, monkeypatch):
    """K and V are the halves of one (U, T, 2 D) buffer inside NaN columns, 8 NaN frames behind every utterance and a NaN utterance
    either side; frames at or past enc_len are NaN in both launches.  enc_len[0] = T + 5 must be clamped to T: the 5 frames behind
    are NaN."""
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    g = torch.Generator().manual_seed(H * 100000 + dh * 1000 + T)
    Dm, R, U = H * dh, len(XROWS), 3
    q = torch.randn(R, Dm, generator=g).to(dtype).to(DEV)
    kv = torch.randn(U, T, 2 * Dm, generator=g)
    lens = [T + 5, max(T - 1, 1), 1]
    for u, n in enumerate(lens):
        kv[u, n:] = float("nan")
    kv = kv.to(dtype).to(DEV)
    row_utt, enc_len = torch.tensor(XROWS, dtype=I32, device=DEV), torch.tensor(lens, dtype=I32, device=DEV)

    def run(L):
        qv, kvv = L.rows(q, rows=4), L.cols(kv, rows=8)
        k, v = kvv[..., :Dm], kvv[..., Dm:]
        ru, el = L.ints(row_utt, 1, unique=False), L.ints(enc_len, T, unique=False)
        out = L.out("out", (R, Dm), dtype, rows=4)
        assert ops.xattn_step(qv, k, v, ru, el, H, bufs={"out": out}) is out
        spy.given("cm_xattn_step", q=qv, k=k, v=v, row_utt=ru, enc_len=el, out=out)
    outs = G.two_step(run, DEV)
    k, v = kv[..., :Dm], kv[..., Dm:]
    ref = TX._ref64(q, k, v, row_utt.cpu(), enc_len.cpu(), H)
    base = ops.xattn_step_torch(q, k, v, row_utt, enc_len, H)
    d_torch, d_native = float((base.double().cpu() - ref).abs().max()), float((outs["out"].double().cpu() - ref).abs().max())
    tol = max(4.0 * d_torch, TX._ulp(dtype, float(ref.abs().max())))
    print(f"xattn_step H {H} dh {dh} T {T} {str(dtype)[6:]}: |native - fp64| {d_native:.3e}, |torch - fp64| {d_torch:.3e}, tolerance {tol:.3e}")
    assert d_native <= tol and bool((outs["out"][6] == 0).all())
    _note("xattn_step", d_native, tol)


# ----------------------------------------------------------------------------------------------------------
# cm_beam_select: two launches with a workspace between them
# ----------------------------------------------------------------------------------------------------------
SELECT_SHAPES = [(1, 1, 1), (3, 5, 37), (2, 66, 165),
                 (2, 3, 5121),          # two chunks, the last of one token: K = 1 < B, wcomp[1..B) zero-filled
                 (1, 128, 5248),        # the last chunk has exactly B tokens
                 (2, 8, 10241)]         # three chunks


@pytest.mark.parametrize("full", [False, True], ids=["att", "delta_blocked"])
@pytest.mark.parametrize("shape", SELECT_SHAPES)
def test_beam_select(shape, full, monkeypatch):
    """The workspace is a scratch of exactly cm_beam_select_workspace_bytes: a merge that reads a word the first launch did not write
    meets NaN bits.  A workgroup of the first launch reads one chunk of one row: att and delta have at least a chunk of NaN either side."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    U, B, V = shape
    att, alive, delta = TB._inputs(U, B, V, 11)
    eos = TB._eos(V)
    blocked = torch.tensor(([1, 0, 1][:U] if V > 1 else [0]), dtype=I32, device=DEV)    # V = 1: the only token stays choosable
    kw = dict(delta=delta, weight=0.4, eos_blocked=blocked) if full else {}
    nws = int(N.lib().cm_beam_select_workspace_bytes(U, B, V))
    assert nws == U * B * -(-V // N.CM_BEAM_SELECT_CHUNK) * B * 12
    rows = -(-N.CM_BEAM_SELECT_CHUNK // V)
    names = ("score", "inc", "parent", "token")

    def run(L):
        a, al = L.around(att, rows=rows), L.around(alive, rows=4)
        d = L.around(delta, rows=rows) if full else None
        eb = L.ints(blocked, 1, unique=False) if full else None
        bufs = {n: L.out(n, (U, B), dt, free=True) for n, dt in (("score", F32), ("inc", F32), ("parent", I32), ("token", I32))}
        bufs["workspace"] = L.scratch("workspace", nws // 4).view(torch.uint8)
        got = ops.beam_select(a, al, B, eos, delta=d, weight=0.4 if full else 0.0, eos_blocked=eb, bufs=bufs)
        assert all(x is bufs[n] for x, n in zip(got, names))
        spy.given("cm_beam_select", att=a, alive=al, delta=d, eos_blocked=eb, **bufs)
        assert spy.calls[-1][1].workspace_bytes == nws
    outs = G.two_step(run, DEV)
    want = SR.select(att, alive, B, eos, **kw)
    assert torch.equal(outs["score"], want[0]) and torch.equal(outs["parent"], want[2]) and torch.equal(outs["token"], want[3])
    fin = torch.isfinite(outs["score"])
    assert bool(fin.all()) and torch.equal(outs["inc"][fin], want[1][fin])


# ----------------------------------------------------------------------------------------------------------
# cm_ctc_prefix_score / cm_ctc_prefix_advance
# ----------------------------------------------------------------------------------------------------------
BLANK, EOS = TP.BLANK, TP.EOS
PROWS = [0, 1, 0, 1, 7]                                             # row 4 names no utterance


def _prefix_case(T, V):
    """U = 2, n_u = (T, max(1, T - 3)); row 0 holds the empty prefix, rows 1-3 one token (the fp64 restatement's state rounded to
    fp32: the input of the kernels and of both restatements), row 4 has no utterance and NaN for a state.  Frames at or past n_u are
    NaN in logp and in the states."""
    g = torch.Generator().manual_seed(1000 * T + V)
    logp = torch.log_softmax(torch.randn(2, T, V, generator=g) * 2.0, dim=-1)
    n_u = [T, max(1, T - 3)]
    a, b = (1, 1) if V == 3 else (5, 9)
    r64 = PR.RefCTCPrefixScorer(BLANK, EOS, np.float64)
    st = r64.advance(r64.init(logp, n_u, PROWS[:4]), torch.tensor([EOS, a, b, a]))
    r_n, r_b, psi, last = PR.padded(st, T)
    r_n32, r_b32, psi32 = r_n.astype(np.float32), r_b.astype(np.float32), psi.astype(np.float32)

    def state(dtype):
        rows = [(r_n32[i, :n_u[u]].astype(dtype), r_b32[i, :n_u[u]].astype(dtype), dtype(psi32[i]), int(last[i])) for i, u in enumerate(PROWS[:4])]
        return {"lp": [logp[u, :n].numpy().astype(dtype) for u, n in enumerate(n_u)], "row_utt": PROWS[:4], "rows": rows}
    nan_row = np.full((1, T), np.nan, dtype=np.float32)
    for u, n in enumerate(n_u):
        logp[u, n:] = float("nan")
    dev = dict(logp=logp.to(DEV), n_u=torch.tensor(n_u, dtype=I32, device=DEV), row_utt=torch.tensor(PROWS, dtype=I32, device=DEV),
               last=torch.tensor(list(last) + [1], dtype=I32, device=DEV), r_n=torch.from_numpy(np.concatenate([r_n32, nan_row])).to(DEV),
               r_b=torch.from_numpy(np.concatenate([r_b32, nan_row])).to(DEV),
               psi_g=torch.from_numpy(np.concatenate([psi32, [np.float32(np.nan)]])).to(DEV))
    assert bool(torch.isnan(dev["r_n"][1, n_u[1]:]).all()) and not bool(torch.isnan(dev["r_n"][:4, :n_u[1]]).any())
    return dev, state, n_u, (a, b)


def _prefix_inputs(L, dev, T, V):
    """The seven shared inputs placed: a workgroup reads one row's states and one utterance's posteriors."""
    return (L.around(dev["logp"], rows=T), L.ints(dev["n_u"], 0), L.ints(dev["row_utt"], 1, unique=False), L.ints(dev["last"], V - 1),
            L.around(dev["r_n"], rows=2), L.around(dev["r_b"], rows=2), L.around(dev["psi_g"], rows=64))


PREFIX_SHAPES = [(1, 3), (65, 70), (513, 65)]


def _prefix_check(err, T, what):
    tol = 4.0 * err.fp32
    print(f"{what}: max|kernel - fp64| {err.kernel:.3e}, max|fp32 restatement - fp64| {err.fp32:.3e}, allowed {tol:.3e}")
    assert err.fp32 > 0.0 or T == 1                                  # one frame: every value is a copy or a difference of copies, exact in fp32
    assert err.kernel <= tol, f"{what}: kernel error {err.kernel:.3e} > 4 x fp32 restatement error {err.fp32:.3e}"
    _note(what.split()[0], err.kernel, tol)


@pytest.mark.parametrize("K", [0, 3, 65], ids=["all", "K3", "K65"])
@pytest.mark.parametrize("T,V", PREFIX_SHAPES)
def test_ctc_prefix_score(T, V, K, monkeypatch):
    """(1, 3): one frame; (65, 70): a second candidate tile of 6 lanes; (513, 65): a second TCHUNK of one frame, a second candidate tile
    with one live lane.  K = 3 holds a candidate outside [0, V)."""
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    dev, state, n_u, _ = _prefix_case(T, V)
    cand = None
    if K == 3:
        cand = torch.tensor([[1, V + 3, V - 1], [V - 1, 1, -1], [1, 1, 0], [EOS, 1, 2 ** 30], [1, EOS, V]], dtype=I32, device=DEV)
    elif K:
        cand = torch.randint(0, V, (5, K), generator=torch.Generator().manual_seed(K)).int().to(DEV)

    def run(L):
        logp, n, ru, last, r_n, r_b, psi = _prefix_inputs(L, dev, T, V)
        c = L.ints(cand, V - 1, rows=2, unique=False)
        out = L.out("out", (5, K or V), F32, rows=2, align=4, free=True)
        assert ops.ctc_prefix_score(logp, n, ru, last, r_n, r_b, psi, BLANK, EOS, candidates=c, validated=True, bufs={"out": out}) is out
        spy.given("cm_ctc_prefix_score", logp=logp, n_u=n, row_utt=ru, last=last, r_n=r_n, r_b=r_b, psi_g=psi, candidates=c, out=out)
    got = G.two_step(run, DEV)["out"].cpu()
    assert bool((got[4] == NEG).all())
    err = TP._Err()
    refs = [PR.RefCTCPrefixScorer(BLANK, EOS, dt).score(state(dt), None if cand is None else cand[:4]) for dt in (np.float32, np.float64)]
    err.add(got[:4].numpy(), refs[0].numpy(), refs[1].numpy(), "deltas")
    _prefix_check(err, T, f"ctc_prefix_score T={T} V={V} K={K}")


@pytest.mark.parametrize("T,V", PREFIX_SHAPES)
def test_ctc_prefix_advance(T, V, monkeypatch):
    """Row 0 extends the empty prefix, row 1 repeats its last token, row 2 takes <eos> and keeps its state bit for bit, row 3 takes
    blank and row 4 has no utterance: both are impossible, -inf everywhere.  T = 65, 513: the 64-frame scan's second and ninth pass."""
    from mamba_asr_amd import ops
    spy = _Spy(monkeypatch)
    dev, state, n_u, (a, b) = _prefix_case(T, V)
    tokens = torch.tensor([a, a, EOS, BLANK, a], dtype=I32, device=DEV)
    assert int(dev["last"][1]) == a and int(dev["last"][0]) == -1

    def run(L):
        logp, n, ru, last, r_n, r_b, psi = _prefix_inputs(L, dev, T, V)
        tk = L.ints(tokens, V - 1, unique=False)
        bufs = {"r_n_out": L.out("r_n_out", (5, T), F32, rows=2, align=4, free=True),
                "r_b_out": L.out("r_b_out", (5, T), F32, rows=2, align=4, free=True),
                "psi_out": L.out("psi_out", (5,), F32, free=True), "last_out": L.out("last_out", (5,), I32)}
        got = ops.ctc_prefix_advance(logp, n, ru, last, r_n, r_b, psi, tk, BLANK, EOS, validated=True, bufs=bufs)
        assert all(x is bufs[k] for x, k in zip(got, ("r_n_out", "r_b_out", "psi_out", "last_out")))
        spy.given("cm_ctc_prefix_advance", logp=logp, n_u=n, row_utt=ru, last=last, r_n=r_n, r_b=r_b, psi_g=psi, tokens=tk, **bufs)
    outs = {k: v.cpu() for k, v in G.two_step(run, DEV).items()}
    assert outs["last_out"].tolist() == [a, a, int(dev["last"][2]), BLANK, a]
    for row in (3, 4):
        assert bool((outs["r_n_out"][row] == NEG).all()) and bool((outs["r_b_out"][row] == NEG).all()) and float(outs["psi_out"][row]) == NEG
    for name, src in (("r_n_out", "r_n"), ("r_b_out", "r_b")):
        assert torch.equal(outs[name][2], dev[src][2].cpu())         # <eos>: kept (utterance 0 has all T frames: nothing NaN in it)
        assert bool((outs[name][1, n_u[1]:] == NEG).all())           # frames at or past n_u of a row that moved on: exactly -inf
    assert float(outs["psi_out"][2]) == float(dev["psi_g"][2])
    err = TP._Err()
    for dt in (np.float32, np.float64):
        r = PR.RefCTCPrefixScorer(BLANK, EOS, dt)
        pad = PR.padded(r.advance(state(dt), torch.tensor([a, a, EOS, EOS])), T)
        if dt == np.float32:
            p32 = pad
    for i, name in enumerate(("r_n_out", "r_b_out", "psi_out")):
        err.add(outs[name][:3].numpy(), p32[i][:3], pad[i][:3], name)
    _prefix_check(err, T, f"ctc_prefix_advance T={T} V={V}")


# ----------------------------------------------------------------------------------------------------------
# cm_ctc_beam_search / cm_ctc_beam_lm_search, whole utterance
# ----------------------------------------------------------------------------------------------------------
FRAMES, LENGTHS = 16, [16, 0, 9]


def _beam_bufs(L, topk, nws, lm):
    """Every output and the workspace placed.  The kernels leave rows past num_hyps and token positions past token_len alone: both
    launches start them from zero, as the wrapper's own tensors do."""
    names = (("tokens", (3, topk, FRAMES), I32), ("token_len", (3, topk), I32), ("scores", (3, topk), torch.float64)) \
        + ((("lm_scores", (3, topk), torch.float64),) if lm else ()) + (("num_hyps", (3,), I32), ("bad_frame", (3,), I32))
    bufs = {n: L.out(n, shape, dt, fill=0, contiguous=True) for n, shape, dt in names}
    bufs["workspace"] = L.scratch("workspace", nws // 4).view(torch.uint8)
    return bufs, tuple(n for n, _, _ in names)


def _poison_tail(lp):
    lp = lp.clone()
    for b, n in enumerate(LENGTHS):
        lp[b, n:] = float("nan")                                     # frames at or past an utterance's length are never read
    return lp.to(DEV)


def test_ctc_beam_search_whole_utterance(monkeypatch):
    """tests/test_ctc_beam_stream_gpu's global_sort regime (beam 100 x 31 tokens: the sorts run in the workspace), 16 frames, lengths
    (16, 0, 9); log_probs a strided view inside NaN rows, columns and utterances."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    spy = _Spy(monkeypatch)
    gen, kw = BS.REGIMES["global_sort"]
    s = BS._searcher(max_frames=FRAMES, **kw)
    lp = _poison_tail(BS._data(gen, frames=FRAMES))
    tc, th, tp = s._tables(DEV)
    lengths = torch.tensor(LENGTHS, dtype=I32, device=DEV)
    a = N.CtcBeamArgs()
    a.batch, a.T, a.V, a.beam_size = 3, FRAMES, BS.V, s.beam_size
    nws = int(N.lib().cm_ctc_beam_workspace_bytes(ct.byref(a)))
    assert nws > 3 * FRAMES * s.beam_size * 4 and nws % 16 == 0      # more than the histories: the sort arrays are in it

    def run(L):
        x, n = L.cols(lp, align=4, rows=4), L.ints(lengths, 12)
        bufs, names = _beam_bufs(L, s.topk, nws, lm=False)
        got = ops.ctc_beam_search(x, n, tc, th, tp, HASH_BASE, HASH_SEP, blank=s.blank_index, beam_size=s.beam_size, topk=s.topk,
                                  prune_history=s.prune_history, beam_prune_logp=s.beam_prune_logp,
                                  token_prune_min_logp=s.token_prune_min_logp, blank_skip_threshold=s.blank_skip_threshold, bufs=bufs)
        assert all(t is bufs[k] for t, k in zip(got, names))
        spy.given("cm_ctc_beam_search", log_probs=x, lengths=n, **bufs)
    outs = G.two_step(run, DEV)
    assert outs["bad_frame"].tolist() == [-1, -1, -1] and int(outs["num_hyps"][0]) >= 1
    BS._same(BS._norm([outs[k] for k in ("tokens", "token_len", "scores", "num_hyps")]), BS._whole(s, lp, LENGTHS))


def test_ctc_beam_lm_search_whole_utterance(arpa, monkeypatch):  # noqa: F811
    """tests/test_ctc_lm_stream_gpu's global_sort regime and LM tables; otherwise as the LM-free case."""
    import mamba_asr_amd._native as N
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import HASH_BASE, HASH_SEP
    spy = _Spy(monkeypatch)
    s = LS._searcher(arpa(4, **LS.RICH), max_frames=FRAMES, **LS.GLOBAL_SORT)
    lp = _poison_tail(LS._batch(D.competing, [FRAMES] * 3, FRAMES, 100))
    tc, th, tp = s._tables(DEV)
    tl, lm = s._tok_len(DEV), s.lm.tables(DEV)
    lengths = torch.tensor(LENGTHS, dtype=I32, device=DEV)
    a = N.CtcBeamLmArgs()
    a.batch, a.T, a.V, a.beam_size = 3, FRAMES, LS.V, s.beam_size
    nws = int(N.lib().cm_ctc_beam_lm_workspace_bytes(ct.byref(a)))
    assert nws > 3 * FRAMES * s.beam_size * 4 and nws % 16 == 0

    def run(L):
        x, n = L.cols(lp, align=4, rows=4), L.ints(lengths, 12)
        bufs, names = _beam_bufs(L, s.topk, nws, lm=True)
        got = ops.ctc_beam_search_lm(x, n, tc, th, tp, tl, HASH_BASE, HASH_SEP, lm, bufs=bufs, **LS._lm_kw(s))
        assert all(t is bufs[k] for t, k in zip(got, names))
        spy.given("cm_ctc_beam_lm_search", log_probs=x, lengths=n, **bufs)
    outs = G.two_step(run, DEV)
    assert outs["bad_frame"].tolist() == [-1, -1, -1] and int(outs["num_hyps"][0]) >= 1
    LS._same(LS._norm([outs[k] for k in LS.NAMES], FRAMES), LS._whole(s, lp, LENGTHS, width=FRAMES))
