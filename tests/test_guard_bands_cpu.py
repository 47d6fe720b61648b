"""tests/guard_bands.py catches what it is for: fake "kernels" written in torch on CPU tensors -- one that writes a row past its view,
one that writes a column to the left, one that writes the first row behind an utterance, one that folds a row from outside its input
view into a row sum -- are each flagged with the tensor's name, and a correct one passes.  The GPU tests
(tests/test_forward_guards_gpu.py) make the same calls on real kernels; this file is why they are not vacuous."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_bands as G  # noqa: E402

CPU = torch.device("cpu")
DTYPES = [torch.float32, torch.bfloat16]


def _reach(view, size, offset=0):
    """What a kernel holding the view's pointer and strides can address: ``size`` elements per axis, ``offset`` elements from the view's start."""
    return view.as_strided(size, view.stride(), view.storage_offset() + offset)


# fake kernels: out = 2 x inp on (rows, D) / (batch, seqlen, width) views -------------------------------------------------
def k_rows_correct(inp, out):
    out.copy_(2 * inp)


def k_rows_one_past(inp, out):
    """The ragged last tile's row test is off by one: row ``rows`` is stored as well."""
    r, d = out.shape
    out.copy_(2 * inp)
    _reach(out, (r + 1, d))[r] = 1.0


def k_cols_correct(inp, out):
    out.copy_(2 * inp)


def k_cols_one_left(inp, out):
    """A column slice written one element too far to the left."""
    out.copy_(2 * inp)
    _reach(out, out.shape, -1)[0, 0, 0] = 1.0


def k_next_utterance(inp, out):
    """The time tile's ``t < seqlen`` test is missing: step ``seqlen`` -- in a dense batch the next utterance's first row -- is stored."""
    b, l, w = out.shape
    out.copy_(2 * inp)
    _reach(out, (b, l + 1, w))[:, l] = 1.0


def k_halo_sum(inp, out, clamp):
    """out[t] = inp[t - 1] + inp[t] + inp[t + 1]; ``clamp``: rows outside the utterance count as zero, else they are read where they lie."""
    b, l, w = inp.shape
    wide = _reach(inp, (b, l + 2, w), -inp.stride(1)).clone()              # rows -1 .. l as they lie in memory
    if clamp:
        wide[:, 0], wide[:, l + 1] = 0.0, 0.0
    out.copy_(wide[:, :l] + wide[:, 1:l + 1] + wide[:, 2:])


# geometry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_rows(dtype):
    buf, view, outside = G.guarded((5, 24), dtype, CPU, rows=G.ROW_TILE)
    assert view.shape == (5, 24) and view.is_contiguous() and view.data_ptr() % 16 == 0
    assert buf.numel() == (5 + 2 * G.ROW_TILE) * 24 and int(outside.sum()) == 2 * G.ROW_TILE * 24
    assert bool((buf == G.SENTINEL).all()) and float(torch.tensor(G.SENTINEL, dtype=dtype)) == G.SENTINEL
    # guard rows lie directly in front of and behind the view
    assert float(_reach(view, (1, 24), -24)[0, 0]) == G.SENTINEL and float(_reach(view, (6, 24))[5, 0]) == G.SENTINEL
    G.assert_untouched(buf, outside, "fresh")


@pytest.mark.parametrize("dtype", DTYPES)
def test_geometry_columns(dtype):
    b, l, w = 2, 5, 24
    buf, view, outside = G.guarded((b, l, w), dtype, CPU, rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
    assert view.shape == (b, l, w) and view.stride() == ((l + G.TIME_TILE) * (w + 24), w + 24, 1) and view.data_ptr() % 16 == 0
    assert buf.shape == (b + 2, l + G.TIME_TILE, G.LEFT + w + G.RIGHT)
    assert int(outside.sum()) == buf.numel() - b * l * w
    assert not bool(outside[1:b + 1, :l, G.LEFT:G.LEFT + w].any()) and bool(outside[0].all()) and bool(outside[b + 1].all())
    assert bool(outside[1:b + 1, l:].all()) and bool(outside[:, :, :G.LEFT].all()) and bool(outside[:, :, G.LEFT + w:].all())
    flat, view3, mask3 = G.guarded((b, l, w), dtype, CPU, rows=G.TIME_TILE, contiguous=True)
    assert view3.is_contiguous() and flat.dim() == 1 and int(mask3.sum()) == 2 * G.TIME_TILE * w


@pytest.mark.parametrize("dtype", DTYPES)
def test_poisoned_keeps_values_and_geometry(dtype):
    t = torch.randn(2, 5, 24).to(dtype)
    _, view, _ = G.guarded(t.shape, dtype, CPU, rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
    p = G.poisoned(t, rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
    assert torch.equal(p, t) and p.stride() == view.stride() and p.storage_offset() == view.storage_offset()
    around = _reach(p, (2, 7, 26), -p.stride(1) - 1).clone()                 # one row and one column on every side
    around[:, 1:6, 1:25] = float("nan")
    assert bool(torch.isnan(around).all())
    p2 = G.poisoned(t[0], rows=G.ROW_TILE)
    assert p2.is_contiguous() and torch.equal(p2, t[0])
    assert bool(torch.isnan(_reach(p2, (1, 24), -24)).all()) and bool(torch.isnan(_reach(p2, (6, 24))[5]).all())


# the faulty kernels are flagged, the correct ones pass -------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [1, 63, 65])
def test_row_kernels(dtype, rows):
    inp = torch.randn(rows, 24).to(dtype)
    want = torch.empty_like(inp)
    k_rows_correct(inp, want)
    g = G.Guards(CPU)
    k_rows_correct(G.poisoned(inp), g.out("rows_out", inp.shape, dtype))
    g.check({"rows_out": want})
    g = G.Guards(CPU)
    k_rows_one_past(G.poisoned(inp), g.out("rows_out", inp.shape, dtype))
    with pytest.raises(AssertionError, match=r"rows_out: 24 element\(s\) written outside the view"):
        g.check({"rows_out": want})


@pytest.mark.parametrize("dtype", DTYPES)
def test_column_slice_kernels(dtype):
    inp = torch.randn(2, 5, 24).to(dtype)
    want = 2 * inp
    kw = dict(rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
    g = G.Guards(CPU)
    k_cols_correct(G.poisoned(inp, **kw), g.out("ucat_f", inp.shape, dtype, **kw))
    g.check({"ucat_f": want})
    g = G.Guards(CPU)
    k_cols_one_left(G.poisoned(inp, **kw), g.out("ucat_f", inp.shape, dtype, **kw))
    with pytest.raises(AssertionError, match=r"ucat_f: 1 element\(s\) written outside the view"):
        g.check({"ucat_f": want})
    g = G.Guards(CPU)
    k_next_utterance(G.poisoned(inp, **kw), g.out("ucat_f", inp.shape, dtype, **kw))
    with pytest.raises(AssertionError, match=r"ucat_f: 48 element\(s\) written outside the view"):
        g.check({"ucat_f": want})


@pytest.mark.parametrize("dtype", DTYPES)
def test_halo_read_across_the_utterance_end(dtype):
    inp = torch.randn(2, 5, 24).to(dtype)
    kw = dict(rows=G.TIME_TILE, left=G.LEFT, right=G.RIGHT)
    z = torch.nn.functional.pad(inp, (0, 0, 1, 1))
    want = z[:, :5] + z[:, 1:6] + z[:, 2:]
    # plain tensors hide the unclamped kernel's fault in the middle of a dense batch: it reads the neighbour's finite rows
    dense = torch.empty_like(inp)
    k_halo_sum(torch.cat([inp, inp, inp])[2:4], dense, clamp=False)
    assert bool(torch.isfinite(dense).all())
    g = G.Guards(CPU)
    k_halo_sum(G.poisoned(inp, **kw), g.out("conv_out", inp.shape, dtype, **kw), clamp=True)
    g.check({"conv_out": want})
    g = G.Guards(CPU)
    k_halo_sum(G.poisoned(inp, **kw), g.out("conv_out", inp.shape, dtype, **kw), clamp=False)
    with pytest.raises(AssertionError, match=r"conv_out: 96 of 240 element\(s\) not finite"):
        g.check({"conv_out": want})
    with pytest.raises(AssertionError, match=r"conv_out: 96 of 240 element\(s\) differ from the plain launch"):
        G.assert_same_bits(g.view("conv_out"), want, "conv_out")


def test_reference_near_the_sentinel_is_refused():
    with pytest.raises(AssertionError, match="ref_out: reference reaches"):
        G.assert_far_from_sentinel(torch.tensor([1.0, -40000.0]), "ref_out")
    with pytest.raises(AssertionError, match="ref_out: reference not finite"):
        G.assert_far_from_sentinel(torch.tensor([1.0, float("inf")]), "ref_out")
    G.assert_far_from_sentinel(torch.tensor([1.0, -300.0]), "ref_out")


# what the training kernels add: workspaces, the uint8 mask, 2-D column slices --------------------------------------------------
TILE = 4                                                                      # rows per "workgroup" of the fake column-sum kernels


def k_colsum(inp, ws, out, fold_extra=0, skip_last_store=False, ws_overrun=False):
    """out[c] = sum over rows of inp[:, c] as per-workgroup partial rows in ``ws`` + a fixed-order fold.  ``fold_extra``: the fold
    reads that many rows more than there are workgroups; ``skip_last_store``: the last workgroup exits without storing its row;
    ``ws_overrun``: one float is stored past the workspace."""
    r, d = inp.shape
    nwg = (r + TILE - 1) // TILE
    part = ws[:nwg * d].view(nwg, d)
    for w in range(nwg):
        if not (skip_last_store and w == nwg - 1):
            part[w] = inp[w * TILE:(w + 1) * TILE].float().sum(0)
    if ws_overrun:
        _reach(ws, (ws.numel() + 1,))[ws.numel()] = 1.0
    out.copy_(_reach(ws, ((nwg + fold_extra) * d,)).view(nwg + fold_extra, d).sum(0))


def _colsum_case(rows=9, d=8, ws_rows=None, **fault):
    """The two-step protocol on k_colsum: the plain launch on a workspace that a previous launch left full of correct partials (what
    the caching allocator hands back), the guarded one on a scratch."""
    inp = torch.randn(rows, d)
    nwg = (rows + TILE - 1) // TILE
    nws = (ws_rows or nwg) * d
    stale = torch.zeros(nws + d)                                              # rows the first run does not write are zero, not whatever the host allocator recycled
    k_colsum(inp, stale[:nws], torch.empty(d))                               # the "first run" of a run-twice determinism check
    stale[nws:] = 0.0

    def run(L):
        ws = L.scratch("workspace", nws, pad=2 * d) if L.guard else stale[:nws]
        k_colsum(L.rows(inp, rows=TILE), ws, L.out("dbias", (d,), torch.float32, rows=TILE), **fault)
    return run, inp


def test_scratch_geometry():
    buf, view, outside = G.scratch(24, torch.float32, CPU, pad=8)
    assert buf.numel() == 40 and view.numel() == 24 and view.data_ptr() % 16 == 0 and int(outside.sum()) == 16
    assert bool(torch.isnan(view).all()) and bool((buf[:8] == G.SENTINEL).all()) and bool((buf[32:] == G.SENTINEL).all())
    G.assert_untouched(buf, outside, "fresh")
    view.fill_(3.0)                                                          # the inside is the kernel's own
    G.assert_untouched(buf, outside, "written inside")


def test_fold_and_workspace_kernels():
    run, inp = _colsum_case()
    outs = G.two_step(run, CPU)
    folded = lambda t: torch.stack([t[:4].sum(0), t[4:8].sum(0), t[8:].sum(0)]).sum(0)
    assert torch.equal(outs["dbias"], folded(inp))
    # a fold that reads one partial row too many, in a workspace with room for it (cm_layernorm_bwd's holds 512 rows whatever the grid):
    # the stale row is zero in the plain launch, NaN in the scratch
    run, _ = _colsum_case(ws_rows=4, fold_extra=1)
    with pytest.raises(AssertionError, match=r"dbias: 8 of 8 element\(s\) not finite"):
        G.two_step(run, CPU)
    # ... and in a workspace of exactly the sizing function's rows: the row behind it is the sentinel band
    run, _ = _colsum_case(fold_extra=1)
    with pytest.raises(AssertionError, match=r"dbias: 8 of 8 element\(s\) differ from the plain launch"):
        G.two_step(run, CPU)
    # a workgroup that exits without storing: the recycled workspace of the plain launch still holds the previous launch's row
    run, inp = _colsum_case(skip_last_store=True)
    plain = G.Launch(False, CPU)
    run(plain)
    assert torch.equal(plain.outs["dbias"], folded(inp)), "the recycled workspace hides it"
    with pytest.raises(AssertionError, match=r"dbias: 8 of 8 element\(s\) not finite"):
        G.two_step(run, CPU)
    # a store one float past the workspace
    run, _ = _colsum_case(ws_overrun=True)
    with pytest.raises(AssertionError, match=r"workspace: 1 element\(s\) written outside the view"):
        G.two_step(run, CPU)


def k_mask(inp, mask, y, one_past=False):
    """y = inp where kept; the keep decisions go to ``mask`` as bytes.  ``one_past``: one byte more is stored."""
    keep = inp > 0
    mask.copy_(keep.to(torch.uint8))
    y.copy_(inp * keep)
    if one_past:
        _reach(mask, (mask.shape[0] + 1, mask.shape[1]))[mask.shape[0], 0] = 1


def test_integer_sentinel_and_mask_kernels():
    buf, view, outside = G.guarded((5, 8), torch.uint8, CPU, rows=16)
    assert bool((buf == G.INT_SENTINEL).all()) and G.INT_SENTINEL not in (0, 1) and int(outside.sum()) == 2 * 16 * 8
    G.assert_untouched(buf, outside, "fresh")
    inp = torch.randn(5, 8)

    def make(one_past):
        def run(L):
            k_mask(L.rows(inp, rows=16), L.out("mask", (5, 8), torch.uint8, rows=16), L.out("y", (5, 8), torch.float32, rows=16), one_past)
        return run
    outs = G.two_step(make(False), CPU)
    assert torch.equal(outs["mask"].bool(), inp > 0)
    faulty = G.Launch(True, CPU)
    make(True)(faulty)
    with pytest.raises(AssertionError, match=r"mask: 1 element\(s\) written outside the view"):
        faulty.g.check(outs)
    with pytest.raises(AssertionError, match="mask: reference holds the integer sentinel"):
        G.assert_far_from_sentinel(torch.tensor([0, 1, G.INT_SENTINEL], dtype=torch.uint8), "mask")
    g = G.Guards(CPU)
    g.out("mask", (5, 8), torch.uint8, rows=16).fill_(1)
    with pytest.raises(AssertionError, match=r"mask: \d+ of 40 element\(s\) differ from the plain launch"):
        g.check({"mask": (inp > 0).to(torch.uint8)})


def k_atb(a, b, out, extra_col=False, extra_row=False):
    """out = a^T b of (rows, m) / (rows, n) operands addressed through their row strides.  ``extra_col``: a's column m is read into
    out's last row; ``extra_row``: row ``rows`` of both operands is contracted as well."""
    r, m = a.shape
    k = r + 1 if extra_row else r
    aa, bb = _reach(a, (k, m + 1 if extra_col else m)).float(), _reach(b, (k, b.shape[1])).float()
    res = aa[:, :m].t() @ bb
    if extra_col:
        res[m - 1] += aa[:, m] @ bb
    out.copy_(res)


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_dim_column_slices(dtype):
    kw = dict(rows=G.ROW_TILE, left=G.LEFT, right=G.RIGHT)
    buf, view, outside = G.guarded((5, 24), dtype, CPU, **kw)
    assert buf.shape == (3, 5 + G.ROW_TILE, G.LEFT + 24 + G.RIGHT) and view.shape == (5, 24) and view.stride() == (48, 1)
    assert view.data_ptr() % 16 == 0 and int(outside.sum()) == buf.numel() - 5 * 24
    assert not bool(outside[1, :5, G.LEFT:G.LEFT + 24].any()) and bool(outside[0].all()) and bool(outside[2].all()) and bool(outside[1, 5:].all())
    a, b = torch.randn(5, 24).to(dtype), torch.randn(5, 16).to(dtype)
    pa = G.poisoned(a, **kw)
    assert torch.equal(pa, a) and pa.stride() == (48, 1)
    around = _reach(pa, (7, 26), -pa.stride(0) - 1).clone()                   # one row and one column on every side
    around[1:6, 1:25] = float("nan")
    assert bool(torch.isnan(around).all())

    def make(**fault):
        def run(L):
            k_atb(L.cols(a, rows=G.ROW_TILE), L.cols(b, rows=G.ROW_TILE), L.out("dw", (24, 16), torch.float32), **fault)
        return run
    outs = G.two_step(make(), CPU)
    assert torch.equal(outs["dw"], a.float().t() @ b.float())
    # in a dense slice of a wider activation the column beside it and the row behind a chunk are finite data: only the poisoned views show
    for fault, count in ((dict(extra_col=True), 16), (dict(extra_row=True), 384)):
        faulty = G.Launch(True, CPU)
        make(**fault)(faulty)
        with pytest.raises(AssertionError, match=rf"dw: {count} of 384 element\(s\) not finite"):
            faulty.g.check(outs)


# the operator route's (dim, batch, time) storage ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_geometry(dtype, shift):
    """(batch, dim, time) view of (dim, batch, time) storage: batch stride = one padded row, channel stride = a padded batch; guard
    columns in time, a guard utterance around every channel's batch, whole guard channels around the tensor.  ``shift`` moves the
    view off its 16-byte alignment, in the plain launch's tensor too."""
    b, d, l, rows = 2, 3, 8, 2
    lp = l + G.LEFT + G.RIGHT
    L = G.Launch(True, CPU)
    view = L.out("du", (b, d, l), dtype, transposed=True, rows=rows, shift=shift)
    buf, _, outside = L.g.items["du"]
    assert buf.shape == (rows + d + rows, b + 2, lp) and view.shape == (b, d, l) and view.stride() == (lp, (b + 2) * lp, 1)
    assert (view.data_ptr() % 16 == 0) == (shift == 0)
    inside = torch.zeros_like(outside)
    inside[rows:rows + d, 1:b + 1, G.LEFT + shift:G.LEFT + shift + l] = True
    assert torch.equal(outside, ~inside)
    t = torch.randn(b, d, l).to(dtype)
    p = L.chan(t, rows=rows, shift=shift)
    assert torch.equal(p, t) and p.stride() == view.stride() and p.storage_offset() == view.storage_offset()
    around = _reach(p, (b + 2, d + 2, l + 2), -p.stride(1) - p.stride(0) - 1).clone()   # one utterance, channel and step on every side
    around[1:b + 1, 1:d + 1, 1:l + 1] = float("nan")
    assert bool(torch.isnan(around).all())
    P = G.Launch(False, CPU)
    q, o = P.chan(t, rows=rows, shift=shift), P.out("du", (b, d, l), dtype, transposed=True, rows=rows, shift=shift)
    assert torch.equal(q, t) and q.stride() == (l, b * l, 1) == o.stride() and (q.data_ptr() % 16 == 0) == (shift == 0) == (o.data_ptr() % 16 == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_transposed_kernels(dtype):
    """In (dim, batch, time) storage the element behind a row's end is the NEXT UTTERANCE's first step of the same channel: a kernel
    that reads or writes one step too many is flagged; the correct one passes."""
    t = torch.randn(2, 3, 8).to(dtype)
    want = 2 * t

    def correct(inp, out):
        out.copy_(2 * inp)

    def one_step_past(inp, out):                       # every row one step longer, input and output
        b, d, l = inp.shape
        _reach(out, (b, d, l + 1)).copy_(2 * _reach(inp, (b, d, l + 1)))

    def reads_past(inp, out):                          # the last step takes the value behind the row's end
        b, d, l = inp.shape
        out.copy_(2 * inp)
        out[:, :, -1] += 0 * _reach(inp, (b, d, l + 1))[:, :, -1]

    L = G.Launch(True, CPU)
    correct(L.chan(t), L.out("ddelta", t.shape, dtype, transposed=True, rows=1))
    L.g.check({"ddelta": want})
    L = G.Launch(True, CPU)
    one_step_past(L.chan(t), L.out("ddelta", t.shape, dtype, transposed=True, rows=1))
    with pytest.raises(AssertionError, match=r"ddelta: 6 element\(s\) written outside the view"):
        L.g.check({"ddelta": want})
    L = G.Launch(True, CPU)
    reads_past(L.chan(t), L.out("ddelta", t.shape, dtype, transposed=True, rows=1))
    with pytest.raises(AssertionError, match=r"ddelta: 6 of 48 element\(s\) not finite"):
        L.g.check({"ddelta": want})


def test_fp16_outputs_take_a_sentinel_fp16_holds():
    buf, view, outside = G.guarded((2, 3, 8), torch.float16, CPU, rows=1, left=G.LEFT, right=G.RIGHT, transposed=True)
    assert G.sentinel_of(torch.float16) == G.F16_SENTINEL and bool((buf == G.F16_SENTINEL).all())
    G.assert_untouched(buf, outside, "fresh")
    G.assert_far_from_sentinel(torch.full((2,), 16000.0, dtype=torch.float16), "y")
    with pytest.raises(AssertionError, match="too near the sentinel"):
        G.assert_far_from_sentinel(torch.full((2,), 17000.0, dtype=torch.float16), "y")


# what the decoding kernels add: integer inputs (indices, lengths, labels) and outputs that hold -inf -----------------------------
def k_gather_sum(table, idx, out, extra=0):
    """out[r] = sum over j of table[idx[r, j]]: a kernel that addresses ``table`` through an index tensor.  ``extra``: the loop over a
    row's indices runs that many elements too far (the next row's, or what lies behind the tensor)."""
    r, k = idx.shape
    wide = _reach(idx, (r, k + extra))
    out.copy_(table[wide.long()].sum(1))


def test_integer_guard_catches_an_index_over_read():
    """NaN cannot stand in an index tensor.  Its guard elements hold a valid row that names a NaN line of the table: the over-read is
    an address inside the test's memory, and it shows in the result."""
    table = torch.randn(6, 8)
    table[5] = float("nan")                                                   # the line no index names
    idx = torch.randint(0, 5, (3, 4), generator=torch.Generator().manual_seed(0), dtype=torch.int32)
    p = G.int_poisoned(idx, 5, rows=2)
    assert torch.equal(p, idx) and p.is_contiguous() and p.dtype == torch.int32
    assert bool((_reach(p, (2, 4), -8) == 5).all()) and bool((_reach(p, (5, 4))[3:] == 5).all())   # 2 x 4 guard elements either side
    with pytest.raises(AssertionError, match="the guard value 3 occurs in the tensor"):
        G.int_poisoned(torch.tensor([1, 3], dtype=torch.int32), 3)
    dense = torch.empty(3, 8)
    k_gather_sum(table, torch.cat([idx, idx])[:3], dense, extra=1)            # in a dense batch the over-read meets valid indices
    assert bool(torch.isfinite(dense).all())

    def make(extra):
        def run(L):                                                           # (the plain tensor has nothing behind it to read)
            k_gather_sum(table, L.ints(idx, 5, rows=2), L.out("y", (3, 8), torch.float32, rows=4), extra if L.guard else 0)
        return run
    outs = G.two_step(make(0), CPU)
    assert torch.equal(outs["y"], table[idx.long()].sum(1))
    with pytest.raises(AssertionError, match=r"y: 8 of 24 element\(s\) not finite"):
        G.two_step(make(1), CPU)                                              # rows 0 and 1 read the next row's first index, row 2 the guard


def test_free_outputs_keep_the_plain_launch_minus_infinity():
    """An output that holds -inf by contract: the guarded view must hold the plain launch's bits, -inf included, be finite where the
    plain launch is, and NaN nowhere."""
    want = torch.tensor([[0.5, -math.inf], [-math.inf, 2.0]])
    with pytest.raises(AssertionError, match="score: reference not finite"):
        g = G.Guards(CPU)
        g.out("score", (2, 2), torch.float32, rows=4).copy_(want)
        g.check({"score": want})
    g = G.Guards(CPU)
    g.out("score", (2, 2), torch.float32, rows=4, free=True).copy_(want)
    g.check({"score": want})
    g = G.Guards(CPU)
    g.out("score", (2, 2), torch.float32, rows=4, free=True).copy_(torch.tensor([[0.5, -math.inf], [-math.inf, float("nan")]]))
    with pytest.raises(AssertionError, match=r"score: 1 of 2 element\(s\) not finite"):
        g.check({"score": want})
    g = G.Guards(CPU)
    g.out("score", (2, 2), torch.float32, rows=4, free=True).copy_(torch.tensor([[0.5, 1.0], [-math.inf, 2.0]]))
    with pytest.raises(AssertionError, match=r"score: 1 of 4 element\(s\) differ from the plain launch"):
        g.check({"score": want})
    token = torch.tensor([G.INT_SENTINEL, 3], dtype=torch.int32)             # a token id may equal the sentinel byte
    g = G.Guards(CPU)
    g.out("token", (2,), torch.int32, rows=4, free=True).copy_(token)
    g.check({"token": token})
