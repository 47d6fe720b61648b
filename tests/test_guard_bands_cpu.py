"""tests/guard_bands.py catches what it is for: fake "kernels" written in torch on CPU tensors -- one that writes a row past its view,
one that writes a column to the left, one that writes the first row behind an utterance, one that folds a row from outside its input
view into a row sum -- are each flagged with the tensor's name, and a correct one passes.  The GPU tests
(tests/test_forward_guards_gpu.py) make the same calls on real kernels; this file is why they are not vacuous."""
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
