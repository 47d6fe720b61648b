"""Guard bands inside ONE allocation, for kernels that no address sanitizer watches: an output is a view of a sentinel-filled buffer,
an input a view of a NaN-filled one.  A store outside the output view turns a sentinel into something else (assert_untouched), a load
from outside an input view that reaches a result turns it into NaN, so the result no longer has the bits of the plain launch
(assert_same_bits) and is not finite (assert_finite).  Every check stays inside memory the test allocated: the guards are at least
one workgroup tile of the kernel under test, so a whole-tile overrun still lands in them.

Geometry.  A 3-D (batch, seqlen, width) view of a (batch + 2, seqlen + rows, left + width + right) buffer: ``left`` / ``right`` guard
columns beside every row, ``rows`` guard rows behind every utterance, one whole guard utterance in front of the batch and one behind.
A 2-D (rows, width) tensor given guard columns (left or right > 0) is a column slice of a wider matrix: the same geometry with batch 1,
indexed [0] -- ``rows`` guard rows behind, a whole guard block in front and behind, guard columns beside every row.
transposed=True: the operator route's production layout -- a 3-D (batch, dim, time) view of (dim, batch, time) storage, buffer
(rows + dim + rows, batch + 2, left + time + right): the view's batch stride is one padded row and its channel stride a whole padded
batch, ``left`` / ``right`` guard columns lie in time beside every row, a whole guard utterance stands in front of and behind every
channel's batch, and ``rows`` whole guard channels stand in front of and behind the tensor.
Everything else (2-D (rows, D) tensors the kernels want contiguous; 3-D with contiguous=True; any other rank) stays contiguous: a flat
buffer with ``rows`` x shape[-1] guard elements in front and behind.

Integer outputs (the uint8 dropout mask) take INT_SENTINEL: -65536 does not exist in uint8, and the byte is neither 0 nor 1.
A workspace (Guards.scratch) is NaN inside and sentinel outside: nothing outside may be written, and a partial row that a fold reads
although no workgroup wrote it brings NaN into a result, where assert_finite / assert_same_bits report it -- a recycled
allocation would still hold the previous launch's correct partials there.

Integer inputs (int_poisoned; indices, lengths, labels) have no NaN: their guard elements hold a value the CASE chooses -- one that
is valid as an address (a row, class or frame the test allocated) yet names poison (a NaN cache line, a class absent from every
target), so that a kernel that reads the guard shows it in its result and never leaves the test's memory.
Outputs that legitimately hold -inf, or integers that may equal the sentinel byte (free=True): the plain launch's non-finite pattern is
part of its bits -- the guarded view must hold the same bits (NaN equals nothing), finite where the plain launch is.

Launch / two_step: the two-launch protocol the GPU files share (plain tensors, then poisoned inputs / guarded outputs).

Plain module (as tests/ctc_beam_ref.py), any torch.device.
"""
import math

import torch

SENTINEL = -65536.0            # exact in bf16 (-2^16); the cases' results stay far from it (assert_far_from_sentinel on the reference)
F16_SENTINEL = -32768.0        # fp16 ends at 65504: its outputs (the causal conv's) take -2^15
INT_SENTINEL = 0xA5            # integer outputs (a stored keep mask holds 0 / 1 only)
ROW_TILE = 64                  # rows per workgroup of the row kernels (cm_ffn_fused, cm_ln_pw_glu, cm_gemm_bf16, cm_add_layernorm)
TIME_TILE = 32                 # time steps per workgroup of the time-tiled kernels (conv_xproj, scan, dwconv rows)
LEFT, RIGHT = 8, 16            # guard columns: 16 / 32 bytes in bf16, 32 / 64 in fp32 -- views stay 16-byte aligned


def _geometry(shape, rows, left, right, contiguous, transposed=False):
    """-> (buffer shape, function buffer -> view)."""
    shape = tuple(int(s) for s in shape)
    assert len(shape) >= 1 and all(s > 0 for s in shape) and rows >= 0 and left >= 0 and right >= 0, (shape, rows, left, right)
    if transposed:
        assert len(shape) == 3 and not contiguous, "transposed: a (batch, dim, time) view of (dim, batch, time) storage"
        b, d, l = shape
        return (rows + d + rows, b + 2, left + l + right), lambda buf: buf[rows:rows + d, 1:b + 1, left:left + l].transpose(0, 1)
    if len(shape) == 3 and not contiguous:
        b, l, w = shape
        return (b + 2, l + rows, left + w + right), lambda buf: buf[1:b + 1, :l, left:left + w]
    if len(shape) == 2 and not contiguous and (left or right):
        l, w = shape
        return (3, l + rows, left + w + right), lambda buf: buf[1:2, :l, left:left + w][0]
    assert left == 0 and right == 0, "a contiguous view has no room for guard columns"
    n, pad = math.prod(shape), rows * shape[-1]
    return (pad + n + pad,), lambda buf: buf[pad:pad + n].view(shape)


def sentinel_of(dtype):
    if dtype == torch.float16:
        return F16_SENTINEL
    return SENTINEL if dtype.is_floating_point else INT_SENTINEL


def guarded(shape, dtype, device, rows=ROW_TILE, left=0, right=0, contiguous=False, align=16, transposed=False):
    """-> (sentinel-filled buffer, its view of ``shape``, bool mask of the buffer's elements outside the view).  ``align``: the byte
    alignment the view's start must keep (16: what the vector loads of most kernels need; odd widths keep less)."""
    bshape, view_of = _geometry(shape, rows, left, right, contiguous, transposed)
    buf = torch.full(bshape, sentinel_of(dtype), dtype=dtype, device=device)
    assert float(buf.reshape(-1)[0]) == sentinel_of(dtype), f"{sentinel_of(dtype)} is not exact in {dtype}"
    outside = torch.ones(bshape, dtype=torch.bool, device=device)
    view_of(outside).fill_(False)
    view = view_of(buf)
    assert int(outside.sum()) == buf.numel() - view.numel() and view.data_ptr() % align == 0
    return buf, view, outside


def poisoned(t, rows=ROW_TILE, left=0, right=0, contiguous=False, align=16, transposed=False):
    """t's values in a view of guarded()'s geometry inside a NaN-filled buffer."""
    assert t.is_floating_point()
    bshape, view_of = _geometry(t.shape, rows, left, right, contiguous, transposed)
    buf = torch.full(bshape, float("nan"), dtype=t.dtype, device=t.device)
    view = view_of(buf)
    view.copy_(t)
    assert view.data_ptr() % align == 0
    return view


def int_poisoned(t, guard, rows=ROW_TILE, unique=True):
    """The integer tensor t (contiguous, any rank) with ``rows`` x its last axis elements of ``guard`` in front and behind: ``guard`` is
    the case's choice of a value that is safe to use as an index and visible in the result when used.  unique=False: the value range
    is too small for a guard that occurs nowhere in t (one row, two utterances); the guard still names poison."""
    assert not t.is_floating_point() and not t.is_complex() and t.dim() >= 1 and t.numel() > 0 and rows > 0, (t.dtype, tuple(t.shape), rows)
    assert not unique or not bool((t == guard).any()), f"the guard value {guard} occurs in the tensor: a read of the guard would not show"
    n, pad = t.numel(), rows * t.shape[-1]
    buf = torch.full((pad + n + pad,), guard, dtype=t.dtype, device=t.device)
    view = buf[pad:pad + n].view(t.shape)
    view.copy_(t)
    return view


def scratch(numel, dtype, device, pad=4096):
    """A workspace of ``numel`` elements: NaN inside, ``pad`` sentinel elements in front and behind (at least one partial row of the
    kernel under test).  -> (buffer, view, outside mask) as guarded()."""
    assert dtype.is_floating_point and numel > 0 and pad > 0 and (pad * dtype.itemsize) % 16 == 0, (numel, dtype, pad)
    buf = torch.full((pad + numel + pad,), SENTINEL, dtype=dtype, device=device)
    outside = torch.ones(buf.shape, dtype=torch.bool, device=device)
    outside[pad:pad + numel] = False
    view = buf[pad:pad + numel]
    view.fill_(float("nan"))
    assert view.data_ptr() % 16 == 0
    return buf, view, outside


def assert_untouched(buffer, outside_mask, name):
    """Every element outside the view still holds the sentinel (of the buffer's dtype)."""
    hit = (buffer != sentinel_of(buffer.dtype)) & outside_mask
    if bool(hit.any()):
        idx = hit.nonzero()
        first = tuple(int(i) for i in idx[0])
        raise AssertionError(f"{name}: {idx.shape[0]} element(s) written outside the view; first at buffer index {first} "
                             f"(buffer shape {tuple(buffer.shape)}): {float(buffer[first])!r}")


def assert_finite(t, name):
    bad = ~torch.isfinite(t)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {t.numel()} element(s) not finite: memory outside an input view reached the result"


def assert_same_bits(got, want, name):
    """The guarded launch's output against the plain launch's: shape, dtype and every bit (NaN equals nothing)."""
    assert got.shape == want.shape and got.dtype == want.dtype, f"{name}: {tuple(got.shape)} {got.dtype} vs {tuple(want.shape)} {want.dtype}"
    if not torch.equal(got, want):
        diff = ~(got == want)
        first = tuple(int(i) for i in diff.nonzero()[0])
        raise AssertionError(f"{name}: {int(diff.sum())} of {got.numel()} element(s) differ from the plain launch; first at {first}: "
                             f"{float(got[first])!r} vs {float(want[first])!r}")


def assert_far_from_sentinel(ref, name):
    """The case's reference output is finite and below half the sentinel's magnitude: a result cannot pass for an untouched guard.
    An integer output never holds the sentinel byte."""
    if not ref.dtype.is_floating_point:
        assert not bool((ref == INT_SENTINEL).any()), f"{name}: reference holds the integer sentinel {INT_SENTINEL:#x}"
        return
    r = ref.detach().double()
    assert bool(torch.isfinite(r).all()), f"{name}: reference not finite"
    s = sentinel_of(ref.dtype)
    assert float(r.abs().max()) < 0.5 * abs(s), f"{name}: reference reaches {float(r.abs().max()):.3e}, too near the sentinel {s}"


class Guards:
    """The guarded outputs of one launch: ``view = g.out(name, shape, dtype, ...)`` per output, ``g.scratch(name, numel, dtype)`` per
    workspace, then ``g.check({name: plain result})``: the plain launch's outputs are far from the sentinel and finite; the guarded
    views hold their bits; nothing outside an output or a workspace is written (a workspace's content is the kernel's own)."""

    def __init__(self, device):
        self.device, self.items, self.scratches, self.free = device, {}, set(), set()

    def scratch(self, name, numel, dtype, pad=4096):
        assert name not in self.items, name
        self.items[name] = scratch(numel, dtype, self.device, pad)
        self.scratches.add(name)
        return self.items[name][1]

    def out(self, name, shape, dtype, free=False, **kw):
        """free: the output may hold -inf (or, an integer one, the sentinel byte's value) in the plain launch."""
        assert name not in self.items, name
        self.items[name] = guarded(shape, dtype, self.device, **kw)
        if free:
            self.free.add(name)
        return self.items[name][1]

    def view(self, name):
        return self.items[name][1]

    def check(self, plain):
        assert set(plain) == set(self.items) - self.scratches, (sorted(plain), sorted(self.items), sorted(self.scratches))
        for name in sorted(self.scratches):
            assert_untouched(self.items[name][0], self.items[name][2], name)
        for name, want in plain.items():
            buf, view, outside = self.items[name]
            assert_untouched(buf, outside, name)
            if name in self.free:
                if view.dtype.is_floating_point:
                    assert not bool(torch.isnan(want).any()), f"{name}: the plain launch holds NaN"
                    fin = torch.isfinite(want)
                    if bool(fin.any()):
                        assert_far_from_sentinel(want[fin], name)
                    assert_finite(view[fin], name)
            else:
                assert_far_from_sentinel(want, name)
                if view.dtype.is_floating_point:
                    assert_finite(view, name)
            assert_same_bits(view, want, name)


class Launch:
    """The tensors of one launch on ``device``: plain (guard=False) or poisoned inputs / guarded outputs / scratch workspaces
    (guard=True)."""

    def __init__(self, guard, device):
        self.guard, self.device, self.g, self.outs = guard, device, (Guards(device) if guard else None), {}

    def vec(self, t):
        """A small contiguous parameter tensor (bias, LayerNorm weight, A, taps) with 4 x its last axis of NaN in front and behind."""
        return None if t is None else (poisoned(t, rows=4) if self.guard else t)

    def rows(self, t, rows=ROW_TILE):
        """A contiguous (rows, D) tensor with ``rows`` NaN rows in front and behind."""
        return None if t is None else (poisoned(t, rows=rows) if self.guard else t.clone())

    def flat(self, t, rows):
        """A contiguous input of any rank with ``rows`` x its last axis of NaN in front and behind."""
        return None if t is None else (poisoned(t, rows=rows, contiguous=True) if self.guard else t.clone())

    def cols(self, t, dead=None, align=16, rows=TIME_TILE, left=LEFT, right=RIGHT):
        """A (batch, seqlen, width) or (rows, width) input inside NaN columns / rows / utterances; ``dead``: a column range the kernel
        must not read."""
        v = poisoned(t, align=align, rows=rows, left=left, right=right) if self.guard else t.clone()
        if dead is not None and self.guard:
            v[..., dead[0]:dead[1]] = float("nan")
        return v

    @staticmethod
    def _chan_align(l, itemsize, shift):
        """Rows of l + LEFT + RIGHT elements start 16-byte aligned only when that is whole 16-byte vectors and nothing shifts them."""
        return 16 if shift == 0 and ((l + LEFT + RIGHT) * itemsize) % 16 == 0 else itemsize

    def _plain_chan(self, shape, dtype, shift):
        b, d, l = shape
        flat = torch.zeros((d * b * l + shift,), dtype=dtype, device=self.device)
        return flat[shift:].view(d, b, l).transpose(0, 1)

    def chan(self, t, rows=1, shift=0):
        """A (batch, dim, time) input as a view of (dim, batch, time) storage inside NaN time columns / utterances / ``rows`` channels;
        plain: the same layout without the guards.  ``shift`` elements move the view off its 16-byte alignment in both."""
        if t is None:
            return None
        if self.guard:
            return poisoned(t, rows=rows, left=LEFT + shift, right=RIGHT - shift, align=self._chan_align(t.shape[-1], t.element_size(), shift), transposed=True)
        v = self._plain_chan(t.shape, t.dtype, shift)
        v.copy_(t)
        return v

    def ints(self, t, guard, rows=ROW_TILE, unique=True):
        """A contiguous integer input with ``rows`` x its last axis elements of ``guard`` in front and behind (int_poisoned)."""
        return None if t is None else (int_poisoned(t, guard, rows=rows, unique=unique) if self.guard else t.clone())

    def around(self, t, rows=1):
        """A contiguous input of any rank and any alignment with ``rows`` x its last axis of NaN in front and behind (a kernel that
        needs more alignment than the element's says so itself)."""
        return None if t is None else (poisoned(t, rows=rows, contiguous=True, align=t.element_size()) if self.guard else t.clone())

    def out(self, name, shape, dtype, fill=None, **kw):
        """An output: zeros (plain) or a sentinel-guarded view; ``fill``: initial content of both (an aliased input, or 0 where the
        kernel need not write every element)."""
        shift = kw.pop("shift", 0)                    # transposed outputs only: as chan()
        if kw.get("transposed"):
            kw.update(left=LEFT + shift, right=RIGHT - shift, align=self._chan_align(shape[-1], torch.empty((), dtype=dtype).element_size(), shift))
        free = kw.pop("free", False)
        if self.guard:
            t = self.g.out(name, shape, dtype, free=free, **kw)
        elif kw.get("transposed"):
            t = self._plain_chan(shape, dtype, shift)
        else:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
        if fill is not None:
            t.copy_(fill) if torch.is_tensor(fill) else t.fill_(fill)
        self.outs[name] = t
        return t

    def scratch(self, name, numel, dtype=torch.float32, pad=4096):
        """A workspace: uninitialised (plain) or NaN inside sentinels."""
        return self.g.scratch(name, numel, dtype, pad) if self.guard else torch.empty((numel,), dtype=dtype, device=self.device)


def two_step(run, device):
    """run(Launch) launches the kernel on the Launch's tensors.  -> the plain launch's outputs by name."""
    plain, guard = Launch(False, device), Launch(True, device)
    run(plain)
    run(guard)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    guard.g.check(plain.outs)
    return plain.outs
