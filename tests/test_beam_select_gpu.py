"""ops.beam_select (csrc/beam_select.hip) against the contract restated in torch (tests/s2s_beam_ref.select) on the
same device tensors.  The contract fixes every bit: the three fp32 operations are the same, and the order is total, so score,
parent and token are compared with torch.equal, and inc wherever the score is finite (a -inf slot's inc is not specified).

Shapes (U, B, V): the smallest; a single beam; V < B; small and odd everywhere; the recipes' beam 66 on two 64-lane tiles plus 37;
the largest beam; and once the recipes' own 66 x 5000.  MULTI: more than one chunk of CM_BEAM_SELECT_CHUNK = 5120 tokens per row -- a last chunk of
one token (K = 1 < B, the rest of its list zero-filled), a last chunk of exactly B tokens, three chunks."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2s_beam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NEG = -math.inf
SHAPES = [(1, 1, 1), (3, 1, 37), (2, 8, 5), (3, 5, 37), (2, 66, 165), (1, 128, 300)]
BOTH = [(3, 5, 37), (2, 66, 165)]
MULTI = [(2, 3, 5121), (1, 128, 5248), (2, 8, 10241)]


def _check(att, alive, B, eos, **kw):
    from mamba_asr_amd import ops
    got = ops.beam_select(att, alive, B, eos, **kw)
    want = R.select(att, alive, B, eos, **kw)
    torch.cuda.synchronize()
    U = att.shape[0] // B
    for g, w, dtype in zip(got, want, (torch.float32, torch.float32, torch.int32, torch.int32)):
        assert g.shape == (U, B) and g.dtype == dtype and w.dtype == dtype
    score, inc, parent, token = got
    assert not torch.isnan(score).any()
    assert torch.equal(score, want[0]), "score"
    assert torch.equal(parent, want[2]) and torch.equal(token, want[3]), "parent / token"
    assert bool(((parent >= 0) & (parent < B) & (token >= 0) & (token < att.shape[1])).all())
    fin = torch.isfinite(score)
    assert torch.equal(inc[fin], want[1][fin]), "inc"
    return got


def _inputs(U, B, V, seed):
    g = torch.Generator().manual_seed(seed)
    att = torch.log_softmax(torch.randn(U * B, V, generator=g) * 3.0, dim=-1)
    alive = -torch.rand(U * B, generator=g) * 20.0
    delta = -torch.rand(U * B, V, generator=g) * 30.0
    return att.to(DEV), alive.to(DEV), delta.to(DEV)


def _eos(V):
    return 2 if V > 2 else 0


@pytest.mark.parametrize("shape", SHAPES + MULTI)
def test_random_scores(shape):
    U, B, V = shape
    att, alive, delta = _inputs(U, B, V, 1)
    _check(att, alive, B, _eos(V))
    _check(att, alive, B, _eos(V), delta=delta, weight=0.4)


def test_the_recipe_shape_once():
    U, B, V = 2, 66, 5000
    att, alive, delta = _inputs(U, B, V, 2)
    delta[:, 0] = NEG
    blocked = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    _check(att, alive, B, 2, delta=delta, weight=0.4, eos_blocked=blocked)


@pytest.mark.parametrize("shape", BOTH + MULTI)
def test_masses_of_ties(shape):
    U, B, V = shape
    att, alive, delta = _inputs(U, B, V, 3)
    q = lambda x: torch.round(x * 4.0) / 4.0
    _check(q(att), q(alive), B, _eos(V))
    _check(q(att), q(alive), B, _eos(V), delta=q(delta), weight=0.5)


@pytest.mark.parametrize("shape", BOTH + [(2, 8, 5), (1, 128, 300)] + MULTI)
def test_all_equal_scores_give_the_first_flat_indices(shape):
    """MULTI: every chunk of every row hands the merge equal scores; the first B flat indices k * V + c win across chunk boundaries."""
    U, B, V = shape
    att, alive = torch.full((U * B, V), -1.5, device=DEV), torch.full((U * B,), -2.0, device=DEV)
    score, inc, parent, token = _check(att, alive, B, _eos(V))
    flat = torch.arange(B, device=DEV).expand(U, B)
    assert torch.equal(parent.long(), flat // V) and torch.equal(token.long(), flat % V)
    assert bool((score == -3.5).all()) and bool((inc == -1.5).all())


@pytest.mark.parametrize("shape", BOTH)
def test_first_step_and_dead_utterance(shape):
    U, B, V = shape
    att, alive, delta = _inputs(U, B, V, 4)
    first = torch.full((U, B), NEG, device=DEV)
    first[:, 0] = 0.0
    score, _, parent, _ = _check(att, first.reshape(-1), B, _eos(V), delta=delta, weight=0.4)
    assert bool((parent[:, :min(B, V)] == 0).all())
    dead = alive.clone().view(U, B)
    dead[-1] = NEG                                                               # one utterance without a live slot
    score, _, parent, token = _check(att, dead.reshape(-1), B, _eos(V))
    flat = torch.arange(B, device=DEV)
    assert bool((score[-1] == NEG).all()) and torch.equal(parent[-1].long(), flat // V) and torch.equal(token[-1].long(), flat % V)


@pytest.mark.parametrize("shape", BOTH)
def test_scattered_inf_zero_and_nan(shape):
    U, B, V = shape
    att, alive, delta = _inputs(U, B, V, 5)
    g = torch.Generator().manual_seed(6)
    kind = torch.randint(0, 12, att.shape, generator=g).to(DEV)
    att = torch.where(kind == 0, torch.full_like(att, NEG), att)
    att = torch.where(kind == 1, torch.zeros_like(att), att)
    att = torch.where(kind == 2, -torch.zeros_like(att), att)
    att = torch.where(kind == 3, torch.full_like(att, math.nan), att)
    alive = alive.clone()
    alive[::3] = 0.0                                                             # 0 + (+0 / -0): the zeros tie
    alive[1::7] = NEG
    _check(att, alive, B, _eos(V))
    delta[:, 1::5] = NEG
    _check(att, alive, B, _eos(V), delta=delta, weight=0.4)
    _check(att, alive, B, _eos(V), delta=delta, weight=0.0)                      # 0 * -inf: NaN ranks as -inf


@pytest.mark.parametrize("shape", BOTH)
def test_eos_blocked_per_utterance(shape):
    U, B, V = shape
    att, alive, delta = _inputs(U, B, V, 7)
    eos = _eos(V)
    att[:, eos] = 0.0                                                            # <eos> would win every row
    blocked = torch.tensor([1, 0, 1][:U], dtype=torch.int32, device=DEV)
    for kw in (dict(), dict(delta=delta, weight=0.4)):
        _, _, _, token = _check(att, alive, B, eos, eos_blocked=blocked, **kw)
        assert not bool((token[0] == eos).any()) and bool((token[1] == eos).any())
    _check(att, alive, B, V + 3, eos_blocked=blocked)                            # an eos outside [0, V) never matches
    _check(att, alive, B, -1, eos_blocked=blocked)


def test_two_calls_give_the_same_bits_and_utterances_do_not_mix():
    from mamba_asr_amd import ops
    U, B, V = 3, 66, 165
    att, alive, delta = _inputs(U, B, V, 8)
    att = torch.round(att * 2.0) / 2.0                                           # ties, so that an order-dependent path would show
    a = ops.beam_select(att, alive, B, 2, delta=delta, weight=0.4)
    b = ops.beam_select(att, alive, B, 2, delta=delta, weight=0.4)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    rows = slice(B, 2 * B)
    alone = ops.beam_select(att[rows].contiguous(), alive[rows].contiguous(), B, 2, delta=delta[rows].contiguous(), weight=0.4)
    for x, y in zip(a, alone):
        assert torch.equal(x[1:2].view(torch.int32), y.view(torch.int32))


def test_bad_arguments_raise_without_a_launch():
    from mamba_asr_amd import ops
    att, alive, _ = _inputs(2, 4, 37, 9)
    with pytest.raises(RuntimeError, match="B must be"):
        ops.beam_select(att, alive, 0, 2)
    with pytest.raises(RuntimeError, match="B must be"):
        ops.beam_select(att, alive, 129, 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.beam_select(att.t().contiguous().t(), alive, 4, 2)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.beam_select(att, alive, 3, 2)                                        # 8 rows are no multiple of 3
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.beam_select(att.cpu(), alive.cpu(), 4, 2)
    with pytest.raises(RuntimeError, match="alive"):
        ops.beam_select(att, alive.double(), 4, 2)
    with pytest.raises(RuntimeError, match="eos_blocked"):
        ops.beam_select(att, alive, 4, 2, eos_blocked=torch.zeros(2, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
