"""The host restatement of the dropout stream (oracle.conmamba_oracle.drop_keep, a restatement of csrc/cm_dropout.h) on the CPU:
its threshold / scale / seed arithmetic, and the statistics of the keep decisions it draws -- keep rate overall, per column and per
row within binomial bounds; no measurable correlation between the two halves of a word, adjacent groups, two seeds, or one
site's masks at consecutive graph-replay epochs.  The GPU kernels are checked against this restatement in
tests/test_dropout_stream.py."""
import numpy as np
import pytest

from oracle import conmamba_oracle as O

ROWS, DIM = 65536, 256


def test_threshold_scale_and_seed_arithmetic():
    assert O.drop_thresh(0.0) == 0 and O.drop_thresh(-1.0) == 0
    assert O.drop_thresh(0.1) == round(0.1 * 65536) == 6554
    assert O.drop_thresh(0.5) == 32768
    assert O.drop_thresh(0.9999) == 65529
    assert O.drop_thresh(0.99999) == 65535 and O.drop_thresh(1.0) == 65535      # the cap: one in 65536 survives
    assert O.drop_scale(0.1) == pytest.approx(1.0 / (1.0 - 6554 / 65536.0), rel=1e-7)
    assert O.drop_scale(0.0) == 1.0
    # the epoch offset is modulo 2^64
    assert O.drop_seed(5, 0) == 5
    assert O.drop_seed(2 ** 64 - 1, 1) == (2 ** 64 - 1 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert O.drop_seed(7, 2 ** 40 + 3) == (7 + (2 ** 40 + 3) * 0x9E3779B97F4A7C15) % 2 ** 64


def _mix32_scalar(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_vectorised_words_match_a_scalar_restatement():
    """drop_words (numpy, wrapping uint32) against plain Python integers, at seeds and groups with high halves set."""
    for seed in (0, 1, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1):
        groups = np.array([0, 1, 7, 2 ** 31 + 5, 2 ** 32 + 9, 2 ** 40 + 123], dtype=np.uint64)
        w = O.drop_words(seed, groups)
        for gi, g in enumerate(groups.tolist()):
            base = (_mix32_scalar((g & 0xFFFFFFFF) ^ (seed & 0xFFFFFFFF)) + ((g >> 32) * 0x85EBCA6B) + (seed >> 32)) & 0xFFFFFFFF
            for j in range(4):
                assert int(w[gi, j]) == _mix32_scalar((base + j * 0x9E3779B9) & 0xFFFFFFFF), (seed, g, j)


def test_offset_and_shape_are_views_of_one_stream():
    k_all, _ = O.drop_keep(99, (40, 24), 0.3)
    k_off, _ = O.drop_keep(99, (13,), 0.3, offset=5 * 24 + 3)
    assert np.array_equal(k_off, k_all.reshape(-1)[123:136])
    assert np.array_equal(O.drop_keep(99, (960,), 0.3)[0], k_all.reshape(-1))


def _zmax(counts, n, q):
    return float(np.max(np.abs(counts - n * q)) / np.sqrt(n * q * (1 - q)))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate_overall_per_column_per_row(p):
    keep, _ = O.drop_keep(0x1234_5678_9ABC_DEF0, (ROWS, DIM), p)
    q = 1.0 - O.drop_thresh(p) / 65536.0
    n = ROWS * DIM
    assert _zmax(np.array([keep.sum()]), n, q) < 5.0
    assert _zmax(keep.sum(0), ROWS, q) < 5.0                                    # 256 columns
    rows = keep.sum(1)
    assert _zmax(rows, DIM, q) < 6.5                                            # 65536 rows
    # the spread of the per-row counts is the binomial one (a correlation inside a row would widen or narrow it)
    assert rows.var() == pytest.approx(DIM * q * (1 - q), rel=0.03)


def _corr(a, b):
    a, b = a.astype(np.float64).ravel(), b.astype(np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / np.sqrt((a * a).sum() * (b * b).sum()))


def test_no_measurable_correlation():
    p = 0.1
    seed = 0x0F1E_2D3C_4B5A_6978
    keep, _ = O.drop_keep(seed, (ROWS, DIM), p)
    flat = keep.reshape(-1, 8)                                                  # groups
    bound = lambda n: 5.0 / np.sqrt(n)
    # the two 16-bit halves of one word: elements 2j and 2j + 1 of a group
    lo, hi = flat[:, 0::2], flat[:, 1::2]
    assert abs(_corr(lo, hi)) < bound(lo.size)
    # words of one group: word j and word j + 1
    assert abs(_corr(flat[:, 0:6:2], flat[:, 2:8:2])) < bound(flat[:, 0:6:2].size)
    # adjacent groups: element k of group g and element k of group g + 1
    assert abs(_corr(flat[:-1], flat[1:])) < bound(flat[:-1].size)
    # the two dropouts of one FFN (two seeds, same shape)
    keep2, _ = O.drop_keep(seed + 1, (ROWS, DIM), p)
    assert abs(_corr(keep, keep2)) < bound(keep.size)
    # one site at consecutive graph-replay epochs, and at epochs 0 and 2^40 + 3
    for e0, e1 in ((0, 1), (1, 2), (0, 2 ** 40 + 3)):
        a, _ = O.drop_keep(seed, (ROWS, DIM), p, epoch=e0)
        b, _ = O.drop_keep(seed, (ROWS, DIM), p, epoch=e1)
        assert abs(_corr(a, b)) < bound(a.size), (e0, e1)
    # and the raw 16-bit values are uniform: the keep rate tracks the threshold at other p
    for p_ in (0.05, 0.9):
        k, _ = O.drop_keep(seed, (ROWS // 4, DIM), p_)
        q = 1.0 - O.drop_thresh(p_) / 65536.0
        assert _zmax(np.array([k.sum()]), k.size, q) < 5.0
