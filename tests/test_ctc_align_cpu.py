"""CTC forced alignment without a GPU: the NumPy reference (tests/ctc_align_ref.py) against brute-force enumeration of every path,
the pure word grouping, the C ABI's declarations, workspace bound and host-side refusals, and the CPU-tensor refusals."""
import ctypes as C
import itertools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_align_ref as AR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------
# the reference against brute force
# ----------------------------------------------------------------------------------------------------------
def _collapse(path, blank):
    out, prev = [], None
    for v in path:
        if v != prev and v != blank:
            out.append(v)
        prev = v
    return out


def _brute(lp, target, blank):
    """The best score over all V^n frame labellings that collapse to the target, summed left to right in float64; None if there is
    none."""
    n, V = lp.shape
    best = None
    for path in itertools.product(range(V), repeat=n):
        if _collapse(path, blank) != list(target):
            continue
        acc = lp[0, path[0]]
        for t in range(1, n):
            acc = acc + lp[t, path[t]]
        if acc > -np.inf and (best is None or acc > best):
            best = acc
    return best


def test_reference_matches_brute_force():
    rng = np.random.default_rng(20240607)
    seen = {0: 0, 1: 0}
    for case in range(300):
        V, n, L = int(rng.integers(1, 4)), int(rng.integers(0, 7)), int(rng.integers(0, 4))
        blank = int(rng.integers(0, V))
        labels = [v for v in range(V) if v != blank]
        target = [labels[int(x)] for x in rng.integers(0, len(labels), size=L)] if labels else []
        L = len(target)
        lp = np.log(rng.dirichlet(np.ones(V), size=n)).reshape(n, V)
        if case % 3 == 0:
            lp = np.round(lp)                                  # exact ties abound
        if case % 5 == 0 and n:
            lp[rng.integers(0, n), rng.integers(0, V)] = -np.inf
        status, score, states, starts, ends, logp = AR.align_one(lp, target, blank)
        want = _brute(lp, target, blank) if n else (0.0 if L == 0 else None)
        seen[status] += 1
        if want is None:
            assert status == 1 and score == -np.inf, (case, status, score)
            continue
        assert status == 0, (case, status, want)
        assert score == want, (case, score, want)                 # the same left fold along the same path: equal, not close
        E = 2 * L + 1
        assert states.shape == (n,)
        if n:
            assert states[0] in (0, 1) and states[-1] in (E - 1, E - 2) and states.min() >= 0
            d = np.diff(states)
            assert ((d >= 0) & (d <= 2)).all(), (case, states)
            e = [blank if s % 2 == 0 else target[s // 2] for s in states]
            assert _collapse(e, blank) == target
            total = lp[0, e[0]]
            for t in range(1, n):
                total = total + lp[t, e[t]]
            assert total == score
        for j in range(L):
            assert 0 <= starts[j] < ends[j] <= n and (states[starts[j]:ends[j]] == 2 * j + 1).all()
            assert (states == 2 * j + 1).sum() == ends[j] - starts[j]                      # every label visited, contiguously
            fold = lp[starts[j], target[j]]
            for t in range(starts[j] + 1, ends[j]):
                fold = fold + lp[t, target[j]]
            assert logp[j] == fold
    assert seen[0] > 50 and seen[1] > 50, seen


def test_reference_nan_and_ties():
    lp = np.log(np.full((4, 3), 1 / 3))
    status, score, states, starts, ends, _ = AR.align_one(lp, [1], 0)
    assert status == 0 and states.tolist() == [1, 2, 2, 2]          # ties keep the smaller move and the last state: the label as early as possible
    assert (starts.tolist(), ends.tolist()) == ([0], [1])
    bad = lp.copy()
    bad[2, 2] = np.nan                                               # a column outside {blank} + targets
    assert AR.align_one(bad, [1], 0)[0] == 0
    bad[2, 1] = np.nan
    st = AR.align_one(bad, [1], 0)
    assert st[0] == 2 and math.isnan(st[1])
    assert AR.align_one(lp[:2], [1, 1], 0)[0] == 1 and AR.align_one(lp[:3], [1, 1], 0)[2].tolist() == [1, 2, 3]


# ----------------------------------------------------------------------------------------------------------
# word grouping
# ----------------------------------------------------------------------------------------------------------
def _spans(k):
    return list(range(0, 2 * k, 2)), list(range(1, 2 * k + 1, 2)), [-(i + 1.0) for i in range(k)]


def test_word_grouping_character_vocabulary():
    from mamba_asr_amd.ctc_decode import CTCAligner, CTCBeamSearcher
    vocab = ["<blank>", " ", "a", "b", "c", "<unk>"]
    al, se = CTCAligner(0, vocab), CTCBeamSearcher(0, vocab)
    #         ' '  a  b ' ' ' ' <unk> c ' '  a
    tokens = [1, 2, 3, 1, 1, 5, 4, 1, 2]
    a, z, lp = _spans(len(tokens))
    words, frames, wlp = al.words(tokens, a, z, lp)
    assert words == ["ab", "<unk>c", "a"] == se.compose(tokens).split(" ")
    assert frames == [(2, 5), (10, 13), (16, 17)]                    # leading and doubled spaces belong to no word
    assert wlp == [-2.0 + -3.0, -6.0 + -7.0, -9.0]
    assert al.words([], [], [], []) == ([], [], [])
    assert al.words([1, 1], [0, 1], [1, 2], [-1.0, -1.0]) == ([], [], [])
    assert al.words([2, 0, 3], [0, 1, 2], [1, 2, 3], [-1.0, -5.0, -2.0]) == (["ab"], [(0, 3)], [-3.0])   # a blank label is no text


def test_word_grouping_sentencepiece_vocabulary():
    from mamba_asr_amd.ctc_decode import CTCAligner, CTCBeamSearcher
    vocab = ["<blank>", "<unk>", "▁the", "▁c", "at", "s", "▁"]
    al, se = CTCAligner(0, vocab), CTCBeamSearcher(0, vocab)
    assert al.is_spm and al.classes == se.classes and al.clean == se.clean
    #         ▁the ▁c at s ▁ <unk> ▁ ▁the
    tokens = [2, 3, 4, 5, 6, 1, 6, 2]
    a, z, lp = _spans(len(tokens))
    words, frames, wlp = al.words(tokens, a, z, lp)
    assert words == ["the", "cats", "<unk>", "the"] == se.compose(tokens).split(" ")
    assert frames == [(0, 1), (2, 7), (10, 11), (14, 15)]            # the bare piece starts a word and belongs to none
    assert wlp == [-1.0, -2.0 + -3.0 + -4.0, -6.0, -8.0]
    assert al.words([4, 5], [3, 5], [4, 9], [-1.0, -2.0]) == (["ats"], [(3, 9)], [-3.0])    # no word-start in front: still a word


# ----------------------------------------------------------------------------------------------------------
# the C ABI on the host
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    if not os.path.exists(N.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "mamba_asr_amd", "csrc")])
    return N


def test_header_declares_the_alignment_abi(native):
    hdr = open(os.path.join(ROOT, "include", "conmamba_hip.h")).read()
    assert re.search(r"typedef\s+struct\s+cm_ctc_align_args\s*\{", hdr)
    assert re.search(r"int64_t\s+cm_ctc_align_workspace_bytes\s*\(const cm_ctc_align_args \*", hdr)
    assert re.search(r"int\s+cm_ctc_align\s*\(const cm_ctc_align_args \*", hdr)
    assert native.ABI_VERSION == 12 and native.lib().cm_abi_version() == 12
    names = [f for f, _ in native.CtcAlignArgs._fields_]
    assert names[:6] == ["batch", "T", "V", "S", "blank", "dtype"] and names[6:9] == ["lp_rows", "lp_bs", "lp_ts"]
    assert names[-3:] == ["workspace", "workspace_bytes", "stream"] and "rows" in names


@pytest.mark.parametrize("batch, T, S", [(64, 4000, 1023), (1, 1, 0), (3, 17, 33), (2, 16, 31), (2, 15, 32)])
def test_workspace_bound(native, batch, T, S):
    a = native.CtcAlignArgs()
    a.batch, a.T, a.S = batch, T, S
    got = native.lib().cm_ctc_align_workspace_bytes(C.byref(a))
    t16, e64 = (T + 15) // 16 * 16, (2 * S + 1 + 63) // 64 * 64
    assert 0 < got <= batch * (t16 * e64 // 4 + 16 * (T + S) + 4096) and got % 16 == 0
    assert got >= batch * T * (2 * S + 1) // 4                      # 2 bits per cell, at least
    assert native.lib().cm_ctc_align_workspace_bytes(None) == 0


def _args(native, S=4, T=8, V=5, batch=2):
    """A valid argument block over host memory (never launched: every case below is refused first)."""
    a = native.CtcAlignArgs()
    a.batch, a.T, a.V, a.S, a.blank, a.dtype = batch, T, V, S, 0, native.CM_F32
    a.lp_rows, a.lp_bs, a.lp_ts = batch, T * V, V
    keep = [C.create_string_buffer(1 << 16) for _ in range(12)]
    ptr = [(C.addressof(k) + 63) // 64 * 64 for k in keep]
    (a.log_probs, a.targets, a.input_lengths, a.target_lengths, a.score, a.status, a.states, a.starts, a.ends, a.label_logp,
     a.workspace) = ptr[:11]
    a.workspace_bytes = native.lib().cm_ctc_align_workspace_bytes(C.byref(a))
    return a, keep


def test_host_refusals(native):
    lib = native.lib()

    def refused(a, code, text):
        assert lib.cm_ctc_align(C.byref(a)) == code, text
        assert text.encode() in lib.cm_last_error(), lib.cm_last_error()
    assert lib.cm_ctc_align(None) == native.CM_EINVAL
    a, keep = _args(native, S=1024)
    refused(a, native.CM_EUNSUPPORTED, "at most 1023 labels")
    for blank in (-1, 5):
        a, keep = _args(native)
        a.blank = blank
        refused(a, native.CM_EINVAL, "blank")
    for field in ("score", "status", "states", "starts", "ends", "label_logp", "log_probs", "input_lengths", "target_lengths",
                  "workspace"):
        a, keep = _args(native)
        setattr(a, field, None)
        refused(a, native.CM_EINVAL, "NULL")
    a, keep = _args(native)
    a.targets = None
    refused(a, native.CM_EINVAL, "targets must be NULL exactly when S == 0")
    a, keep = _args(native, S=0)
    refused(a, native.CM_EINVAL, "targets must be NULL exactly when S == 0")
    a, keep = _args(native)
    a.workspace_bytes -= 1
    refused(a, native.CM_EINVAL, "workspace smaller")
    a, keep = _args(native)
    a.workspace += 8
    refused(a, native.CM_EALIGN, "aligned")
    a, keep = _args(native)
    a.dtype = native.CM_F16
    refused(a, native.CM_EUNSUPPORTED, "dtype")
    a, keep = _args(native)
    a.T = 0
    refused(a, native.CM_EINVAL, "bad sizes")
    a, keep = _args(native)
    a.lp_rows = 1                                                    # no rows: every utterance needs its own
    refused(a, native.CM_EINVAL, "lp_rows")


def test_cpu_tensors_raise(native):
    from mamba_asr_amd import ops
    from mamba_asr_amd.ctc_decode import CTCAligner
    lp = torch.zeros(1, 4, 3).log_softmax(-1)
    tg, one = torch.tensor([[1]]), torch.tensor([1])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.ctc_align(lp, tg, torch.tensor([4]), one)
    with pytest.raises(RuntimeError, match="GPU only"):
        CTCAligner(0, ["<b>", "a", "b"])(lp, [[1]])
