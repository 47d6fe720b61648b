"""The host contract of the Fbank + CNN front end's entry points, with host pointers only: every call here
is refused before a launch (a launch would fault).  The forms of one kernel family -- whole utterance, ``_lens``, lock-step ``_stream``,
per-slot ``_stream_slots`` -- go through one set of checks in csrc/cnn_front.hip and csrc/fbank_fft.hip, so one violation gets one
status from every form, under the form's own name, and a plan row is held to what cm_*_stream asks of the same scalars."""
import ctypes as C

import pytest

EINVAL, EUNSUPPORTED, EALIGN = -1, -2, -3


@pytest.fixture(scope="module")
def native():
    import mamba_asr_amd._native as N
    assert (N.CM_EINVAL, N.CM_EUNSUPPORTED, N.CM_EALIGN) == (EINVAL, EUNSUPPORTED, EALIGN)
    return N


_BUF = C.create_string_buffer((1 << 16) + 256)
BASE = (C.addressof(_BUF) + 255) // 256 * 256
SLOT_FIELDS = {"n": 0, "consumed": 1, "total": 2, "f0": 3, "nf": 4, "r0": 5, "nr": 6, "T_total": 7}      # plan-table columns


def call(native, name, a, plan=None, extra=None):
    """-> (status, message) of entry point ``name`` on struct ``a``; ``plan``: the rows of a per-slot form's table (one host array
    stands in for both copies); ``extra``: the second argument of a ``_lens`` form."""
    fn = getattr(native.lib(), name)
    if plan is not None:
        arr = (C.c_int32 * (8 * len(plan)))(*[v for row in plan for v in row])
        rc = fn(C.byref(a), C.addressof(arr), C.addressof(arr))
    elif name.endswith("_lens"):
        rc = fn(C.byref(a), BASE + 32768 if extra is None else extra)
    else:
        rc = fn(C.byref(a))
    return rc, native.lib().cm_last_error().decode()


def with_fields(a, plan, changes):
    """``changes`` applied to struct ``a``; a count that a per-slot form reads from its table goes into every row of ``plan`` too."""
    for field, value in changes:
        if hasattr(a, field):
            setattr(a, field, value)
        if plan is not None and field in SLOT_FIELDS:
            for row in plan:
                row[SLOT_FIELDS[field]] = value
    return a, plan


def case_ids(cases):
    return ["+".join(f"{f}={'NULL' if v is None else v - BASE if v >= BASE else v}" for f, v in changes) for changes, _ in cases]


# ------------------------------------------------------------------------------------------------ cm_cnn_front*
CNN_FRONT = ("cm_cnn_front", "cm_cnn_front_lens", "cm_cnn_front_stream", "cm_cnn_front_stream_slots")
STREAM_COUNTS = dict(f0=11, nf=9, r0=2, nr=3, T_total=-1)      # rows 2 .. 4 read frames 5 .. 19 of which 11 .. 19 arrive, 8 are history


def cnn_valid(native, name, **counts):
    """-> (struct, plan or None) that the entry point would launch."""
    stream = "stream" in name
    a = native.CnnFrontStreamArgs() if stream else native.CnnFrontArgs()
    a.batch, a.F, a.C1, a.C2 = 2, 80, 64, 32
    for f in ("feats", "w1", "b1", "ln1_g", "ln1_b", "w2", "b2", "ln2_g", "ln2_b", "out"):
        setattr(a, f, BASE)
    if not stream:
        a.T = 9
        return a, None
    a.feat_hist = BASE
    c = dict(STREAM_COUNTS, **counts)
    plan = [[0, 0, -1, c["f0"], c["nf"], c["r0"], c["nr"], c["T_total"]] for _ in range(2)] if name.endswith("_slots") else None
    return with_fields(a, None, c.items())[0], plan


CNN_SHARED = ((("feats", None),), EINVAL), ((("out", None),), EINVAL), ((("w2", None),), EINVAL), \
             ((("F", 81),), EUNSUPPORTED), ((("C1", 32),), EUNSUPPORTED), ((("C2", 64),), EUNSUPPORTED), \
             ((("w2", BASE + 8),), EALIGN), ((("ln1_g", BASE + 4),), EALIGN), \
             ((("w2", BASE + 8), ("F", 81)), EUNSUPPORTED)                      # the shape is asked before the alignment


@pytest.mark.parametrize("changes, status", CNN_SHARED, ids=case_ids(CNN_SHARED))
def test_cnn_front_forms_share_their_refusals(native, changes, status):
    for name in CNN_FRONT:
        a, plan = with_fields(*cnn_valid(native, name), changes)
        rc, msg = call(native, name, a, plan)
        assert rc == status and msg.startswith(name[3:] + ": "), (name, changes, rc, msg)


CNN_PER_STREAM = (("frames not arrived", dict(nr=4), "row 5 needs frames that have not arrived"),
                  ("T_total is not f0 + nf", dict(T_total=21), "T_total must be f0 + nf and at least 5"),
                  ("T_total under 5", dict(T_total=4), "T_total must be f0 + nf and at least 5"),
                  ("row past the last", dict(T_total=20, nr=4), "row 5 is past the utterance's last"),
                  ("row behind the history", dict(r0=1), "row 1 reaches behind the feature history"))


@pytest.mark.parametrize("what, counts, text", CNN_PER_STREAM, ids=[c[0] for c in CNN_PER_STREAM])
def test_cnn_front_plan_row_is_held_to_the_lock_step_conditions(native, what, counts, text):
    """The same scalars in cm_cnn_front_stream's struct and in a row of cm_cnn_front_stream_slots' plan: one status, one text."""
    rc, msg = call(native, "cm_cnn_front_stream", *cnn_valid(native, "cm_cnn_front_stream", **counts))
    assert rc == EINVAL and msg == "cnn_front_stream: " + text, (rc, msg)
    a, plan = cnn_valid(native, "cm_cnn_front_stream_slots", **counts)
    plan[0] = [0, 0, -1, 0, 0, 0, 0, -1]                                           # an idle slot in front: the refusal names slot 1
    rc, msg = call(native, "cm_cnn_front_stream_slots", a, plan)
    assert rc == EINVAL and msg == "cnn_front_stream_slots: slot 1: " + text, (rc, msg)


def test_cnn_front_slots_asymmetries_stay(native):
    """The per-slot form does not read the struct's f0 / r0 / T_total, and asks nothing of a slot without rows beyond its counts'
    range: with either in place the call gets as far as the refusal planted behind them (slot 1's frames have not arrived)."""
    a, plan = cnn_valid(native, "cm_cnn_front_stream_slots")
    a.f0, a.r0, a.T_total = -5, -1, 3                                              # each refused by cm_cnn_front_stream
    plan[0] = [0, 0, -1, 100, 0, 7, 0, 4]                                          # nr = 0: frames, history and T_total not looked at
    plan[1][4] = 8
    rc, msg = call(native, "cm_cnn_front_stream_slots", a, plan)
    assert rc == EINVAL and msg == "cnn_front_stream_slots: slot 1: row 4 needs frames that have not arrived", (rc, msg)
    b, _ = cnn_valid(native, "cm_cnn_front_stream")
    b.f0, b.r0, b.T_total = -5, -1, 3
    assert call(native, "cm_cnn_front_stream", b) == (EINVAL, "cnn_front_stream: bad sizes or NULL tensor")


# ------------------------------------------------------------------------------------------------ cm_fbank_wav / cm_fbank_finish and their _lens forms
def fbank_valid(native):
    a = native.FbankArgs()
    a.batch, a.n_freq, a.frames, a.n_mels, a.n_fft, a.hop, a.samples, a.wav_bs = 2, 257, 11, 80, 512, 160, 1600, 1600
    for f in ("wav", "window", "twiddle", "band_lo", "band_hi", "band_off", "band_w", "db", "umax", "umax_part"):
        setattr(a, f, BASE)
    a.amin, a.top_db = 1e-10, 80.0
    return a


FBANK_WAV = tuple((((f, None),), EINVAL) for f in ("window", "twiddle", "band_lo", "band_hi", "band_off", "band_w", "db", "umax_part")) + \
            ((((("n_fft", 400),), EUNSUPPORTED), ((("hop", 161),), EALIGN), ((("window", BASE + 4),), EALIGN), ((("frames", 12),), EINVAL),
              ((("window", BASE + 4), ("n_fft", 400)), EUNSUPPORTED)))


@pytest.mark.parametrize("changes, status", FBANK_WAV, ids=case_ids(FBANK_WAV))
def test_fbank_wav_forms_share_their_refusals(native, changes, status):
    """cm_fbank_wav_lens reports the checks it shares under the name of the form without lengths (its own three, on n_samples, under
    its own): kept as it is, DESIGN.md §4l."""
    for name in ("cm_fbank_wav", "cm_fbank_wav_lens"):
        rc, msg = call(native, name, with_fields(fbank_valid(native), None, changes)[0])
        assert rc == status and msg.startswith("fbank_wav: "), (name, changes, rc, msg)
    assert call(native, "cm_fbank_wav_lens", fbank_valid(native), extra=0) == (EINVAL, "fbank_wav_lens: n_samples is NULL (cm_fbank_wav is the form without lengths)")
    rc, msg = call(native, "cm_fbank_wav_lens", fbank_valid(native), extra=BASE + 2)
    assert rc == EALIGN and msg.startswith("fbank_wav_lens: "), (rc, msg)


FBANK_FINISH = ((("db", None),), "bad sizes or NULL tensor"), ((("umax", None),), "bad sizes or NULL tensor"), ((("frames", 0),), "bad sizes or NULL tensor"), \
               ((("mean", BASE),), "mean without std"), ((("batch", 65536),), "batch 65536 exceeds the grid limit")


@pytest.mark.parametrize("changes, text", FBANK_FINISH, ids=[c[0][0][0] for c in FBANK_FINISH])
def test_fbank_finish_forms_share_their_refusals(native, changes, text):
    for name in ("cm_fbank_finish", "cm_fbank_finish_lens"):
        rc, msg = call(native, name, with_fields(fbank_valid(native), None, changes)[0])
        assert rc == EINVAL and msg.startswith(f"{name[3:]}: {text}"), (name, changes, rc, msg)


def test_fbank_finish_forms_differ_where_they_did(native):
    """Only the form with lengths requires umax_part (without it cm_fbank_finish takes the maximum cm_fbank_mel_db left in umax) and
    the frame count of the samples; only the stream forms refuse std without mean.  Seen through the refusal behind: batch 65536."""
    a = fbank_valid(native)
    a.umax_part, a.batch = None, 65536
    assert call(native, "cm_fbank_finish", a) == (EINVAL, "fbank_finish: batch 65536 exceeds the grid limit")
    assert call(native, "cm_fbank_finish_lens", a) == (EINVAL, "fbank_finish_lens: bad sizes or NULL tensor (umax_part included)")
    a = fbank_valid(native)
    a.frames, a.batch = 12, 65536
    assert call(native, "cm_fbank_finish", a) == (EINVAL, "fbank_finish: batch 65536 exceeds the grid limit")
    assert call(native, "cm_fbank_finish_lens", a) == (EINVAL, "fbank_finish_lens: frames must be 1 + samples / hop")
    a = fbank_valid(native)
    a.std, a.batch = BASE, 65536                                                   # std without mean
    for name in ("cm_fbank_finish", "cm_fbank_finish_lens"):
        assert call(native, name, a) == (EINVAL, f"{name[3:]}: batch 65536 exceeds the grid limit")


# ------------------------------------------------------------------------------------------------ the stream forms of the Fbank
def fbank_stream_valid(native, slots):
    """tests/test_frontend_streaming_cpu.py's struct: frames 11 .. 19 of 160-sample hops from samples 2015 .. 3391 and 512 of history."""
    a = native.FbankStreamArgs()
    a.batch, a.n_mels, a.n_fft, a.hop, a.n, a.consumed, a.total, a.f0, a.nf = 2, 80, 512, 160, 1377, 2015, -1, 11, 9
    for f in ("chunk", "hist", "window", "twiddle", "band_lo", "band_hi", "band_off", "band_w", "db", "fmax", "umax", "feat_hist"):
        setattr(a, f, BASE)
    a.hist_out, a.feat_hist_out, a.chunk_bs, a.amin, a.top_db = BASE + 4096, BASE + 6144, 1377, 1e-10, 80.0
    return a, ([[1377, 2015, -1, 11, 9, 0, 0, -1] for _ in range(2)] if slots else None)


WAV_STREAM = (("chunk", None, EINVAL), ("hist", None, EINVAL), ("hist_out", None, EINVAL), ("hist_out", BASE, EINVAL), ("hist_out", BASE + 4092, EINVAL),
              ("db", None, EINVAL), ("fmax", None, EINVAL), ("band_w", None, EINVAL), ("n_fft", 400, EUNSUPPORTED), ("n_mels", 129, EUNSUPPORTED),
              ("hop", 161, EUNSUPPORTED), ("window", BASE + 4, EALIGN), ("twiddle", BASE + 4, EALIGN), ("nf", 10, EINVAL), ("f0", 10, EINVAL),
              ("total", 3000, EINVAL), ("n", -1, EINVAL))
FINISH_STREAM = (("db", None, EINVAL), ("fmax", None, EINVAL), ("umax", None, EINVAL), ("nf", 0, EINVAL), ("n_fft", 400, EUNSUPPORTED),
                 ("n_mels", 129, EUNSUPPORTED), ("feat_hist_out", BASE, EINVAL), ("feat_hist_out", BASE + 8 * 80 * 4 * 2 - 4, EINVAL),
                 ("feat_hist_out", None, EINVAL), ("std", BASE, EINVAL))


STREAM_CASES = [("cm_fbank_wav_stream",) + c for c in WAV_STREAM] + [("cm_fbank_finish_stream",) + c for c in FINISH_STREAM]


@pytest.mark.parametrize("entry, field, bad, status", STREAM_CASES,
                         ids=[f"{e[9:]}-{f}={'NULL' if v is None else v - BASE if v >= BASE else v}" for e, f, v, _ in STREAM_CASES])
def test_fbank_stream_forms_share_their_refusals(native, entry, field, bad, status):
    """Every refusal tests/test_frontend_streaming_cpu.py lists for the lock-step form, on that form and on the per-slot one (a count
    the latter reads per slot stands in the struct, its maximum, and in every row of the plan)."""
    for name, slots in ((entry, False), (entry + "_slots", True)):
        rc, msg = call(native, name, *with_fields(*fbank_stream_valid(native, slots), ((field, bad),)))
        assert rc == status and msg.startswith(name[3:] + ": "), (name, field, bad, rc, msg)


FBANK_PER_STREAM = (("samples not arrived", dict(nf=10), "frame 20 needs samples that have not arrived"),
                    ("total is not consumed + n", dict(total=3000), "total must be -1 or consumed + n, below 2^30"),
                    ("frame behind the history", dict(f0=10), "frame 10 reaches behind the history"),
                    ("negative count", dict(consumed=-1), "bad sample counts"))


@pytest.mark.parametrize("what, counts, text", FBANK_PER_STREAM, ids=[c[0] for c in FBANK_PER_STREAM])
def test_fbank_wav_plan_row_is_held_to_the_lock_step_conditions(native, what, counts, text):
    rc, msg = call(native, "cm_fbank_wav_stream", *with_fields(*fbank_stream_valid(native, False), counts.items()))
    assert rc == EINVAL and msg == "fbank_wav_stream: " + text, (rc, msg)
    a, plan = fbank_stream_valid(native, True)
    a.nf = 10                                                                      # the maximum: slot 1 alone breaks the condition
    for field, value in counts.items():
        plan[1][SLOT_FIELDS[field]] = value
    rc, msg = call(native, "cm_fbank_wav_stream_slots", a, plan)
    assert rc == EINVAL and msg == "fbank_wav_stream_slots: " + text, (rc, msg)
