"""The bidirectional ConMamba encoder on a ragged batch (GPU): fused.encoder_forward(encoder, src, lens=...) gives every
utterance the rows it has when encoded ALONE -- torch.equal to encoder_forward on src[b:b+1, :lens[b]] with the scan unchunked
(ops.SCAN_CHUNKS = "1" for the solo runs: chunked and unchunked scans differ in bits, the route under ``lens`` is unchunked).

2 layers, d_model 256, bf16.  (a) B = 12, T_max = 70, lens 0 .. 70 across every tile edge, one part; (b) B = 32, T_max = 40, two
parts, joined (one scan on the whole batch) and paired (one scan per part), with the launch log: six native launches per layer and
part, no library GEMM inside a layer; (c) a captured hipGraph
replayed with other lengths written into the same tensor; (d) the same batch WITHOUT lens differs from the solo rows for every
utterance shorter than T_max -- the defect, and the proof that the inputs discriminate; (e) d_model 144, where library GEMMs remain,
at the bound of tests/test_encoder_d144_gpu.py (rtol 3e-2, atol 5e-2).  Rows of src at and past lens[b] are NaN throughout."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
LENS_A = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 69, 70]
T_A = 70
T_B = 40
LENS_B = [40, 1, 17, 33, 0, 16, 31, 40, 2, 39, 15, 32, 3, 24, 40, 8] + [5, 40, 29, 30, 12, 0, 36, 21, 40, 7, 18, 35, 1, 40, 27, 16]
LAYERS = 2
PART = ["cm_ffn_fused", "cm_conv_xproj_lens"], ["cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu_lens", "cm_ffn_fused"]


def _encoder(d=256, seed=11):
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(seed)
    enc = ConmambaEncoder(num_layers=LAYERS, d_model=d, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    return enc


def _src(batch, t, d, lens, seed):
    x = torch.randn(batch, t, d, generator=torch.Generator().manual_seed(seed)).to(DEV)
    ragged = x.clone()
    for b, n in enumerate(lens):
        ragged[b, n:] = NAN
    return x, ragged


def _solo(enc, x, lens):
    """Every utterance encoded alone on its own rows, the scan unchunked; computed once per case, left unchanged."""
    from mamba_asr_amd import fused, ops
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        mp.setattr(ops, "SCAN_CHUNKS", "1")
        return [fused.encoder_forward(enc, x[b:b + 1, :n], dtype=BF16, streams=1)[0] if n else None for b, n in enumerate(lens)]


def _lens(values):
    return torch.tensor(values, dtype=torch.int32, device=DEV)


def _same(out, solo, lens, what):
    for b, n in enumerate(lens):
        if n:
            assert bool(torch.isfinite(solo[b]).all())
            assert torch.equal(out[b, :n], solo[b]), f"{what}: utterance {b}, {n} rows: max |diff| {float((out[b, :n] - solo[b]).abs().max()):.3e}"


@pytest.fixture(scope="module")
def case_a():
    enc = _encoder()
    x, ragged = _src(len(LENS_A), T_A, 256, LENS_A, 21)
    return enc, x, ragged, _solo(enc, x, LENS_A)


def test_one_part_equals_every_utterance_alone(case_a):
    from mamba_asr_amd import fused
    enc, x, ragged, solo = case_a
    with torch.no_grad():
        out = fused.encoder_forward(enc, ragged, dtype=BF16, streams=1, lens=_lens(LENS_A))
    assert out.shape == (len(LENS_A), T_A, 256) and out.dtype == torch.float32
    _same(out, solo, LENS_A, "one part")


def test_without_lens_padding_reaches_every_shorter_utterance(case_a):
    """The defect: zero padding behind an utterance (the kindest padding there is) changes its rows."""
    from mamba_asr_amd import fused, ops
    enc, x, ragged, solo = case_a
    with pytest.MonkeyPatch.context() as mp, torch.no_grad():
        mp.setattr(ops, "SCAN_CHUNKS", "1")
        out = fused.encoder_forward(enc, ragged.nan_to_num(0.0), dtype=BF16, streams=1)
    for b, n in enumerate(LENS_A):
        if 0 < n < T_A:
            assert not torch.equal(out[b, :n], solo[b]), f"utterance {b} ({n} rows) does not see its padding: the case does not discriminate"
        elif n == T_A:
            assert torch.equal(out[b], solo[b])


@pytest.mark.parametrize("mode", ["join", "pair"])
def test_two_parts_joined_and_the_route(monkeypatch, mode):
    """join: one scan per layer on the whole batch, with the whole lens tensor; pair: one scan per part, with the part's slice."""
    from mamba_asr_amd import fused, ops
    monkeypatch.setattr(fused, "STREAM_MODE", mode)
    enc = _encoder(seed=12)
    x, ragged = _src(len(LENS_B), T_B, 256, LENS_B, 22)
    solo = _solo(enc, x, LENS_B)
    calls = {"gemm": 0}

    def counted(name):
        real = getattr(fused, name)

        def f(*a, **k):
            calls["gemm"] += 1
            return real(*a, **k)
        return f

    for name in ("_out_proj", "_in_proj", "_ffn"):
        monkeypatch.setattr(fused, name, counted(name))
    lens = _lens(LENS_B)
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            out = fused.encoder_forward(enc, ragged, dtype=BF16, streams=2, lens=lens)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    print("launches of the ragged joined route:", names)
    assert names == (PART[0] * 2 + ["cm_scan_cl_fwd_lens"] * (1 if mode == "join" else 2) + PART[1] * 2) * LAYERS, names
    assert calls == {"gemm": 0}, calls
    _same(out, solo, LENS_B, "two parts joined")
    with torch.no_grad():
        one = fused.encoder_forward(enc, ragged, dtype=BF16, streams=1, lens=lens)
    _same(one, solo, LENS_B, "one part")


def test_a_captured_graph_follows_lens_on_the_device(case_a):
    from mamba_asr_amd import fused
    enc, x, _, solo = case_a
    second = [70, 33, 0, 16, 3, 69, 1, 17, 32, 2, 15, 31]
    lens = _lens(LENS_A)
    src = x.clone()                                               # finite everywhere: both sets of lengths read their own rows of it
    with torch.no_grad():
        fused.encoder_forward(enc, src, dtype=BF16, streams=1, lens=lens)            # caches, packed weights
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = fused.encoder_forward(enc, src, dtype=BF16, streams=1, lens=lens)
        graph.replay()
        torch.cuda.synchronize()
        _same(out, solo, LENS_A, "captured, first lengths")
        lens.copy_(_lens(second))
        graph.replay()
        torch.cuda.synchronize()
        eager = fused.encoder_forward(enc, src, dtype=BF16, streams=1, lens=_lens(second))
    for b, n in enumerate(second):
        assert torch.equal(out[b, :n], eager[b, :n]), f"replay with other lengths: utterance {b}, {n} rows"
    _same(out, _solo(enc, x, second), second, "captured, second lengths")


def test_fallback_routes_give_the_same_semantics(case_a, monkeypatch):
    """fp32, and bf16 with a switch off: each utterance alone on its own rows, scattered -- lens= never raises for a supported model."""
    from mamba_asr_amd import fused, ops
    enc, x, ragged, _ = case_a
    lens = _lens(LENS_A)
    monkeypatch.setattr(ops, "SCAN_CHUNKS", "1")
    for dtype, switch in ((torch.float32, None), (BF16, "USE_LN_PW_GLU")):
        if switch:
            monkeypatch.setattr(fused, switch, False)
        enc2 = _encoder()                                         # a fresh encoder: the layer caches read the switches
        with torch.no_grad():
            out = fused.encoder_forward(enc2, ragged, dtype=dtype, streams=1, lens=lens)
            for b, n in enumerate(LENS_A):
                if n:
                    assert torch.equal(out[b, :n], fused.encoder_forward(enc2, x[b:b + 1, :n], dtype=dtype, streams=1)[0]), (dtype, switch, b, n)


def test_d_model_144_against_solo_runs():
    """d_model 144: whichever route encoder_forward picks (library GEMMs remain at this width: out_proj and the closing Linear)."""
    from mamba_asr_amd import fused
    lens = [75, 1, 16, 33, 74, 47, 0, 64, 17]
    enc = _encoder(d=144, seed=13)
    x, ragged = _src(len(lens), 75, 144, lens, 23)
    solo = _solo(enc, x, lens)
    with torch.no_grad():
        out = fused.encoder_forward(enc, ragged, dtype=BF16, streams=1, lens=_lens(lens))
    worst = 0.0
    for b, n in enumerate(lens):
        if n:
            worst = max(worst, float((out[b, :n] - solo[b]).abs().max()))
            torch.testing.assert_close(out[b, :n], solo[b], rtol=3e-2, atol=5e-2)
    print(f"d_model 144, ragged against solo: max |diff| {worst:.3e}")
