"""Every route of fused.encoder_forward is one layer -- head, scan, tail (fused.py's docstring) -- composed for one part or several.

  * each route's ordered native launches (name, units), its library out_proj GEMMs (fused._out_proj) and its library GEMMs in
    all (aten mm / addmm / _addmm_activation) equal what was recorded on MI355X from the commit before the layer was written
    once, when the single-stream route and the joined route were separate hand-written copies;
  * the joined route's layer is the single-stream layer once per part, except for the scan, which runs once; same bits;
  * a 'free' split with more parts than an earlier call's stream pool holds grows the pool (it used to index past its end).
"""
from collections import Counter

import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

pytestmark = pytest.mark.gpu
DEV = "cuda"
CFG = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
LAYERS, BATCH, FRAMES = 3, 17, 75                  # 17 utterances: uneven parts; 75 frames: no multiple of the scan's 16-step block
ALL = BATCH * FRAMES                               # or of the FFN's 64-token tile
PARTS = (6 * FRAMES, 5 * FRAMES, 6 * FRAMES)       # joined: utterances 0-6, 6-11, 11-17; 'free': chunks of 6, 6, 5 run as 2nd, 3rd, 1st

HEAD = ["cm_ffn_fused", "cm_conv_xproj"]
SCAN = ["cm_scan_cl_fwd"]
TAIL = ["cm_ln_pw_glu", "cm_glu_dwconv_ln_gelu", "cm_ffn_fused"]
FUSED = HEAD + SCAN + TAIL
PLAIN_CONV = ["cm_ffn_fused", "cm_conv_cl_fwd"] + SCAN + TAIL
SEAM_OFF = HEAD + SCAN + ["cm_add_layernorm", "cm_glu_dwconv_ln_gelu", "cm_ffn_fused"]
LIBRARY_FFN = ["cm_add_layernorm", "cm_add_layernorm", "cm_conv_xproj", "cm_scan_cl_fwd", "cm_add_layernorm", "cm_glu_dwconv_ln_gelu",
               "cm_add_layernorm", "cm_add_layernorm"]
NATIVE_GEMM = ["cm_gemm_bf16"] * 3 + ["cm_conv_cl_fwd", "cm_scan_cl_fwd"] + ["cm_gemm_bf16"] * 2 + ["cm_glu_dwconv_ln_gelu"] + ["cm_gemm_bf16"] * 3


def at(names, rows):
    """The launches ``names`` on ``rows`` rows: every kernel counts rows, the scan rows x 2 directions."""
    return [(n, rows * (2 if n == "cm_scan_cl_fwd" else 1)) for n in names]


def per_part(names):
    return [e for rows in PARTS for e in at(names, rows)]


# case -> (streams, STREAM_MODE, switches off (on for USE_NATIVE_GEMM), launches, fused._out_proj calls, library GEMMs)
ROUTES = {
    "one_part": (1, "join", (), at(FUSED, ALL) * LAYERS, 0, 0),
    "three_parts_join": (3, "join", (), (per_part(HEAD) + at(SCAN, ALL) + per_part(TAIL)) * LAYERS, 0, 0),
    "three_parts_pair": (3, "pair", (), (per_part(HEAD) + per_part(SCAN) + per_part(TAIL)) * LAYERS, 0, 0),
    "three_parts_free": (3, "free", (), [e for rows in PARTS for e in at(FUSED, rows) * LAYERS], 0, 0),
    "no_fused_ffn": (1, "join", ("USE_FUSED_FFN",), at(LIBRARY_FFN, ALL) * LAYERS + at(["cm_add_layernorm"], ALL), 3, 24),
    "no_ln_pw_glu": (1, "join", ("USE_LN_PW_GLU",), at(SEAM_OFF, ALL) * LAYERS, 3, 6),
    "no_conv_xproj": (1, "join", ("USE_CONV_XPROJ",), at(PLAIN_CONV, ALL) * LAYERS, 0, 3),
    "no_scan_rows": (1, "join", ("USE_SCAN_ROWS",), at(PLAIN_CONV, ALL) * LAYERS, 0, 3),
    "no_mixer_tail": (1, "join", ("USE_MIXER_TAIL",), at(FUSED, ALL) * LAYERS, 3, 3),
    "no_ffn_inproj": (1, "join", ("USE_FFN_INPROJ",), at(FUSED, ALL) * LAYERS, 0, 3),
    "no_dwconv_lin": (1, "join", ("USE_DWCONV_LIN",), at(FUSED, ALL) * LAYERS, 0, 3),
    "native_gemm": (1, "join", ("USE_NATIVE_GEMM",),
                    at(["cm_add_layernorm"], ALL) + at(NATIVE_GEMM, ALL) * LAYERS + at(["cm_add_layernorm"], ALL), 0, 3),
    # join with a layer the joined route does not cover falls through to the 'free' split
    "no_ln_pw_glu_three_parts": (3, "join", ("USE_LN_PW_GLU",), [e for rows in PARTS for e in at(SEAM_OFF, rows) * LAYERS], 9, 18),
}


def _encoder():
    """test_multi_stream_encoder_matches_single_stream's encoder and input; a fresh one per run: the layer caches read switches."""
    from mamba_asr_amd.modules.Conmamba import ConmambaEncoder
    torch.manual_seed(11)
    enc = ConmambaEncoder(num_layers=LAYERS, d_model=256, d_ffn=1024, kernel_size=31, activation=nn.GELU, bias=True,
                          dropout=0.0, causal=False, mamba_config=dict(CFG)).to(DEV).eval()
    for p in enc.parameters():
        if p.dim() > 1:
            nn.init.xavier_normal_(p)
    return enc, torch.randn(BATCH, FRAMES, 256, device=DEV)


class _LibraryGemms(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.count = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.count += func.overloadpacket.__name__ in ("mm", "addmm", "_addmm_activation", "bmm")
        return func(*args, **(kwargs or {}))


def _run_logged(monkeypatch, streams, mode="join", switches=()):
    """-> (output, [(kernel, units), ...] in launch order, fused._out_proj calls, library GEMMs)."""
    from mamba_asr_amd import fused, ops
    for s in switches:
        monkeypatch.setattr(fused, s, s == "USE_NATIVE_GEMM")
    monkeypatch.setattr(fused, "STREAM_MODE", mode)
    enc, x = _encoder()
    calls = []
    real = fused._out_proj
    monkeypatch.setattr(fused, "_out_proj", lambda c, ycat: (calls.append(1), real(c, ycat))[1])
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad(), _LibraryGemms() as gemms:
            out = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=streams)
        torch.cuda.synchronize()
        log = [(e[0], e[3]) for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    return out, log, len(calls), gemms.count


@pytest.fixture(scope="module")
def single_stream_output():
    from mamba_asr_amd import fused
    enc, x = _encoder()
    with torch.no_grad():
        out = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=1)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", list(ROUTES))
def test_every_route_launches_the_recorded_sequence(case, monkeypatch):
    streams, mode, switches, launches, out_projs, gemms = ROUTES[case]
    _, log, got_out_projs, got_gemms = _run_logged(monkeypatch, streams, mode, switches)
    assert log == launches, log
    assert (got_out_projs, got_gemms) == (out_projs, gemms)


def test_one_part_and_many_parts_are_the_same_layer(monkeypatch):
    one, log1, _, _ = _run_logged(monkeypatch, 1)
    three, log3, _, _ = _run_logged(monkeypatch, 3, "join")
    n1, n3 = len(log1) // LAYERS, len(log3) // LAYERS
    for li in range(LAYERS):
        layer1 = Counter(name for name, _ in log1[li * n1:(li + 1) * n1])
        layer3 = Counter(name for name, _ in log3[li * n3:(li + 1) * n3])
        assert layer1["cm_scan_cl_fwd"] == layer3.pop("cm_scan_cl_fwd") == 1
        del layer1["cm_scan_cl_fwd"]
        assert layer3 == Counter({name: 3 * k for name, k in layer1.items()})
    assert torch.equal(three, one)


def test_free_split_after_a_smaller_pool(monkeypatch, single_stream_output):
    """streams=2 leaves a pool of one side stream; a 'free' split into three then needs two."""
    from mamba_asr_amd import fused
    monkeypatch.setattr(fused, "_side_streams", {})
    enc, x = _encoder()
    with torch.no_grad():
        monkeypatch.setattr(fused, "STREAM_MODE", "join")
        two = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=2)
        assert len(fused._side_streams[x.device.index]) == 1
        monkeypatch.setattr(fused, "STREAM_MODE", "free")
        three = fused.encoder_forward(enc, x, dtype=torch.bfloat16, streams=3)
    torch.cuda.synchronize()
    assert torch.equal(two, single_stream_output) and torch.equal(three, single_stream_output)
