"""The benchmark's own shapes, on the code paths bench.py times.

Forward (bench.py defaults): conmamba_large_ctc, 64 x 40 s, bf16, replayed by fused.GraphedEncode.  At 64 utterances the fused
encoder runs the batch as two parts of 32 on two HIP streams, joined around one whole-batch, unchunked scan launch per layer
(fused._encoder_forward_joined).  Training (bench.py --mode train's micro-batch): 32 x 40 s through brain.Brain(graph_steps=True),
bf16, dropout live.  Checked here:
  * the route: the forward takes exactly that path (a silent fall-back to another route fails);
  * graph == eager, bit for bit, also after copying a permuted batch into the graph's input buffers;
  * utterances are independent across the part seam (utterances 31 | 32), bit for bit;
  * four utterances of the graphed output (0, 31, 32, 63) against the oracle, with negative controls that perturb the oracle the
    way a plausible kernel bug would;
  * cm_scan_cl_fwd at (64, 1000, 512) and cm_scan_cl_bwd at (32, 1000, 512) against the oracle's scans in fp64 on the unchunked launches;
  * the graphed training micro-batch == an eager one drawn at the same dropout epoch ("fresh" and "warm" captures);
  * outputs and gradients do not change when the caching allocator hands out memory poisoned with NaN bytes or a large finite
    pattern (a kernel that reads a torch.empty workspace, pad row or tail before writing it would show);
  * two fresh processes compute the same forward bits.
"""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conmamba_oracle as O
from test_hip_parity_r3 import _same_grads, rel_l2
from test_scan_rows_bwd import _case, close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, T = 4000, 1000                      # 40 s: 4000 Fbank frames, 1000 encoder steps
B_FWD, B_TRAIN = 64, 32                      # bench.py --batch default; the --mode train micro-batch of the `train` key
SEAM = B_FWD // 2                            # first utterance of part 1
PICK = (0, SEAM - 1, SEAM, B_FWD - 1)        # utterances checked against the oracle: both ends of both parts

# Oracle bounds for the 18-layer bf16 forward, per utterance (relative L2 of the encoder output, max |error| / max |oracle|, max
# |error| of the CTC log-probabilities).  Measured on an MI355X over PICK: worst rel L2 4.16e-3, worst max-error ratio 6.75e-3, worst
# log-prob error 9.83e-3 (the four utterances agree to 1 %); the bounds are 1.56x, 1.56x and 1.48x those values.
REL_L2_BOUND, MAX_ERR_BOUND, LOGP_BOUND = 6.5e-3, 1.05e-2, 1.45e-2



# ----------------------------------------------------------------------------------------------------------
# forward: 64 x 40 s, bench.py's defaults
# ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd():
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = CONFIGS["conmamba_large_ctc"]
    model = ConMambaASR(cfg).to(DEV).eval()
    wavs, lens = synthetic_wavs(B_FWD, samples_for_frames(FRAMES), cfg.seed, DEV)       # bench.make_batch at rank 0
    model.calibrate(wavs, lens)

    def encode(w, l):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return model.encode(w, l)

    full = encode(wavs, lens)
    assert full.shape == (B_FWD, T, cfg.d_model) and torch.isfinite(full).all()
    return dict(cfg=cfg, model=model, wavs=wavs, lens=lens, encode=encode, full=full, cache={})


def _seam_perm():
    """A permutation that moves every utterance to the other part, and to another position inside it."""
    g = torch.Generator().manual_seed(11)
    perm = torch.cat([SEAM + torch.randperm(SEAM, generator=g), torch.randperm(SEAM, generator=g)])
    assert bool((perm // SEAM != torch.arange(B_FWD) // SEAM).all())
    return perm.to(DEV)


def test_forward_takes_the_benchmark_route(fwd):
    """One eager 64 x 40 s pass under ops.LAUNCH_LOG: the CNN front end kernel, per layer exactly one cm_scan_cl_fwd over all 64
    utterances (both directions), cm_ffn_fused per part (two parts of 32), and the size policy leaves the scan unchunked."""
    from mamba_asr_amd import _native, ops
    assert _native.lib().cm_scan_cl_fwd_auto_chunks(B_FWD, T, 512, 2) == 1
    ops.LAUNCH_LOG = []
    try:
        out = fwd["encode"](fwd["wavs"], fwd["lens"])
        torch.cuda.synchronize()
        log = [(name, units) for name, _, _, units in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    names = [n for n, _ in log]
    layers = fwd["cfg"].num_encoder_layers
    assert names.count("cm_cnn_front") == 1, sorted(set(names))
    scans = [u for n, u in log if n == "cm_scan_cl_fwd"]
    assert scans == [B_FWD * T * 2] * layers, scans
    ffn = [u for n, u in log if n == "cm_ffn_fused"]
    assert len(ffn) == layers * 2 * 2 and set(ffn) == {SEAM * T}, (len(ffn), sorted(set(ffn)))
    assert "cm_add_layernorm" not in names and "cm_gemm_bf16" not in names, sorted(set(names))
    assert torch.equal(out, fwd["full"])                         # event brackets change nothing; the forward repeats bit for bit


def test_ffn_fused_is_bit_reproducible_at_the_benchmark_rows():
    """cm_ffn_fused at the row counts the benchmark launches (one part: 32000 rows; the unsplit batch: 64000), every variant the
    forward and the training forward use, 6 repeats on the same inputs: the same bits each time.  Before the LayerNorm statistics' DPP sums were settled
    (mamba_asr_amd/csrc/ffn_fused.hip, group_sum16_settled) rows 7 mod 8 of a tile differed from run to run in the variants without an
    addend at 32000 rows and more -- the ~1 bf16 ulp run-to-run difference of the 64 x 40 s forward."""
    from mamba_asr_amd import ops
    g = torch.Generator(device=DEV).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    ln = lambda: (1 + 0.1 * r(256), 0.1 * r(256), 1e-5)
    pre, n1, n2 = ln(), ln(), ln()
    pk = lambda *s: ops.PackedWeight((r(*s) * 0.05).bfloat16(), ops.FFN_LAYOUT)
    w1, w2, wp = pk(1024, 256), pk(256, 1024), pk(1024, 256)
    b1, b2 = 0.1 * r(1024), 0.1 * r(256)
    bad = []
    for rows in (16000, 32000, 64000):
        x0, add = r(rows, 256), r(rows, 256).bfloat16()
        for name, kw in (("in_proj epilogue", dict(norm2=n1, proj_w=wp)), ("h out", dict(norm2=n1)),
                         ("addend, norm1", dict(addend=add, norm1=n2, want_h=False)),
                         ("training forward, dropout 0.1", dict(train=(0.1, 0.1, 1234, 5678)))):
            outs = []
            for _ in range(6):
                x = x0.clone()
                _, h = ops.ffn_fused(x, pre, w1, b1, w2, b2, alpha=0.5, **kw)
                outs.append((x, [] if h is None else list(h) if isinstance(h, tuple) else [h]))
            torch.cuda.synchronize()
            for x, h in outs[1:]:
                if not (torch.equal(x, outs[0][0]) and all(torch.equal(u, v) for u, v in zip(h, outs[0][1]))):
                    rows_bad = (x != outs[0][0]).any(1).nonzero().flatten()
                    bad.append((rows, name, rows_bad[:8].tolist()))
                    break
    print("cm_ffn_fused repeats that differ (rows, variant, first differing rows):", bad)
    assert not bad, bad


def test_graphed_forward_equals_eager_and_reads_its_inputs(fwd):
    """GraphedEncode (what bench.py times): two replays give the same bits, a replay gives eager model.encode's bits, and a permuted
    batch copied into the graph's input buffers gives eager encode of the permuted batch (a graph that baked in its inputs fails)."""
    from mamba_asr_amd.fused import GraphedEncode
    model, wavs, lens = fwd["model"], fwd["wavs"], fwd["lens"]
    graphed = GraphedEncode(model, wavs, lens, dtype=torch.bfloat16)
    a = graphed().clone()
    b = graphed().clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(a, fwd["full"]), f"graph vs eager max|diff| {float((a - fwd['full']).abs().max()):.3e}"
    perm = _seam_perm()
    gp = graphed(wavs[perm], lens[perm]).clone()
    ep = fwd["encode"](wavs[perm], lens[perm])
    assert torch.equal(gp, ep)
    assert torch.equal(graphed(wavs, lens), a)                   # and back
    fwd["cache"]["graphed"] = a
    fwd["cache"]["perm_eager"] = (perm, ep)
    del graphed


def test_utterances_are_independent_across_the_part_seam(fwd):
    """Eager encode of the seam-crossing permutation == the permuted full output, bit for bit; a 16-utterance slice around the seam
    (one part, one unchunked scan: no stream join) gives the full batch's rows."""
    from mamba_asr_amd import _native
    wavs, lens, full = fwd["wavs"], fwd["lens"], fwd["full"]
    perm, ep = fwd["cache"].get("perm_eager") or (None, None)
    if perm is None:
        perm = _seam_perm()
        ep = fwd["encode"](wavs[perm], lens[perm])
    assert torch.equal(ep, full[perm])
    assert _native.lib().cm_scan_cl_fwd_auto_chunks(16, T, 512, 2) == 1
    sl = slice(SEAM - 8, SEAM + 8)
    part = fwd["encode"](wavs[sl], lens[sl])
    assert torch.equal(part, full[sl]), f"max|diff| {float((part - full[sl]).abs().max()):.3e}"


class _Scan:
    """The oracle's scan, optionally perturbed at some calls.  bimamba_v2 scans the forward direction, then the backward one, per
    layer: call 2 * layer is layer's forward direction, 2 * layer + 1 its backward direction (on time-flipped inputs)."""

    def __init__(self, base, calls=(), kind=None):
        self.base, self.calls, self.kind, self.n = base, set(calls), kind, 0

    def __call__(self, u, delta, A, B, C, D=None, z=None, **kw):
        hit = self.n in self.calls
        self.n += 1
        if hit and self.kind == "no_D":
            D = None                                              # the skip term u * D never added
        out = self.base(u, delta, A, B, C, D, z, **kw)
        if hit and self.kind == "shift":
            out = torch.cat([out[..., :1], out[..., :-1]], -1)    # every output one step late in the scan's own time order
        return out


def _oracle_encode(fwd, i, scan):
    """O.asr_encode of utterance i in fp64: fp64 parameters and fp64 normalisation statistics, so everything after the (fp32)
    Fbank runs in fp64 -- except the mixer's conv / x_proj / scan, which the oracle's bimamba_v2 runs in fp32."""
    c = fwd["cache"]
    if "params" not in c:
        sd = fwd["model"].state_dict()
        c["params"] = {k: v.detach().double().cpu() for k, v in sd.items() if v.is_floating_point()}
    p = c["params"]
    cfg = fwd["cfg"]
    return O.asr_encode(p, fwd["wavs"][i:i + 1].cpu(), fwd["lens"][i:i + 1].cpu(), cfg.num_encoder_layers,
                        p["normalize.glob_mean"], p["normalize.glob_std"], scan=scan, n_fft=cfg.n_fft, win_ms=cfg.win_length)[0]


def _errors(got, ref, p):
    """(relative L2, max |error| / max |ref|, max |error| of the CTC log-probabilities) of one utterance's encoder output."""
    g, r = got.detach().double().cpu(), ref.detach().double()
    lg = torch.log_softmax(F.linear(g, p["ctc_lin.w.weight"], p["ctc_lin.w.bias"]), -1)
    lr = torch.log_softmax(F.linear(r, p["ctc_lin.w.weight"], p["ctc_lin.w.bias"]), -1)
    return rel_l2(g, r), float((g - r).abs().max() / r.abs().max()), float((lg - lr).abs().max())


def _fails(e):
    return e[0] > REL_L2_BOUND or e[1] > MAX_ERR_BOUND or e[2] > LOGP_BOUND


def test_graphed_forward_vs_oracle_with_negative_controls(fwd):
    """Utterances 0, 31, 32, 63 of the graphed 64 x 40 s output against O.asr_encode run one utterance at a time; then three
    perturbed oracles (what a plausible kernel bug would compute) must fail the same bounds: one layer's backward-direction scan one
    step late, one layer's D skip dropped, and one utterance's rows taken from its neighbour across the seam."""
    O.set_threads(16)
    try:
        O.load_c_oracle()
        base = O.selective_scan_c                                 # fp32 C restatement, ~10x the torch loop's speed
    except OSError:
        base = O.selective_scan
    got = fwd["cache"].get("graphed")
    if got is None:
        from mamba_asr_amd.fused import GraphedEncode
        graphed = GraphedEncode(fwd["model"], fwd["wavs"], fwd["lens"], dtype=torch.bfloat16)
        got = graphed().clone()
        torch.cuda.synchronize()
        del graphed
    got = got.cpu()
    refs, worst = {}, [0.0, 0.0, 0.0]
    for i in PICK:
        refs[i] = _oracle_encode(fwd, i, _Scan(base))
        p = fwd["cache"]["params"]
        e = _errors(got[i], refs[i], p)
        worst = [max(a, b) for a, b in zip(worst, e)]
        print(f"utterance {i:2d} vs oracle: rel L2 {e[0]:.3e}  max|err|/max|ref| {e[1]:.3e}  CTC log-prob max|err| {e[2]:.3e}")
    print(f"worst: rel L2 {worst[0]:.3e} (bound {REL_L2_BOUND})  max-error ratio {worst[1]:.3e} (bound {MAX_ERR_BOUND})  "
          f"log-prob {worst[2]:.3e} (bound {LOGP_BOUND})")
    # negative controls on utterance 31 (the last one of part 0)
    i, n = SEAM - 1, fwd["cfg"].num_encoder_layers
    controls = {
        f"layer {n // 2} backward scan one step late": _oracle_encode(fwd, i, _Scan(base, [2 * (n // 2) + 1], "shift")),
        "every layer's backward scan one step late": _oracle_encode(fwd, i, _Scan(base, range(1, 2 * n, 2), "shift")),
        f"layer {n // 2} forward-direction D skip dropped": _oracle_encode(fwd, i, _Scan(base, [2 * (n // 2)], "no_D")),
        f"layer {n - 1} forward-direction D skip dropped": _oracle_encode(fwd, i, _Scan(base, [2 * n - 2], "no_D")),
    }
    errs = {k: _errors(got[i], r, p) for k, r in controls.items()}
    errs["utterance 31 <- rows of utterance 32"] = _errors(got[SEAM], refs[i], p)
    last = got[i].clone()
    last[-1] = got[SEAM][-1]
    errs["utterance 31, last row <- utterance 32's"] = _errors(last, refs[i], p)
    for k, e in errs.items():
        print(f"control {k}: rel L2 {e[0]:.3e} ({e[0] / REL_L2_BOUND:.2f}x bound)  max-error ratio {e[1]:.3e} "
              f"({e[1] / MAX_ERR_BOUND:.2f}x)  log-prob {e[2]:.3e} ({e[2] / LOGP_BOUND:.2f}x)")
    assert worst[0] <= REL_L2_BOUND and worst[1] <= MAX_ERR_BOUND and worst[2] <= LOGP_BOUND, worst
    # A single layer's scan one step late stays under the bf16 error of 18 layers (measured 1.2x the worst clean rel L2, 0.8x the
    # bound): the whole-model comparison cannot see it, test_scan_fwd_at_the_benchmark_shape_vs_oracle's control does.  Every other
    # control must fail: on rel L2 (scan or D-skip bugs), on the max-error ratio (rows from another utterance).
    undetectable = f"layer {n // 2} backward scan one step late"
    for k, e in errs.items():
        if k != undetectable:
            assert _fails(e), (k, e)
    assert errs["utterance 31, last row <- utterance 32's"][1] > MAX_ERR_BOUND


def test_scan_fwd_at_the_benchmark_shape_vs_oracle():
    """cm_scan_cl_fwd at (64, 1000, 512), dt_rank 16, both directions in one launch, as the size policy launches it (unchunked),
    against O.selective_scan in fp64 on utterances 0, 31, 32, 63 -- test_hip_ops' bf16 bounds for the row-group scan."""
    from mamba_asr_amd import _native, ops
    b, l, e, rank = B_FWD, T, 512, 16
    RW = 16 + 32
    assert _native.lib().cm_scan_cl_fwd_auto_chunks(b, l, e, 2) == 1
    gen = torch.Generator().manual_seed(6401)
    xz = torch.randn(b, l, 2 * e, generator=gen).bfloat16()
    z = xz[:, :, e:]
    ycat = torch.zeros(b, l, 2 * e, dtype=torch.bfloat16, device=DEV)
    xcat = (torch.randn(b, l, 2 * RW, generator=gen) * 0.5).bfloat16()
    ucat = torch.randn(b, l, 2 * e, generator=gen).bfloat16()
    dirs, params = [], []
    for i, rev in enumerate((False, True)):
        A = -torch.exp(torch.randn(e, 16, generator=gen) * 0.3)
        Wdt = torch.randn(e, rank, generator=gen) * 0.3
        D, bias = torch.randn(e, generator=gen), torch.randn(e, generator=gen) - 1
        params.append((A, Wdt, D, bias))
        dirs.append(dict(u=ucat[:, :, e * i:e * (i + 1)].to(DEV), A=A.to(DEV), D=D.to(DEV), delta_bias=bias.to(DEV),
                         dt_weight=ops.pad_dt_weight(Wdt.to(DEV)), xdbl=xcat[:, :, RW * i:RW * (i + 1)].to(DEV),
                         out=ycat[:, :, e * i:e * (i + 1)], reverse=rev))
    ops.LAUNCH_LOG = []
    try:
        ops.scan_cl_fwd(dirs, z=xz.to(DEV)[:, :, e:], delta_softplus=True)
        torch.cuda.synchronize()
        log = [(n, u) for n, _, _, u in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert log == [("cm_scan_cl_fwd", b * l * 2)]
    got = ycat.cpu()
    for i, rev in enumerate((False, True)):
        A, Wdt, D, bias = params[i]
        sel = list(PICK)
        xd = xcat[sel][:, :, RW * i:RW * (i + 1)].double()
        delta = torch.einsum("er,blr->bel", Wdt.bfloat16().double(), xd[:, :, :rank])
        f = (lambda t: t.flip(-1)) if rev else (lambda t: t)
        tr = lambda t: t.double().transpose(1, 2)
        ref = O.selective_scan(f(tr(ucat[sel][:, :, e * i:e * (i + 1)])), f(delta), A, f(tr(xd[:, :, 16:32])), f(tr(xd[:, :, 32:])), D,
                               f(tr(z[sel])), bias, True, work_dtype=torch.float64)
        ref = f(ref).transpose(1, 2)
        g = got[sel][:, :, e * i:e * (i + 1)].double()
        print(f"scan fwd (64, 1000, 512) {'backward' if rev else 'forward'} direction: max|err| {float((g - ref).abs().max()):.3e}, "
              f"rel L2 {rel_l2(g, ref):.3e}")
        close(g, ref, 1.6e-2, 1e-2)
        # negative control: the oracle one step late in the direction's own time order fails the same bound
        late = torch.cat([ref[:, 1:], ref[:, -1:]], 1) if rev else torch.cat([ref[:, :1], ref[:, :-1]], 1)
        print(f"  control, one step late: max|err| {float((g - late).abs().max()):.3e}")
        with pytest.raises(AssertionError):
            close(g, late, 1.6e-2, 1e-2)


# ----------------------------------------------------------------------------------------------------------
# training: 32 x 40 s, bench.py --mode train's micro-batch
# ----------------------------------------------------------------------------------------------------------
def test_scan_bwd_at_the_train_shape_vs_oracle():
    """cm_scan_cl_bwd at (32, 1000, 512), dt_rank 16, both directions, through the library's chunk policy (one pass here) against
    O.selective_scan_bwd in fp64 (tests/test_scan_rows_bwd.py's _case and bf16 bounds): du, dz, dxdbl on every utterance, and the
    parameter gradients dA, ddt_weight, dD, ddelta_bias summed over the whole batch."""
    from mamba_asr_amd import _native, ops
    b, l, e = B_TRAIN, T, 512
    assert _native.lib().cm_scan_cl_bwd_auto_chunks(b, l, e, 2) == 1
    dirs, gz, refs, rank, P = _case(ops, b, l, e, 16, torch.bfloat16, seed=3201)
    ops.LAUNCH_LOG = []
    try:
        outs = ops.scan_cl_bwd(dirs, gz)
        torch.cuda.synchronize()
        log = [(n, u) for n, _, _, u in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert log == [("cm_scan_cl_bwd", b * l * 2)]
    rt, at = 2e-2, 1.2e-2
    for d, (o, r) in enumerate(zip(outs, refs)):
        pairs = {"du": (o["du"], r["du"].transpose(1, 2)), "dz": (o["dz"], r["dz"].transpose(1, 2)),
                 "dB": (o["dxdbl"][:, :, P:P + 16], r["dB"].transpose(1, 2)), "dC": (o["dxdbl"][:, :, P + 16:], r["dC"].transpose(1, 2)),
                 "ddt": (o["dxdbl"][:, :, :rank], r["ddt"]), "dA": (o["dA"], r["dA"]), "ddt_weight": (o["ddt_weight"][:, :rank], r["dW"]),
                 "dD": (o["dD"], r["dD"]), "ddelta_bias": (o["ddelta_bias"], r["ddelta_bias"])}
        print(f"scan bwd (32, 1000, 512) direction {d}: " + ", ".join(
            f"{k} {float((g.double().cpu() - w).abs().max() / w.abs().max()):.1e}" for k, (g, w) in pairs.items()) + " (max|err| / max|ref|)")
        for k in ("du", "dz", "dB", "dC", "ddt"):
            close(pairs[k][0].float(), pairs[k][1], rt, at)
        close(o["dA"], r["dA"], 2e-2, 5e-3)
        close(o["dD"], r["dD"], 2e-2, 5e-3)
        close(o["ddelta_bias"], r["ddelta_bias"], 2e-2, 5e-3)
        close(o["ddt_weight"][:, :rank], r["dW"], 2e-2, 8e-3)
    # a second launch of the same inputs computes the same bits (a grid of 32 x 2 x 512 channels runs past residency)
    again = ops.scan_cl_bwd(dirs, gz)
    for d, (o, o2) in enumerate(zip(outs, again)):
        for k in o:
            if torch.is_tensor(o[k]):
                assert torch.equal(o[k], o2[k]), f"scan bwd direction {d}: {k} differs between two identical launches"


@pytest.fixture(scope="module")
def train():
    """bench.run_train's Brain at the `train` key's micro-batch: 32 x 40 s, bf16, accum 1, AdamW, dropout at the config's 0.1, without
    SpecAugment; normalisation statistics calibrated and frozen, so every micro-batch sees the same features."""
    from mamba_asr_amd import sb_compat as sb
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
    from mamba_asr_amd.brain import Brain
    cfg = CONFIGS["conmamba_large_ctc"]
    assert cfg.transformer_dropout > 0
    model = ConMambaASR(cfg).to(DEV)
    wavs, lens = synthetic_wavs(B_TRAIN, samples_for_frames(FRAMES), cfg.seed, DEV)
    tokens = torch.randint(3, cfg.output_neurons, (B_TRAIN, FRAMES // 8), generator=torch.Generator().manual_seed(0)).to(DEV)
    model.calibrate(wavs, lens)

    class ASR(Brain):
        def graph_prologue(self, batch):
            wavs, lens, tokens, tlens = batch
            with torch.no_grad():
                feats = self.modules["asr"].features(wavs, lens, epoch=0)
            return (feats, lens, tokens, tlens)

        def compute_forward(self, batch, stage):
            wavs, lens, tokens, tlens = batch
            return self.modules["asr"].forward_ctc(wavs, lens, epoch=0, feats=wavs if wavs.dim() == 3 else None)

        def compute_objectives(self, pred, batch, stage):
            wavs, lens, tokens, tlens = batch
            return self.modules["asr"].ctc_objective(pred, tokens, lens, tlens)

    brain = ASR({"asr": model}, opt_class=lambda ps: torch.optim.AdamW(ps, lr=1e-3, betas=(0.9, 0.98), eps=1e-9, weight_decay=5e-4),
                hparams={"precision": "bf16", "grad_accumulation_factor": 1, "max_grad_norm": 5.0},
                run_opts={"device": DEV, "graph_steps": True})
    brain.on_fit_start()
    brain.modules.train()
    model.normalize.eval()
    brain.max_grad_norm = 1e9               # clip coefficient exactly 1: the optimizer sees the micro-batch's raw gradients
    names = [k for k, p in model.named_parameters() if p.requires_grad]
    params = [p for p in model.parameters() if p.requires_grad]
    grabbed, real = [], brain.optimizer.step
    state = {"step": True}

    def step(*a, **k):                      # every optimizer step hands over the gradients; weights move only while state["step"]
        grabbed.append([None if q.grad is None else q.grad.detach().clone() for q in params])
        if state["step"]:
            real(*a, **k)
    brain.optimizer.step = step
    yield dict(brain=brain, batch=(wavs, lens, tokens, lens.clone()), names=names, grabbed=grabbed, state=state, model=model)
    from mamba_asr_amd import ops, weight_cache
    ops.SEED_EPOCH = None
    weight_cache.CACHE_INPLACE = False


# The CNN front end's conv2d backward is the vendor library's (MIOpen), whose weight gradient accumulates with atomics: under bf16
# autocast it changes from run to run (measured on an MI355X: CNN.blocks.1.conv.weight only, max |diff| 4.5e-4 of the tensor's largest
# |gradient|, 0 in the other comparisons).  The front end's tensors get 1e-3 of their scale (2.2x that); every other gradient must be
# bit-equal.
CNN_BF16_TOL = 1e-3


def _grads_equal(names, a, b):
    assert [x is None for x in a] == [y is None for y in b]
    keep = [(k, x, y) for k, x, y in zip(names, a, b) if x is not None]
    cnn = {k: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30)) for k, x, y in keep if k.startswith("CNN.")}
    print("  CNN front-end gradients, max |diff| / max |grad|: " + ", ".join(f"{k} {v:.1e}" for k, v in cnn.items()))
    return _same_grads([x for _, x, _ in keep], [y for _, _, y in keep], [k for k, _, _ in keep], cnn_tol=CNN_BF16_TOL)


def test_graphed_train_step_equals_eager_step(train, monkeypatch):
    """Each captured variant's replay ("fresh": right after an optimizer step, with the weight-cache refresh kernels; "warm": the
    weights unchanged) against an eager micro-batch at the same dropout draw: the host seeds the capture drew, the epoch word the
    replay used (ops.SEED_EPOCH) and torch's generator state at the replay.  Loss bit for bit; gradients by _same_grads (bit-equal
    outside the CNN front end's vendor convolution backward)."""
    from mamba_asr_amd import ops
    brain, batch, names, grabbed, state = train["brain"], train["batch"], train["names"], train["grabbed"], train["state"]
    seeds, replay = [], []
    draw = ops.draw_seed
    monkeypatch.setattr(ops, "draw_seed", lambda: replay.pop(0) if replay else (seeds.append(draw()), seeds[-1])[1])
    brain.fit_batch(batch)                                       # first sight: eager, then a real optimizer step
    state["step"] = False
    for variant in ("fresh", "warm"):
        n0, rng = len(seeds), torch.cuda.get_rng_state()
        loss_g = brain.fit_batch(batch)
        torch.cuda.synchronize()
        assert variant in brain._graphs[next(iter(brain._graphs))], (variant, list(brain._graphs.values()))
        grads_g, epoch = grabbed[-1], int(ops.SEED_EPOCH.item())
        captured = seeds[n0:]
        assert captured, "the capture drew no dropout seed"
        brain.graph_steps = False
        try:
            pro = brain.graph_prologue(batch)
            torch.cuda.set_rng_state(rng)
            ops.SEED_EPOCH.fill_(epoch)
            replay[:] = captured
            loss_e = brain.fit_batch(pro)
            torch.cuda.synchronize()
            assert not replay and len(seeds) == n0 + len(captured), "the eager micro-batch drew another number of seeds"
        finally:
            brain.graph_steps = True
            replay.clear()
        grads_e = grabbed[-1]
        print(f"{variant} replay (epoch {epoch}): loss graph {float(loss_g):.6f} eager {float(loss_e):.6f}")
        assert torch.equal(loss_g, loss_e), (variant, float(loss_g), float(loss_e))
        diff = [k for k, x, y in zip(names, grads_g, grads_e) if x is not None and y is not None and not _same_grads([x], [y], [k])]
        print(f"{variant}: {len(diff)} parameter gradients differ from the eager micro-batch: {diff[:12]}")
        assert _grads_equal(names, grads_g, grads_e), (variant, diff)


# ----------------------------------------------------------------------------------------------------------
# poisoned memory and separate processes
# ----------------------------------------------------------------------------------------------------------
def _poison(byte, streams):
    """Release the cache, then fill 6 GiB of large-pool and 256 MiB of small-pool blocks per stream with ``byte`` and free them
    again: the caching allocator hands these blocks out next (it keeps them per stream)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = []
    for k, st in enumerate(streams):
        with torch.cuda.stream(st):
            blocks = [torch.empty(512 << 20, dtype=torch.uint8, device=DEV) for _ in range(12 if k == 0 else 4)]
            blocks += [torch.empty(1 << 19, dtype=torch.uint8, device=DEV) for _ in range(512)]
            for t in blocks:
                t.fill_(byte)
            held += blocks
            del blocks
    torch.cuda.synchronize()
    del held


def _eager_micro_batch(train, seed):
    """One eager training micro-batch of the Brain (dropout drawn from torch's generators seeded with ``seed``) -> loss, gradients."""
    from mamba_asr_amd import ops
    brain = train["brain"]
    brain.graph_steps = False
    epoch = ops.SEED_EPOCH
    try:
        ops.SEED_EPOCH = None
        torch.manual_seed(seed)
        loss = brain.fit_batch(brain.graph_prologue(train["batch"]))
        torch.cuda.synchronize()
    finally:
        brain.graph_steps = True
        ops.SEED_EPOCH = epoch
    return loss, train["grabbed"][-1]


@pytest.mark.parametrize("byte", [0xFF, 0x4B], ids=["nan_bytes", "large_finite"])
def test_outputs_do_not_depend_on_uninitialised_memory(fwd, train, byte):
    """The eager 64 x 40 s forward and the eager 32 x 40 s training micro-batch, each after the caching allocator's free blocks (on
    every stream the paths launch on) were filled with 0xFF bytes (NaN in bf16 / fp32) or 0x4B bytes (1.3e7 in bf16 / fp32): the
    output, the loss and every gradient equal the run on clean memory (gradients: bit for bit outside the CNN front end's vendor
    convolution backward, as in _same_grads)."""
    from mamba_asr_amd import fused
    train["state"]["step"] = False
    streams = [torch.cuda.current_stream()] + list(fused._side_streams.get(torch.cuda.current_device(), []))
    cache = train.setdefault("clean", {})
    if "train" not in cache:
        cache["train"] = _eager_micro_batch(train, 77)
    _poison(byte, streams)
    out = fwd["encode"](fwd["wavs"], fwd["lens"])
    torch.cuda.synchronize()
    bad = ~torch.isfinite(out)
    assert not bool(bad.any()), f"{int(bad.sum())} non-finite values, first at {bad.nonzero()[0].tolist()}"
    assert torch.equal(out, fwd["full"]), f"max|diff| {float((out - fwd['full']).abs().max()):.3e}"
    del out
    _poison(byte, streams)
    loss, grads = _eager_micro_batch(train, 77)
    clean_loss, clean_grads = cache["train"]
    print(f"poison 0x{byte:02X}: forward equal; training loss {float(loss):.6f} (clean {float(clean_loss):.6f})")
    assert torch.equal(loss, clean_loss)
    assert _grads_equal(train["names"], grads, clean_grads)


_CHILD = r'''
import hashlib, os, sys
sys.path.insert(0, os.environ["CM_ROOT"])
import numpy as np, torch
from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
from mamba_asr_amd.fused import GraphedEncode
h = lambda t: hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:16]
cfg = CONFIGS["conmamba_large_ctc"]
model = ConMambaASR(cfg).to("cuda").eval()
wavs, lens = synthetic_wavs(64, samples_for_frames(4000), cfg.seed, "cuda")
model.calibrate(wavs, lens)
graphed = GraphedEncode(model, wavs, lens, dtype=torch.bfloat16)
out = graphed().clone()
with torch.no_grad():
    feats = model.compute_features(wavs, norm=(model.normalize.glob_mean, model.normalize.glob_std))
torch.cuda.synchronize()
np.save(os.environ["CM_OUT"], out.cpu().numpy())
print("HASH params", h(torch.cat([p.detach().flatten() for p in model.parameters()])), "feats", h(feats), "out", h(out))
'''


def test_two_processes_compute_the_same_forward(tmp_path):
    """Two fresh processes, one after the other, each under its own time limit, build the benchmark's model and batch and replay the
    64 x 40 s graphed forward: parameters, features and output hash the same."""
    script = tmp_path / "child.py"
    script.write_text(_CHILD)
    lines, outs = [], []
    for k in range(2):
        env = dict(os.environ, CM_ROOT=ROOT, CM_OUT=str(tmp_path / f"out{k}.npy"))
        cmd = [sys.executable, str(script)]
        if shutil.which("timeout"):
            cmd = ["timeout", "-k", "10", "300"] + cmd
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=330)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines.append([l for l in r.stdout.splitlines() if l.startswith("HASH ")][-1])
        outs.append(np.load(tmp_path / f"out{k}.npy"))
    diff = float(np.abs(outs[0] - outs[1]).max())
    print(f"process 1: {lines[0]}\nprocess 2: {lines[1]}\nmax|diff| {diff:.3e}, elements that differ: {int((outs[0] != outs[1]).sum())}")
    assert lines[0] == lines[1], (lines, diff)
