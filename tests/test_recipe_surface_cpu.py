"""The recipe surface without a GPU: the objects a recipe YAML builds (mamba_asr_amd.hparams) against the hand-written mirror
(asr.ConMambaASR(CONFIGS[...])) that every GPU test and the benchmark run, what brain.Brain reads from the recipe, the epoch
counter, and InputNormalization's update_until_epoch gate along the epochs the counter yields.

Both recipe files run every case: hparams/CTC/conmamba_small.yaml (build-authored) and tests/golden/conmamba_large_ctc.yaml
(the reference's own, unmodified)."""
import os
from dataclasses import replace

import pytest
import torch
import torch.nn as nn

from recipe_brain import RecipeBrain, load_recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = {"conmamba_small_ctc": os.path.join(ROOT, "hparams", "CTC", "conmamba_small.yaml"),
           "conmamba_large_ctc": os.path.join(ROOT, "tests", "golden", "conmamba_large_ctc.yaml")}
NAMES = sorted(RECIPES)
SCALARS = (int, float, bool, str, tuple, type(None))


def _recipe_tree(hp):
    return nn.ModuleDict({**hp["modules"], "compute_features": hp["compute_features"]})


def _mirror(name, **over):
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR
    return ConMambaASR(replace(CONFIGS[name], **over))


def _scalars(m):
    return {k: v for k, v in vars(m).items() if not k.startswith("_") and k != "training" and isinstance(v, SCALARS)}


def _walk(a, b):
    """Every difference between two module trees as {(module name, what): (a's, b's)}: module names, classes, public scalar
    attributes, state-dict keys / shapes / dtypes, and the VALUES of every buffer, non-persistent ones included.
    -> (differences, number of modules, number of scalar attributes compared)."""
    diff = {}
    ma, mb = dict(a.named_modules()), dict(b.named_modules())
    for n in sorted(set(ma) ^ set(mb)):
        diff[(n, "module")] = (type(ma[n]).__name__ if n in ma else None, type(mb[n]).__name__ if n in mb else None)
    n_scalars = 0
    for n in sorted(set(ma) & set(mb)):
        x, y = ma[n], mb[n]
        if type(x) is not type(y):
            diff[(n, "class")] = (type(x).__name__, type(y).__name__)
        sx, sy = _scalars(x), _scalars(y)
        n_scalars += len(sx)
        for k in sorted(set(sx) | set(sy)):
            if k not in sx or k not in sy or type(sx[k]) is not type(sy[k]) or sx[k] != sy[k]:
                diff[(n, k)] = (sx.get(k, "<absent>"), sy.get(k, "<absent>"))
    sa, sb = a.state_dict(), b.state_dict()
    for k in sorted(set(sa) | set(sb)):
        mod = k.rpartition(".")[0]
        if k not in sa or k not in sb:
            diff[(mod, "state_dict key " + k)] = (k in sa, k in sb)
        elif sa[k].shape != sb[k].shape or sa[k].dtype != sb[k].dtype:
            diff[(mod, "state_dict entry " + k)] = ((tuple(sa[k].shape), sa[k].dtype), (tuple(sb[k].shape), sb[k].dtype))
    ba, bb = dict(a.named_buffers()), dict(b.named_buffers())
    for k in sorted(set(ba) | set(bb)):
        mod = k.rpartition(".")[0]
        if k not in ba or k not in bb:
            diff[(mod, "buffer " + k)] = (k in ba, k in bb)
        elif ba[k].shape != bb[k].shape or ba[k].dtype != bb[k].dtype or not torch.equal(ba[k], bb[k]):
            diff[(mod, "buffer " + k)] = ("differs", "differs")
    return diff, len(ma), n_scalars


def _allowed(key, hp):
    """The two differences the mirror may have -- a condition, not a tolerance: the root container's class, and
    Transformer.decoder_module while the model has no decoder (nothing reads it at zero decoder layers)."""
    return key == ("", "class") or (key == ("Transformer", "decoder_module") and hp["num_decoder_layers"] == 0)


@pytest.mark.parametrize("layers", [None, 2])
@pytest.mark.parametrize("name", NAMES)
def test_recipe_and_mirror_are_the_same_model(name, layers):
    over = {} if layers is None else {"num_encoder_layers": layers}
    hp = load_recipe(RECIPES[name], **over)
    tree, mirror = _recipe_tree(hp), _mirror(name, **over)
    diff, n_mod, n_attr = _walk(tree, mirror)
    print(f"{name}, {hp['num_encoder_layers']} layers: {n_mod} modules, {n_attr} scalar attributes, "
          f"{len(tree.state_dict())} state-dict entries; differences: {sorted(diff)}")
    assert n_mod > 50 and n_attr > 100 and len(hp["Transformer"].encoder.layers) == hp["num_encoder_layers"]
    assert set(diff) == {("", "class"), ("Transformer", "decoder_module")}, diff
    assert all(_allowed(k, hp) for k in diff), diff
    # the mirror seeds torch as the recipe's __set_seed does and builds its modules in the recipe's order: the same initial weights
    pa, pb = dict(tree.named_parameters()), dict(mirror.named_parameters())
    assert set(pa) == set(pb)
    unequal = [k for k in pa if not torch.equal(pa[k], pb[k])]
    assert not unequal, unequal[:5]


@pytest.mark.parametrize("name", NAMES)
def test_walk_negative_controls(name):
    """The walk reports a changed hyper-parameter at exactly the modules that hold it."""
    mirror = _mirror(name, num_encoder_layers=2)
    # (i) transformer_dropout 0.2: every module of the Transformer that carries the rate, nothing else
    hp = load_recipe(RECIPES[name], num_encoder_layers=2, transformer_dropout=0.2)
    tree = _recipe_tree(hp)
    diff, _, _ = _walk(tree, mirror)
    extra = {k: v for k, v in diff.items() if not _allowed(k, hp)}
    assert extra and all(v == (0.2, 0.1) for v in extra.values()), extra
    hit = {k[0] for k in extra}
    holders = {n for n, m in tree.named_modules() if n.startswith("Transformer.") and any(type(v) is float and v == 0.2 for v in _scalars(m).values())}
    drops = {n for n, m in tree.named_modules() if n.startswith("Transformer.") and isinstance(m, nn.Dropout)}
    print(f"{name}: transformer_dropout 0.2 reported at {len(hit)} modules ({len(drops)} of them nn.Dropout)")
    assert hit == holders and drops <= hit and len(drops) >= 1 + 5 * 2          # src dropout + five sites per encoder layer
    # (ii) the CNN's second block at 16 channels instead of 32: its convolution and its LayerNorm, nothing else
    with open(RECIPES[name]) as f:
        text = f.read()
    assert text.count("out_channels: (64, 32)") == 1
    from mamba_asr_amd.hparams import load_hparams
    hp = load_hparams(text.replace("out_channels: (64, 32)", "out_channels: (64, 16)"), overrides={"data_folder": "/nowhere", "num_encoder_layers": 2})
    diff, _, _ = _walk(_recipe_tree(hp), mirror)
    extra = {k: v for k, v in diff.items() if not _allowed(k, hp)}
    print(f"{name}: CNN out_channels (64, 16) reported as {sorted(extra)}")
    assert {k[0] for k in extra} == {"CNN.blocks.1.conv", "CNN.blocks.1.norm.norm"}, extra
    assert extra[("CNN.blocks.1.conv", "out_channels")] == (16, 32)
    assert extra[("CNN.blocks.1.norm.norm", "normalized_shape")] == ((20, 16), (20, 32))


@pytest.mark.parametrize("name", NAMES)
def test_brain_reads_the_recipe(name):
    from mamba_asr_amd import sb_compat as sb
    from mamba_asr_amd.hparams import Opaque
    hp = load_recipe(RECIPES[name], num_encoder_layers=2)
    assert isinstance(hp["epoch_counter"], sb.EpochCounter) and hp["epoch_counter"].limit == hp["number_of_epochs"] == 500
    assert isinstance(hp["checkpointer"], Opaque)
    assert hp["checkpointer"].kwargs["recoverables"]["counter"] is hp["epoch_counter"]
    br = RecipeBrain(hp, run_opts={"device": "cpu"})
    assert br.precision == "bf16" and br.grad_accumulation_factor == 4 and br.max_grad_norm == 5.0
    assert br.modules["Transformer"] is hp["Transformer"] and br.hparams.normalize is br.modules["normalize"]
    br.on_fit_start()
    assert isinstance(br.optimizer, torch.optim.AdamW)
    for g in br.optimizer.param_groups:
        assert g["lr"] == 0.001 and g["betas"] == (0.9, 0.98) and g["eps"] == 1e-9 and g["weight_decay"] == 0.0005
    held = {id(p) for g in br.optimizer.param_groups for p in g["params"]}
    assert held == {id(p) for p in hp["model"].parameters()}                    # the optimizer holds the recipe's `model` list
    if br.reducer is not None:
        br.reducer.close()


def test_epoch_counter():
    from mamba_asr_amd.sb_compat import EpochCounter
    c = EpochCounter(limit=4)
    assert c.current == 0
    seen = []
    for epoch in c:
        assert c.current == epoch                                               # set before the epoch runs
        seen.append(epoch)
    assert seen == [1, 2, 3, 4] and c.current == 4 and list(c) == []
    r = EpochCounter(6)
    r.current = 3                                                               # restored: continues at 4
    assert list(r) == [4, 5, 6]
    sd = EpochCounter(9)
    for _, epoch in zip(range(5), sd):
        pass
    state = sd.state_dict()
    assert state == {"current": 5}
    fresh = EpochCounter(9)
    fresh.load_state_dict(state)
    assert fresh.current == 5 and next(iter(fresh)) == 6 and sd.state_dict() == {"current": 5}


def norm_stats_fp64(batches):
    """InputNormalization's rule (class docstring) restated in fp64: per batch the mean over utterances of the per-utterance
    mean / unbiased std (floored at 1e-10) over the valid frames round(rel * frames); the first batch sets the statistics, batch
    k + 1 enters with weight 1 / (k + 1).  ``batches``: (features (b, frames, bins), relative lengths) -> (mean, std)."""
    mean = std = None
    for k, (x, lens) in enumerate(batches):
        x = x.double().cpu()
        ms, ss = [], []
        for i in range(x.shape[0]):
            n = max(int(torch.round(lens[i].double().cpu() * x.shape[1])), 1)
            ms.append(x[i, :n].mean(0))
            ss.append((x[i, :n].std(0) if n > 1 else torch.zeros_like(ms[-1])).clamp(min=1e-10))
        m, s = torch.stack(ms).mean(0), torch.stack(ss).mean(0)
        w = 1.0 / (k + 1)
        mean, std = (m, s) if k == 0 else ((1 - w) * mean + w * m, (1 - w) * std + w * s)
    return mean, std


def norm_stats_bound(frames, updates=1):
    """Relative bound of the fp32 statistics against norm_stats_fp64, from the frame count: a sum of n fp32 terms in any order
    is within (n - 1) u of the sum of their magnitudes (u = 2^-24), so a mean over ``frames`` frames is within frames * u of
    max|x|; the squared deviations are non-negative, so their sum carries the same relative error and the square root halves
    it.  What follows the frame sums is a fixed number of roundings: the division, the subtraction and the square under the
    deviation, the mean over utterances, and three per running-average update -- 16 u covers them with 4 u per update on top.
    Use: |mean - ref| <= bound * max|x|, |std - ref| <= bound * max(ref std)."""
    return (frames + 16 + 4 * updates) * 2.0 ** -24


@pytest.mark.parametrize("name", NAMES)
def test_normalisation_gate_along_epochs(name):
    from mamba_asr_amd.sb_compat import EpochCounter
    hp = load_recipe(RECIPES[name], num_encoder_layers=2)
    norm = hp["normalize"]
    assert norm.update_until_epoch == 4
    frames, bins = 137, hp["n_mels"]
    g = torch.Generator().manual_seed(11)
    batches = [(torch.randn(3, frames, bins, generator=g) * 7.0 - 20.0, torch.tensor([1.0, 0.83, 0.41])) for _ in range(6)]
    norm.train()
    counter, snaps = EpochCounter(6), []
    for epoch, (x, lens) in zip(counter, batches):                              # one batch per epoch
        out = norm(x, lens, epoch=counter.current)
        snaps.append((norm.count, norm.glob_mean.clone(), norm.glob_std.clone()))
        assert torch.equal(out, (x - norm.glob_mean) / norm.glob_std)
    assert counter.current == 6
    assert [s[0] for s in snaps] == [1, 2, 3, 3, 3, 3]                          # epochs 1, 2, 3 are below update_until_epoch: 4
    for s in snaps[3:]:
        assert torch.equal(s[1], snaps[2][1]) and torch.equal(s[2], snaps[2][2])    # bits kept from epoch 4 on
    assert not torch.equal(snaps[0][1], snaps[1][1]) and not torch.equal(snaps[1][2], snaps[2][2])
    want_mean, want_std = norm_stats_fp64(batches[:3])
    bound = norm_stats_bound(frames, updates=3)
    scale = max(float(x.abs().max()) for x, _ in batches[:3])
    e_mean = float((norm.glob_mean.double() - want_mean).abs().max()) / scale
    e_std = float((norm.glob_std.double() - want_std).abs().max()) / float(want_std.max())
    print(f"{name}: running statistics after 3 updates vs fp64: mean {e_mean:.2e} ({e_mean / bound:.3f} of the bound {bound:.2e}), "
          f"std {e_std:.2e} ({e_std / bound:.3f})")
    assert e_mean <= bound and e_std <= bound
    # a statistic that left one update out, or weighted the batches equally from the start, is far outside the bound
    two_mean, _ = norm_stats_fp64(batches[:2])
    assert float((two_mean - want_mean).abs().max()) / scale > 100 * bound
    # eval mode: nothing moves, whatever the epoch
    norm.eval()
    for epoch in (0, 1, 3, 9):
        norm(batches[5][0], batches[5][1], epoch=epoch)
    assert norm.count == 3 and torch.equal(norm.glob_mean, snaps[2][1]) and torch.equal(norm.glob_std, snaps[2][2])
    # a fresh normaliser in eval mode stays at mean 0 / std 1
    cold = load_recipe(RECIPES[name], num_encoder_layers=2)["normalize"].eval()
    out = cold(batches[0][0], batches[0][1], epoch=1)
    assert cold.count == 0 and torch.equal(out, batches[0][0])
