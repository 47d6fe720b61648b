"""The CTC recipe's own objects on the GPU, in training order, against the fp64 oracle.

Every other GPU test builds asr.ConMambaASR(CONFIGS[...]); here the model, the feature pipeline, SpecAugment, the loss, the
optimizer, the scheduler and the beam search's keywords come out of the recipe YAML (tests/recipe_brain.py), at two encoder
layers: hparams/CTC/conmamba_small.yaml (d_model 144) and tests/golden/conmamba_large_ctc.yaml (d_model 256).  The batch is
tests/test_dropout_live_step._case's (2 utterances of 300 frames, lengths 1.0 / 0.8, ten tokens each); the reference is
oracle/conmamba_oracle.py through that file's machinery, which maps onto the recipe's modules by state-dict key
(tests/test_recipe_surface_cpu.py holds the two trees to the same keys).

  * eval forward: RecipeBrain.compute_forward (VALID) and ConMambaASR.forward_ctc on the same weights and statistics, both against
    the oracle's fp64 log-probabilities under the whole-model forward bound of tests/test_hip_parity_r3.py (close: rtol 2e-3,
    atol 5e-4 x max(1, max|ref|)); equal greedy tokens;
  * the training step with everything live (first-batch normalisation statistics at epoch 1, SpecAugment, every dropout site),
    fp32 and bf16 autocast: loss, every gradient and the normaliser's statistics against an oracle that computes its OWN
    statistics and fills the recorded masks with its OWN mean; negative controls on the CPU;
  * the loop at the recipe's accumulation, eager and graphed, with the Noam schedule;
  * the TEST stage's beam search, built from the recipe's keywords, against tests/ctc_beam_ref.py."""
from dataclasses import replace

import pytest
import torch

import test_dropout_live_step as L
from recipe_brain import RecipeBrain, load_recipe
from test_hip_parity_r3 import close                        # the whole-model forward comparison: rtol 2e-3, atol 5e-4 x max(1, max|ref|)
from test_recipe_surface_cpu import NAMES, RECIPES, norm_stats_bound, norm_stats_fp64

pytestmark = pytest.mark.gpu
DEV = "cuda"
FWD_RTOL, FWD_ATOL = 2e-3, 5e-4                             # close()'s arguments wherever a whole model's forward is compared


def _brain(name, graph=False, vocab_list=None, **over):
    from mamba_asr_amd.asr import CONFIGS
    hp = load_recipe(RECIPES[name], num_encoder_layers=L.LAYERS, **over)
    br = RecipeBrain(hp, run_opts={"device": DEV, "graph_steps": graph}, vocab_list=vocab_list)
    cfg = replace(CONFIGS[name], num_encoder_layers=L.LAYERS, transformer_dropout=hp["transformer_dropout"])
    return hp, br, cfg


def _batch(batch=2, frames=300, n_tok=10, seed=3502, lens=(1.0, 0.8), tok_lens=(1.0, 0.7)):
    """test_dropout_live_step._case's batch (its defaults), without its model."""
    from mamba_asr_amd.asr import samples_for_frames, synthetic_wavs
    wavs, _ = synthetic_wavs(batch, samples_for_frames(frames), seed, DEV)
    lens = torch.tensor(lens[:batch], device=DEV)
    for i, r in enumerate(lens.tolist()):
        wavs[i, int(round(r * wavs.shape[1])):] = 0.0
    gen = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randint(1, 31, (batch, n_tok), generator=gen)
    return wavs, lens, tokens, torch.tensor(tok_lens[:batch])


def _forward_error(got, ref):
    """The worst element's error as a fraction of close()'s allowance for it."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    allow = FWD_ATOL * max(1.0, float(ref.abs().max())) + FWD_RTOL * ref.abs()
    return float(((got - ref).abs() / allow).max())


@pytest.mark.parametrize("name", NAMES)
def test_eval_forward_recipe_and_mirror_vs_oracle(name):
    from mamba_asr_amd import dataio, ops
    from mamba_asr_amd.asr import ConMambaASR
    from mamba_asr_amd.brain import Stage
    hp, br, cfg = _brain(name)
    batch = wavs, lens, tokens, tok_lens = _batch()
    with torch.no_grad():
        hp["normalize"].update_statistics(hp["compute_features"](wavs), lens)
    br.modules.eval()
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            p_ctc, out_lens, greedy = br.compute_forward(batch, Stage.VALID)
        torch.cuda.synchronize()
        names = {e[0] for e in ops.LAUNCH_LOG}
    finally:
        ops.LAUNCH_LOG = None
    assert out_lens is lens and p_ctc.dtype == torch.float32 and p_ctc.shape == (2, 75, hp["output_neurons"])
    mirror = ConMambaASR(cfg).to(DEV).eval()
    mirror.load_state_dict(br.modules.state_dict())                           # strict: the same key set
    assert mirror.normalize.count == 1 and torch.equal(mirror.normalize.glob_mean, hp["normalize"].glob_mean)
    with torch.no_grad():
        p_mirror = mirror.forward_ctc(wavs, lens)
    want = L._oracle_logp(cfg, br.modules, wavs, None)[1].detach()
    e_recipe, e_mirror = _forward_error(p_ctc, want), _forward_error(p_mirror, want)
    print(f"{name} eval forward vs oracle (fp64), worst error / bound: recipe route {e_recipe:.2e}, ConMambaASR.forward_ctc {e_mirror:.2e}; "
          f"recipe route launched {sorted(names)}")
    close(p_ctc, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    close(p_mirror, want, rtol=FWD_RTOL, atol=FWD_ATOL)
    assert e_recipe <= 1.0 and e_mirror <= 1.0
    assert greedy == dataio.ctc_greedy_decode(p_mirror, lens, hp["blank_index"])
    assert greedy == dataio.ctc_greedy_decode(want, lens.cpu(), hp["blank_index"])


def _spec_masked(x, calls):
    """SpectrogramDrop(replace='mean') restated on fp64 features: per recorded call the cells under any of its masks take the
    mean of the tensor as it stood before that call."""
    for start, length, dim in calls:
        ar = torch.arange(x.shape[dim]).view(1, 1, -1)
        m = ((ar >= start[..., None]) & (ar < (start + length)[..., None])).any(1)
        m = m[:, :, None] if dim == 1 else m[:, None, :]
        x = torch.where(m, x.mean(), x)
    return x


def _oracle_features(calls, lens, stats):
    """-> the features hook of L._oracle: the oracle's own first-batch statistics from its own Fbank (kept in ``stats``), then the
    recorded masks filled with its own mean."""
    def hook(raw):
        x = raw.double()
        stats["mean"], stats["std"] = norm_stats_fp64([(x, lens.cpu())])
        stats["scale"] = float(x.abs().max())
        return _spec_masked((x - stats["mean"]) / stats["std"], calls)
    return hook


def _moved(calls, frames):
    """One time mask of utterance 0 one frame later (the first whose move changes the masked set)."""
    for c, (start, length, dim) in enumerate(calls):
        if dim != 1:
            continue
        for j in range(start.shape[1]):
            s2 = start.clone()
            s2[0, j] += 1
            assert int(s2[0, j] + length[0, j]) <= frames
            ar = torch.arange(frames)
            cover = lambda s: ((ar >= s[0, :, None]) & (ar < (s + length)[0, :, None])).any(0)
            if not torch.equal(cover(start), cover(s2)):
                return calls[:c] + [(s2, length, dim)] + calls[c + 1:], (int(start[0, j]), int(length[0, j]))
    raise AssertionError("no time mask whose move changes the masked frames")


@pytest.mark.parametrize("name", NAMES)
def test_training_step_with_everything_live_vs_oracle(name, monkeypatch):
    from mamba_asr_amd import ops
    from mamba_asr_amd.brain import Stage
    hp, br, cfg = _brain(name)
    batch = wavs, lens, tokens, tok_lens = _batch()
    norm = hp["normalize"]
    assert next(iter(hp["epoch_counter"])) == 1 and hp["epoch_counter"].current == 1
    br.modules.train()
    assert cfg.transformer_dropout == hp["transformer_dropout"] == 0.1 and hp["CNN"].blocks[0].drop.p == 0.1

    def run(autocast):
        norm.count, norm.glob_mean, norm.glob_std = 0, torch.zeros(1, device=DEV), torch.ones(1, device=DEV)   # the first batch sets them
        calls, real = [], ops.spec_drop_

        def spec_drop(feats, start, length, dim, fill):                       # the fill value is NOT recorded: the oracle uses its own
            calls.append((start.detach().cpu().long().clone(), length.detach().cpu().long().clone(), int(dim)))
            return real(feats, start, length, dim, fill)
        monkeypatch.setattr(ops, "spec_drop_", spec_drop)                     # undone by _gpu_step with its own patches
        step = lambda: br.compute_objectives(br.compute_forward(batch, Stage.TRAIN), batch, Stage.TRAIN)
        loss, grads, names, seeds, cnn, src, tdrop = L._gpu_step(br.modules, wavs, lens, tokens, tok_lens, autocast, monkeypatch, step=step)
        assert ops.spec_drop_ is real
        assert norm.count == 1 and norm.glob_mean.shape == (hp["n_mels"],)
        assert [c[2] for c in calls] == [1, 2], calls                         # one time drop, one frequency drop, in the recipe's order
        assert 1 <= calls[0][0].shape[1] <= 5 and 1 <= calls[1][0].shape[1] <= 3
        x_in = src[0][0]
        rows, t = x_in.shape[0] * x_in.shape[1], x_in.shape[1]
        masks = L._masks(br.modules, seeds, cnn, src, tdrop, rows, t, cfg=cfg)
        for k, v in masks.items():
            kept = float((v != 0).double().mean())
            assert 0.8 < kept < 0.97, (k, kept)                               # every site really drops
        return loss, grads, names, calls, masks, tdrop

    def oracle(calls, masks):
        stats = {}
        ref_loss, ref = L._oracle(cfg, br.modules, wavs, lens, tokens, tok_lens, masks, features=_oracle_features(calls, lens, stats),
                                  reduction=hp["loss_reduction"])
        return ref_loss, ref, stats

    # ---- fp32
    loss, grads, names, calls, masks, tdrop = run(False)
    got_mean, got_std = norm.glob_mean.double().cpu(), norm.glob_std.double().cpu()
    print(f"{name} live step, fp32: launched {sorted(names)}")
    assert "cm_spec_drop" in names and "cm_ctc_loss" in names, sorted(names)
    ref_loss, ref, stats = oracle(calls, masks)
    assert set(grads) == set(ref), sorted(set(grads) ^ set(ref))
    bad = L._fp32_failures(loss, grads, ref_loss, ref)
    errs = {k: L.rel_l2(grads[k], ref[k]) for k in ref}
    d = abs(float(loss) - float(ref_loss))
    print(f"{name} live step, fp32: CTC oracle(fp64) {float(ref_loss):.6f} gpu {float(loss):.6f}, |delta| {d:.2e} ({d / 1e-3:.3f} of the bound); "
          f"worst gradient relative L2 {max(errs.values()):.2e} ({max(errs.values()) / 2e-3:.3f} of the bound, {max(errs, key=errs.get)})")
    assert not bad, bad
    # the normaliser's first-batch statistics against the oracle's own
    bound = norm_stats_bound(wavs.shape[1] // 160 + 1, updates=1)
    e_mean = float((got_mean - stats["mean"]).abs().max()) / stats["scale"]
    e_std = float((got_std - stats["std"]).abs().max()) / float(stats["std"].max())
    print(f"{name} live step: normaliser statistics vs the oracle's: mean {e_mean:.2e} ({e_mean / bound:.3f} of the bound {bound:.2e}), "
          f"std {e_std:.2e} ({e_std / bound:.3f})")
    assert e_mean <= bound and e_std <= bound
    # ---- negative controls (CPU): one time mask one frame later; no SpecAugment at all
    moved, (s0, l0) = _moved(calls, wavs.shape[1] // 160 + 1)
    nl, nref, _ = oracle(moved, masks)
    nbad = L._fp32_failures(loss, grads, nl, nref)
    print(f"  negative control (time mask at frame {s0}, {l0} long, moved to {s0 + 1}): {len(nbad)} comparisons fail, e.g. {list(nbad)[:3]}")
    assert nbad
    nl, nref, _ = oracle([], masks)
    nbad = L._fp32_failures(loss, grads, nl, nref)
    print(f"  negative control (masks dropped altogether): {len(nbad)} comparisons fail, e.g. {list(nbad)[:3]}")
    assert "loss" in nbad and len(nbad) > len(ref) // 2
    # ---- bf16 autocast, the recipe's precision: fresh statistics, fresh draws
    loss_bf, grads_bf, names, calls, masks, tdrop = run(True)
    print(f"{name} live step, bf16: launched {sorted(names)}; module-tree dropout sites: {sorted(tdrop)}")
    assert "cm_spec_drop" in names and "cm_ctc_loss" in names, sorted(names)
    ref_loss, ref, stats = oracle(calls, masks)
    assert set(grads_bf) == set(ref), sorted(set(grads_bf) ^ set(ref))
    dbf = abs(float(loss_bf) - float(ref_loss))
    errs = {k: L.rel_l2(grads_bf[k], ref[k]) for k in ref}
    print(f"{name} live step, bf16 autocast: oracle {float(ref_loss):.6f} gpu {float(loss_bf):.6f}, relative {dbf / abs(float(ref_loss)):.2e} "
          f"({dbf / (2e-3 * abs(float(ref_loss))):.3f} of the bound); gradients: median rel L2 {sorted(errs.values())[len(errs) // 2]:.2e}, "
          f"max {max(errs.values()):.2e} ({max(errs.values()) / 6e-2:.3f} of the bound, {max(errs, key=errs.get)})")
    assert dbf <= 2e-3 * abs(float(ref_loss))
    bad = {k: round(v, 4) for k, v in errs.items() if v > 6e-2}
    assert not bad, bad


@pytest.mark.parametrize("name", NAMES)
def test_loop_eager_and_graphed(name, monkeypatch):
    """8 micro-batches of two shapes at the recipe's accumulation of 4, transformer_dropout 0.0 and SpecAugment on (it runs in the
    prologue in both modes: the same torch seeds give the same draws).  The criteria for losses and parameters are
    test_graph_train.test_graphed_brain_trains_like_the_eager_one's."""
    from mamba_asr_amd import ops
    batches = [_batch(), _batch(batch=3, frames=236, n_tok=8, seed=77, lens=(1.0, 0.9, 0.75), tok_lens=(1.0, 0.75, 0.5))]
    order = [0, 0, 0, 1, 1, 0, 1, 0]              # shape 0: eager, capture, replay; shape 1 enters on the stepping micro-batch
    draws = []
    draw = ops.draw_seed
    monkeypatch.setattr(ops, "draw_seed", lambda: (draws.append(1), draw())[1])
    replays = []
    replay = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), replay(self))[1])
    try:
        runs = []
        for graph in (False, True):
            hp, br, cfg = _brain(name, graph=graph, transformer_dropout=0.0)
            assert br.grad_accumulation_factor == 4 and br.precision == "bf16"
            br.on_fit_start()
            epoch = next(iter(hp["epoch_counter"]))
            assert epoch == 1
            br.modules.train()
            torch.manual_seed(hp["seed"] + epoch)
            losses, lrs, pure_replays = [], [], 0
            for n, i in enumerate(order):
                n_draws, n_replays, captured = len(draws), len(replays), sum(len(v) for v in br._graphs.values())
                losses.append(float(br.fit_batch(batches[i])))
                if len(replays) > n_replays and sum(len(v) for v in br._graphs.values()) == captured:
                    pure_replays += 1
                    assert len(draws) == n_draws, "a replay drew a dropout seed on the host"
                if (n + 1) % 4 == 0:
                    lrs.append(br.optimizer.param_groups[0]["lr"])
            runs.append((losses, [p.detach().clone() for p in br.modules.parameters()], br, hp, lrs, pure_replays))
        (l_e, p_e, be, he, lr_e, r_e), (l_g, p_g, bg, hg, lr_g, r_g) = runs
        assert be.optimizer_step == 2 and bg.optimizer_step == 2
        assert r_e == 0 and r_g >= 3, (r_e, r_g)
        assert len(bg._graphs) == 2 and any(set(v) == {"fresh", "warm"} for v in bg._graphs.values()), {k: set(v) for k, v in bg._graphs.items()}
        lr0, warm = hg["lr_model"], hg["n_warmup_steps"]
        want = [lr0 * warm ** 0.5 * min(n ** -0.5, n * warm ** -1.5) for n in (1, 2)]      # NoamScheduler's closed form
        assert lr_e == lr_g and lr_g == pytest.approx(want, rel=1e-12), (lr_e, lr_g, want)
        assert he["noam_annealing"].n_steps == hg["noam_annealing"].n_steps == 2
        assert he["normalize"].count == 8 and hg["normalize"].count == 8      # epoch 1 < update_until_epoch: every micro-batch updates
        worst_l = max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(l_e, l_g))
        worst_p = max(float((a - b).abs().max()) for a, b in zip(p_e, p_g))
        print(f"{name} loop: eager losses {[round(x, 3) for x in l_e]}, graphed {[round(x, 3) for x in l_g]}; worst relative loss difference "
              f"{worst_l:.2e} (bound 2e-3), worst parameter difference {worst_p:.2e} (bound 5e-4); {r_g} pure replays; lr {lr_g}")
        for a, b in zip(l_e, l_g):
            assert abs(a - b) <= 2e-3 * max(1.0, abs(a)), (l_e, l_g)
        assert l_g[-1] < l_g[0]                                               # it trains (first and last micro-batch are the same batch)
        assert worst_p < 5e-4, worst_p
    finally:
        ops.SEED_EPOCH = None


def test_test_stage_beam_search_from_the_recipe_keywords():
    """Stage.TEST on the large recipe (the one with test_beam_search): the searcher built from the YAML's keywords returns, on the
    recipe's own p_ctc, what tests/ctc_beam_ref.py returns for the same log-probabilities and keywords."""
    import ctc_beam_data as D
    from test_ctc_beam_search_gpu import _match, _ref
    from mamba_asr_amd.brain import Stage
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    hp, br, cfg = _brain("conmamba_large_ctc", vocab_list=D.SPM_VOCAB)
    assert hp["test_beam_search"] == D.RECIPE
    batch = wavs, lens, tokens, tok_lens = _batch()
    with torch.no_grad():
        hp["normalize"].update_statistics(hp["compute_features"](wavs), lens)
        hp["ctc_lin"].w.weight.mul_(3.0)          # a freshly initialised head is near uniform: sharpen it so that the beam has candidates
    br.modules.eval()
    with torch.no_grad():
        p_ctc, _, hyps = br.compute_forward(batch, Stage.TEST)
    s = br.test_searcher
    assert isinstance(s, CTCBeamSearcher) and s.vocab_list == list(D.SPM_VOCAB)
    for k, v in hp["test_beam_search"].items():
        assert getattr(s, k) == v, k
    assert len(hyps) == 2
    lp = p_ctc.float().cpu()
    frames = [75, 60]                                                         # round(1.0 * 75), round(0.8 * 75)
    for b, n in enumerate(frames):
        _match(hyps[b], _ref(s, lp[b], n))
    print(f"TEST stage: {[h[0].text for h in hyps]} scores {[round(h[0].score, 3) for h in hyps]}")
    assert any(h[0].text for h in hyps)
