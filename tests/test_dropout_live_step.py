"""The whole-model training step with every dropout site LIVE, against the oracle's fp64 autograd on the SAME masks.

tests/test_hip_parity_r3.py pins the step in eval mode (every dropout off).  Here the model runs in train mode (normalisation
statistics frozen) at transformer_dropout 0.1 and the CNN front end's Dropout2d at its default 0.1:
  * the seeds of the native dropout sites (both dropouts of every feed-forward module, the convolution module's last one) are
    recorded by wrapping ops.draw_seed and turned into masks by the HOST restatement of the stream (oracle drop_keep) -- in fp32
    the library FFN route with stored masks, under bf16 autocast the fused cm_ffn_fused / cm_ffn_bwd_fused route that re-derives
    them; no mask is read back from a kernel under test;
  * the torch-drawn masks (the CNN blocks' per-(sample, channel) factors handed to ops.LnActDropFn, the src module's nn.Dropout)
    are captured at test level;
  * the loss and every parameter gradient are compared with the bounds of the eval-mode test;
  * negative control (CPU): the oracle rerun with ONE site's mask taken at the wrong graph-replay epoch fails the same comparison.
"""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAYERS = 2


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def _case(batch=2, frames=300, seed=3502):
    from dataclasses import replace
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = replace(CONFIGS["conmamba_large_ctc"], num_encoder_layers=LAYERS, transformer_dropout=0.1)
    model = ConMambaASR(cfg).to(DEV)
    wavs, _ = synthetic_wavs(batch, samples_for_frames(frames), seed, DEV)
    lens = torch.tensor([1.0, 0.8][:batch], device=DEV)
    for i, r in enumerate(lens.tolist()):
        wavs[i, int(round(r * wavs.shape[1])):] = 0.0
    gen = torch.Generator().manual_seed(seed + 1)
    tokens = torch.randint(1, cfg.output_neurons, (batch, 10), generator=gen)
    tok_lens = torch.tensor([1.0, 0.7][:batch])
    with torch.no_grad():
        model.calibrate(wavs, lens)
    model.train()
    model.normalize.eval()                                  # frozen statistics; every dropout site stays in training mode
    return cfg, model, wavs, lens, tokens, tok_lens


def _site_names():
    """The encoder's dropout sites in forward order (ConmambaEncoderLayer.forward), with the nn.Dropout module behind each."""
    out = []
    for i in range(LAYERS):
        pre = f"Transformer.encoder.layers.{i}."
        out += [(pre + "ffn_module1.drop1", pre + "ffn_module1.1.ffn.2"), (pre + "ffn_module1.drop2", pre + "ffn_module1.2"),
                (pre + "convolution_module.drop", pre + "convolution_module.after_conv.3"),
                (pre + "ffn_module2.drop1", pre + "ffn_module2.1.ffn.2"), (pre + "ffn_module2.drop2", pre + "ffn_module2.2")]
    return out


def _hook_torch_dropouts(model, store):
    """A site that falls back to the module tree (e.g. a layer whose input is not the fp32 residual stream under autocast) runs its
    nn.Dropout module with torch's generator: record that module's output, from which its mask is read.  The native row nodes only
    read the module's p, so their sites record nothing here."""
    mods = dict(model.named_modules())
    return [mods[mod].register_forward_hook(lambda m, i, o, site=site: store.__setitem__(site, (o, m.p))) for site, mod in _site_names()]


def _gpu_step(model, wavs, lens, tokens, tok_lens, autocast, monkeypatch, step=None):
    """One forward + backward; -> (loss, grads, kernel names, seeds in draw order, CNN masks, (src dropout in, out, p)).
    ``step``: a callable returning the loss instead of model.forward_ctc + model.ctc_objective (tests/test_recipe_surface_gpu.py
    runs the recipe's own objects); ``model`` is then any module holding CNN / Transformer / ctc_lin under those names."""
    from mamba_asr_amd import ops
    seeds, cnn, src = [], [], []
    draw = ops.draw_seed
    monkeypatch.setattr(ops, "draw_seed", lambda: (seeds.append(draw()), seeds[-1])[1])
    apply = ops.LnActDropFn.apply

    def ln_act_drop(*args):
        cnn.append(args[5].detach().clone())                # chan_mask (batch, channel), 1 / keep folded in
        return apply(*args)
    monkeypatch.setattr(ops.LnActDropFn, "apply", ln_act_drop)
    drop = [m for m in model.Transformer.custom_src_module.modules() if isinstance(m, nn.Dropout)]
    assert len(drop) == 1
    hook = drop[0].register_forward_hook(lambda m, i, o: src.append((i[0].detach().clone(), o.detach().clone(), m.p)))
    tdrop = {}
    hooks = _hook_torch_dropouts(model, tdrop)
    for p in model.parameters():
        p.grad = None
    ops.LAUNCH_LOG = []
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if step is not None:
                loss = step()
            else:
                logp = model.forward_ctc(wavs, lens)
                loss = model.ctc_objective(logp.float(), tokens.to(DEV), lens, tok_lens.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        names = {e[0] for e in ops.LAUNCH_LOG}
    finally:
        ops.LAUNCH_LOG = None
        hook.remove()
        for h in hooks:
            h.remove()
        monkeypatch.undo()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return loss.detach(), grads, names, seeds, cnn, src, tdrop


def _masks(model, seeds, cnn, src, tdrop, rows, t, epochs=None, cfg=None):
    """Every site's multiplier as an fp64 CPU tensor, keyed as the oracle expects: native sites (in forward order, one seed each)
    from the host restatement, module-tree sites from their recorded nn.Dropout output.  ``epochs`` {site: epoch} overrides the
    epoch the host restatement uses for a site (the negative control).  ``cfg``: for a ``model`` that carries none."""
    from oracle import conmamba_oracle as O
    cfg = model.cfg if cfg is None else cfg
    b = rows // t
    native = [name for name, _ in _site_names() if name not in tdrop]
    assert len(seeds) == len(native), (len(seeds), native)
    m = {}
    p = cfg.transformer_dropout
    for name, s in zip(native, seeds):
        width = cfg.d_ffn if name.endswith("drop1") else cfg.d_model
        e = (epochs or {}).get(name, 0)
        m[name] = O.drop_mask(s, (rows, width), p, epoch=e).view(b, t, width)
    for name, (out, sp) in tdrop.items():
        m[name] = (out != 0).double().cpu().view(b, t, -1) / (1.0 - sp)
    assert len(cnn) == 2, "the CNN blocks did not run the LnActDropFn tail with a mask"
    for i, c in enumerate(cnn):
        m[f"CNN.blocks.{i}.drop"] = c.double().cpu()
    (x_in, x_out, sp), = src
    m["Transformer.custom_src_module.drop"] = (x_out != 0).double().cpu() / (1.0 - sp)
    return m


def _oracle_logp(cfg, model, wavs, masks, features=None):
    """The forward on the CPU in fp64 (Fbank fp32, as in the product), dropout = the given masks (None: eval mode)
    -> (fp64 parameters with requires_grad, log-probabilities).  ``features``: callable (the oracle's fp32 Fbank output) -> the
    normalised, possibly augmented fp64 features; default: normalised with the model's own statistics."""
    from oracle import conmamba_oracle as O
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    p = {k: (v.double().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd.items()}
    feats = O.fbank(wavs.cpu(), n_fft=cfg.n_fft, win_ms=cfg.win_length)
    if features is not None:
        feats = features(feats)
    else:
        feats = ((feats - sd["normalize.glob_mean"]) / sd["normalize.glob_std"]).double()
    src = O.cnn_frontend(p, feats, "CNN.", masks)
    src = O.src_projection(p, src, "Transformer.", masks)
    enc = O.encoder(p, src, LAYERS, "Transformer.encoder.", masks=masks)
    return p, torch.log_softmax(F.linear(enc, p["ctc_lin.w.weight"], p["ctc_lin.w.bias"]), -1)


def _oracle(cfg, model, wavs, lens, tokens, tok_lens, masks, features=None, reduction="batchmean"):
    """The step on the CPU in fp64 (Fbank fp32, as in the product), dropout = the given masks, torch autograd.  ``reduction``:
    the recipe's loss_reduction (speechbrain's ctc_loss: 'batchmean' = sum / batch, 'mean' = sum / target tokens, 'sum')."""
    p, logp = _oracle_logp(cfg, model, wavs, masks, features)
    b, t, _ = logp.shape
    il, tl = torch.round(lens.cpu() * t).int(), torch.round(tok_lens * tokens.shape[1]).int()
    loss = F.ctc_loss(logp.transpose(0, 1), tokens, il, tl, 0, reduction="sum", zero_infinity=True)
    loss = {"batchmean": loss / b, "mean": loss / tl.sum(), "sum": loss}[reduction]
    names = [k for k, _ in model.named_parameters()]
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return loss.detach(), {k: g for k, g in zip(names, grads) if g is not None}


def _fp32_failures(loss, grads, ref_loss, ref):
    """The eval-mode test's fp32 bounds: |loss delta| <= 1e-3, per gradient relative L2 and max element error <= 2e-3."""
    bad = {}
    d = abs(float(loss) - float(ref_loss))
    if d > 1e-3:
        bad["loss"] = d
    for k in ref:
        r = rel_l2(grads[k], ref[k])
        e = float((grads[k].double().cpu() - ref[k]).abs().max() / ref[k].abs().max().clamp_min(1e-30))
        if r > 2e-3 or e > 2e-3:
            bad[k] = (r, e)
    return bad


def test_training_step_with_dropout_live_vs_oracle(monkeypatch):
    cfg, model, wavs, lens, tokens, tok_lens = _case()
    # ---- fp32: the library FFN route, masks stored by cm_bias_act_dropout_fwd
    loss, grads, names, seeds, cnn, src, tdrop = _gpu_step(model, wavs, lens, tokens, tok_lens, False, monkeypatch)
    assert not tdrop, f"fp32: every encoder dropout site should be native (module tree ran: {sorted(tdrop)})"
    for k in ("cm_bias_act_dropout_fwd", "cm_bias_act_dropout_bwd", "cm_layernorm_fwd", "cm_layernorm_bwd"):
        assert k in names, f"{k} did not run in the fp32 step (ran: {sorted(names)})"
    x_in = src[0][0]
    rows, t = x_in.shape[0] * x_in.shape[1], x_in.shape[1]
    masks = _masks(model, seeds, cnn, src, tdrop, rows, t)
    for k, v in masks.items():
        kept = float((v != 0).double().mean())
        assert 0.8 < kept < 0.97, (k, kept)                                        # every site really drops
    ref_loss, ref = _oracle(cfg, model, wavs, lens, tokens, tok_lens, masks)
    assert set(grads) == set(ref), sorted(set(grads) ^ set(ref))
    bad = _fp32_failures(loss, grads, ref_loss, ref)
    errs = {k: rel_l2(grads[k], ref[k]) for k in ref}
    top = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print(f"dropout-live step, fp32: CTC oracle(fp64) {float(ref_loss):.6f} gpu {float(loss):.6f}; worst relative L2: "
          + ", ".join(f"{k} {v:.1e}" for k, v in top))
    assert not bad, bad
    # ---- negative control (CPU): one site's mask at the wrong epoch must fail the same comparison
    wrong = _masks(model, seeds, cnn, src, tdrop, rows, t, epochs={"Transformer.encoder.layers.1.ffn_module1.drop1": 1})
    nl, nref = _oracle(cfg, model, wavs, lens, tokens, tok_lens, wrong)
    nbad = _fp32_failures(loss, grads, nl, nref)
    print(f"  negative control (layer 1 ffn_module1 drop1 at epoch 1): {len(nbad)} comparisons fail, e.g. "
          + ", ".join(f"{k}" for k in list(nbad)[:3]))
    assert any(k.startswith("Transformer.encoder.layers.1.ffn_module1.") for k in nbad), nbad
    # ---- bf16 autocast: the fused route (cm_ffn_fused training forward, cm_ffn_bwd_fused) re-derives the masks from the seeds
    loss_bf, grads_bf, names, seeds, cnn, src, tdrop = _gpu_step(model, wavs, lens, tokens, tok_lens, True, monkeypatch)
    print(f"  bf16: {len(seeds)} native dropout sites, module-tree sites: {sorted(tdrop)}")
    for k in ("cm_ffn_fused", "cm_ffn_bwd_fused", "cm_bias_act_dropout_fwd", "cm_bias_act_dropout_bwd", "cm_layernorm_fwd"):
        assert k in names, f"{k} did not run in the bf16 step (ran: {sorted(names)})"
    masks = _masks(model, seeds, cnn, src, tdrop, rows, t)
    ref_loss, ref = _oracle(cfg, model, wavs, lens, tokens, tok_lens, masks)
    dbf = abs(float(loss_bf) - float(ref_loss))
    errs = {k: rel_l2(grads_bf[k], ref[k]) for k in ref}
    print(f"dropout-live step, bf16 autocast: oracle {float(ref_loss):.6f} gpu {float(loss_bf):.6f} (rel {dbf / abs(float(ref_loss)):.2e}); "
          f"gradients: median rel L2 {sorted(errs.values())[len(errs) // 2]:.2e}, max {max(errs.values()):.2e} ({max(errs, key=errs.get)})")
    assert dbf <= 2e-3 * abs(float(ref_loss))
    bad = {k: round(v, 4) for k, v in errs.items() if v > 6e-2}
    assert not bad, bad


def test_graphed_step_with_dropout_live_vs_oracle(monkeypatch):
    """brain.Brain graph_steps on tests/test_graph_train.py's tiny model (bf16, dropout 0.1): for 3 replays of the captured
    micro-batch the loss against the oracle's fp64 loss on that replay's masks -- the native sites' from the host restatement
    at effective_seed(seed, epoch) with the epoch read from ops.SEED_EPOCH, the torch-drawn ones from the tensors the replay
    wrote -- and, for one replay, every gradient (read before the optimizer step).  Forward and backward of a replay must
    agree on the epoch for this to hold."""
    from mamba_asr_amd import ops
    from test_graph_train import _batches, _tiny_brain
    batch = _batches()[0]
    seeds, cnn, src = [], [], []
    try:
        brain = _tiny_brain(True, dropout=0.1)
        model = brain.modules["asr"]
        model.calibrate(batch[0], batch[1])
        model.normalize.eval()
        for g in brain.optimizer.param_groups:
            g["lr"] = 0.0                                                      # frozen weights: one set of parameters for the oracle
            g["weight_decay"] = 0.0
        brain.max_grad_norm = 1e9                                              # no clipping: the hook sees the raw gradients
        brain.fit_batch(batch)                                                 # first sight: eager
        draw = ops.draw_seed
        monkeypatch.setattr(ops, "draw_seed", lambda: (seeds.append(draw()), seeds[-1])[1])
        apply = ops.LnActDropFn.apply
        monkeypatch.setattr(ops.LnActDropFn, "apply", lambda *a: (cnn.append(a[5]), apply(*a))[1])
        drop = [m for m in model.Transformer.custom_src_module.modules() if isinstance(m, nn.Dropout)][0]
        hook = drop.register_forward_hook(lambda m, i, o: src.append((i[0], o, m.p)))
        tdrop = {}
        hooks = _hook_torch_dropouts(model, tdrop)
        grabbed = {}

        def pre_step(opt, args, kwargs):
            if not grabbed:
                grabbed.update({k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None})
        step_hook = brain.optimizer.register_step_pre_hook(pre_step)
        results = []
        for _ in range(3):
            n_seeds = len(seeds)
            loss = brain.fit_batch(batch)
            assert len(seeds) > 0 and (not results or len(seeds) == n_seeds), "a replay must not draw seeds on the host"
            torch.cuda.synchronize()
            epoch = int(ops.SEED_EPOCH.item())
            # the captured tensors hold what THIS replay wrote: snapshot them before the next one
            results.append((float(loss), epoch, [c.detach().clone() for c in cnn], [(i.detach().clone(), o.detach().clone(), p) for i, o, p in src],
                            {k: (o.detach().clone(), p) for k, (o, p) in tdrop.items()}))
            if len(results) == 1:
                first_grads = dict(grabbed)
        hook.remove()
        for h in hooks:
            h.remove()
        step_hook.remove()
        monkeypatch.undo()
        assert any(brain._graphs.values())
        assert len({r[1] for r in results}) == 3, [r[1] for r in results]       # a fresh epoch per replay
        wavs, lens, tokens, tlens = batch
        x_in = results[0][3][0][0]
        rows, t = x_in.shape[0] * x_in.shape[1], x_in.shape[1]
        from oracle import conmamba_oracle as O
        worst = 0.0
        for i, (loss, epoch, cnn_r, src_r, tdrop_r) in enumerate(results):
            eff = [O.drop_seed(s, epoch) for s in seeds]
            masks = _masks(model, eff, cnn_r, src_r, tdrop_r, rows, t)
            ref_loss, ref = _oracle(model.cfg, model, wavs, lens, tokens.cpu(), tlens.cpu(), masks)
            d = abs(loss - float(ref_loss)) / abs(float(ref_loss))
            worst = max(worst, d)
            assert d <= 2e-3, (i, epoch, loss, float(ref_loss))
            if i == 0:
                errs = {k: rel_l2(first_grads[k], ref[k]) for k in ref}
                bad = {k: round(v, 4) for k, v in errs.items() if v > 6e-2}
                print(f"graphed dropout-live step: replay epoch {epoch}, gradients max rel L2 {max(errs.values()):.2e}")
                assert set(first_grads) == set(ref), sorted(set(first_grads) ^ set(ref))
                assert not bad, bad
        print(f"graphed dropout-live step: 3 replays, losses {[round(r[0], 4) for r in results]}, worst relative loss error {worst:.1e}")
    finally:
        ops.SEED_EPOCH = None
