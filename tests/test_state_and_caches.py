"""Host-side state handling (CPU): the normaliser's statistics survive a state_dict round trip and stay frozen in eval
(sb_compat.InputNormalization), weight-copy caches notice `.data` swaps, unsupported TransformerASR
configurations fail loudly."""
import pytest
import torch

from mamba_asr_amd import ops, weight_cache
from mamba_asr_amd import sb_compat as sb


def _feats(seed, b=3, t=50, f=8):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(b, t, f, generator=g) * 2.0 + 1.0, torch.tensor([1.0, 0.8, 0.6])[:b]


def test_input_normalization_round_trip_and_eval_freeze():
    n = sb.InputNormalization(norm_type="global", update_until_epoch=4).train()
    x1, l1 = _feats(1)
    y_train = n(x1, l1, epoch=0)
    assert n.count == 1 and n.glob_mean.shape == (8,)
    mean, std = n.glob_mean.clone(), n.glob_std.clone()
    torch.testing.assert_close(y_train, (x1 - mean) / std)
    sd = n.state_dict()
    assert int(sd["count_buf"]) == 1
    fresh = sb.InputNormalization(norm_type="global", update_until_epoch=4).eval()
    fresh.load_state_dict(sd, strict=True)                      # (1,) placeholder buffers take the checkpoint's shape
    assert fresh.count == 1
    x2, l2 = _feats(2)
    y = fresh(x2, l2, epoch=0)                                  # a different batch, eval: statistics must not move
    torch.testing.assert_close(fresh.glob_mean, mean)
    torch.testing.assert_close(fresh.glob_std, std)
    torch.testing.assert_close(y, (x2 - mean) / std)
    assert fresh.count == 1
    # training resumes the running average where it stopped (weight 1 / (count + 1))
    fresh.train()
    fresh(x2, l2, epoch=0)
    assert fresh.count == 2 and not torch.allclose(fresh.glob_mean, mean)
    # beyond update_until_epoch the statistics are frozen in training too
    m2 = fresh.glob_mean.clone()
    fresh(x1, l1, epoch=4)
    torch.testing.assert_close(fresh.glob_mean, m2)


def test_input_normalization_eval_before_any_update_is_identity():
    n = sb.InputNormalization(norm_type="global").eval()
    x, l = _feats(3)
    torch.testing.assert_close(n(x, l), x)                      # mean 0 / std 1 until something updates them
    assert n.count == 0
    n.update_statistics(x, l)                                   # the explicit calibration entry point
    assert n.count == 1 and n.glob_mean.shape == (8,)


def test_whole_model_state_dict_round_trip_keeps_fused_path_eligible():
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR
    cfg = ASRConfig("tiny", d_model=32, d_ffn=64, num_encoder_layers=1, n_fft=400, seed=3)
    a = ConMambaASR(cfg).train()
    x, l = _feats(4, b=2, t=30, f=80)
    a.normalize(x, l[:2], epoch=0)
    b = ConMambaASR(cfg).eval()
    b.load_state_dict(a.state_dict(), strict=True)
    assert b.normalize.count == 1                               # asr.encode's fused-path condition (count > 0) holds
    torch.testing.assert_close(b.normalize.glob_mean, a.normalize.glob_mean)


def test_cast_cache_sees_data_swap_and_invalidate():
    p = torch.nn.Parameter(torch.randn(4, 4))
    c1 = ops.cast_cached(p, torch.bfloat16)
    assert ops.cast_cached(p, torch.bfloat16) is c1
    p.data = torch.randn(4, 4)                                  # storage swap: _version unchanged, data_ptr changes
    c2 = ops.cast_cached(p, torch.bfloat16)
    torch.testing.assert_close(c2.float(), p.detach().to(torch.bfloat16).float())
    p.data.copy_(torch.randn(4, 4))                             # write THROUGH .data: invisible -> invalidate_caches
    lin = torch.nn.Linear(4, 4)
    lin.weight = p
    ops.invalidate_caches(lin)
    c3 = ops.cast_cached(p, torch.bfloat16)
    torch.testing.assert_close(c3.float(), p.detach().to(torch.bfloat16).float())
    with torch.no_grad():
        p.add_(1.0)                                             # in-place on the parameter itself: version bump
    torch.testing.assert_close(ops.cast_cached(p, torch.bfloat16).float(), p.detach().to(torch.bfloat16).float())


def test_inplace_cache_mode_keeps_storage_and_tracks_generations():
    """weight_cache.CACHE_INPLACE (what a graphed training loop runs under: captured launches hold the caches' ADDRESSES): a stale entry is
    refreshed in its own storage; forced_refresh() re-derives every entry once and lists what it refreshed; rekey_caches marks exactly
    those entries current; CACHE_GENERATION moves only when an entry gets new storage or entries are dropped."""
    p = torch.nn.Parameter(torch.randn(6, 4))
    q = torch.nn.Parameter(torch.randn(3, 4))
    old = weight_cache.CACHE_INPLACE
    try:
        weight_cache.CACHE_INPLACE = True
        g0 = weight_cache.CACHE_GENERATION
        c1 = ops.cast_cached(p, torch.bfloat16)
        assert weight_cache.CACHE_GENERATION == g0 + 1              # first sight: new storage
        with torch.no_grad():
            p.mul_(2.0)
        c2 = ops.cast_cached(p, torch.bfloat16)
        assert c2 is c1 and weight_cache.CACHE_GENERATION == g0 + 1  # refreshed in place
        torch.testing.assert_close(c2.float(), p.detach().to(torch.bfloat16).float())
        ops.cast_cached(q, torch.bfloat16)
        g1 = weight_cache.CACHE_GENERATION
        with weight_cache.forced_refresh() as log:
            assert ops.cast_cached(p, torch.bfloat16) is c1         # current key, refreshed anyway (a capture records the kernel) ...
            assert ops.cast_cached(p, torch.bfloat16) is c1         # ... once
        assert [(o is p, a) for o, a in log] == [(True, "_cm_cast")] and weight_cache.CACHE_GENERATION == g1
        with torch.no_grad():
            p.add_(1.0)
            q.add_(1.0)
        c1.copy_(p.detach())                                        # what a replay of the captured refresh does to p's entry only
        weight_cache.rekey_caches(log)
        assert p._cm_cast[0] == (p._version, p.data_ptr())          # p's entry is current again ...
        assert q._cm_cast[0] != (q._version, q.data_ptr())          # ... q's, which no replay refreshed, still counts as stale
        torch.testing.assert_close(ops.cast_cached(q, torch.bfloat16).float(), q.detach().to(torch.bfloat16).float())
        lin = torch.nn.Linear(4, 6)
        lin.weight = p
        ops.invalidate_caches(lin)
        assert weight_cache.CACHE_GENERATION == g1 + 1 and not hasattr(p, "_cm_cast")
        # a module-owned entry keyed on all of its module's parameters (the mixers' derived operands) follows the same protocol
        from mamba_asr_amd import fused
        from mamba_asr_amd.asr import ASRConfig, ConMambaASR
        from mamba_asr_amd.modules.mamba import mixer_rows
        model = ConMambaASR(ASRConfig("tiny", d_model=32, d_ffn=64, num_encoder_layers=1, n_fft=400, seed=3))
        m = model.Transformer.encoder.layers[0].mamba
        derived = lambda: mixer_rows._derived(m, ("", "_b"), torch.float32, 0.5)
        d1 = derived()
        g2 = weight_cache.CACHE_GENERATION
        # (probes: w_out and A are tensors of their own; in fp32 w_in IS in_proj's weight and would prove nothing)
        with torch.no_grad():
            m.out_proj.weight.mul_(2.0)
        assert derived() is d1 and weight_cache.CACHE_GENERATION == g2 and torch.equal(d1.w_out, m.out_proj.weight.detach() * 0.5)
        with weight_cache.forced_refresh() as log:
            assert derived() is d1 and derived() is d1
        assert [(o is m, a) for o, a in log] == [(True, "_cm_rows_derived")] and weight_cache.CACHE_GENERATION == g2
        with torch.no_grad():
            m.out_proj.weight.add_(1.0)
        d1.A[0].zero_()
        assert derived() is d1 and d1.A[0].any()                    # stale: refreshed, A rewritten
        with torch.no_grad():
            m.out_proj.weight.add_(1.0)
        weight_cache.rekey_caches(log)                              # as after a replay of the captured refresh ...
        d1.A[0].zero_()
        assert derived() is d1 and not d1.A[0].any()                # ... the entry counts as current: a hit, nothing rewritten
        # the fused inference path's bundles are rebuilt on a miss without moving the generation (an evaluation pass must not make a
        # training loop drop its graphs) and take no part in a forced refresh
        bias = model.CNN.blocks[1].conv.bias
        f1 = fused._frontend_cache(model, torch.bfloat16)
        assert fused._frontend_cache(model, torch.bfloat16) is f1
        with torch.no_grad():
            bias.add_(1.0)
        with weight_cache.forced_refresh() as log:
            f2 = fused._frontend_cache(model, torch.bfloat16)
            assert fused._frontend_cache(model, torch.bfloat16) is f2
        assert f2 is not f1 and f2["b2"].data_ptr() != bias.data_ptr() and torch.equal(f2["b2"], bias.detach().to(torch.bfloat16)) and log == []
        assert not torch.equal(f1["b2"], f2["b2"]) and weight_cache.CACHE_GENERATION == g2
        ops.invalidate_caches(model)
        assert weight_cache.CACHE_GENERATION == g2 + 1 and not hasattr(model, "_cm_frontend_cache") and not hasattr(m, "_cm_rows_derived")
    finally:
        weight_cache.CACHE_INPLACE = old


def test_transformer_asr_rejects_unimplemented_attention_type():
    from mamba_asr_amd.modules.TransformerASR import TransformerASR
    cfg = {"d_state": 16, "expand": 2, "d_conv": 4, "bidirectional": True}
    with pytest.raises(NotImplementedError):
        TransformerASR(tgt_vocab=31, input_size=640, d_model=32, num_encoder_layers=1, num_decoder_layers=0, d_ffn=64,
                       encoder_module="conmamba", normalize_before=True, causal=False, mamba_config=cfg)   # default regularMHA
    TransformerASR(tgt_vocab=31, input_size=640, d_model=32, num_encoder_layers=1, num_decoder_layers=0, d_ffn=64,
                   encoder_module="conmamba", attention_type="RelPosMHAXL", normalize_before=True, causal=False, mamba_config=cfg)
