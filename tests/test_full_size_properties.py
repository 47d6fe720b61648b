"""Parity at BASELINE.json's full sizes through size-independent properties (the CPU oracle needs minutes there):
ConMamba-large CTC (18 layers, D=256, E=512, N=16), 40 s utterances (4000 frames -> 1000 scan steps)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def large_model():
    from mamba_asr_amd.asr import CONFIGS, ConMambaASR, samples_for_frames, synthetic_wavs
    cfg = CONFIGS["conmamba_large_ctc"]
    model = ConMambaASR(cfg).to(DEV).eval()
    wavs, lens = synthetic_wavs(6, samples_for_frames(4000), cfg.seed, DEV)
    model.calibrate(wavs, lens)                               # first batch fixes the global normalisation statistics
    return model, wavs, lens


def test_utterances_are_independent_at_full_size(large_model):
    """Each utterance of a 6 x 40 s batch gives bit-identical encoder output when it is encoded alone, in another
    position of the batch, or with fused.N_STREAMS forced to 1: no kernel leaks state across utterances, tile edges
    or workgroup mappings at T = 1000 (63 ragged-tail scan blocks, 251 CNN tiles, 7 scan time chunks).  At 6 utterances the
    default stream setting also runs one part (parts hold at least 16 utterances): the two-part joined route of the benchmark's
    64 x 40 s batch is tested in test_bench_shapes.py."""
    from mamba_asr_amd import fused
    model, wavs, lens = large_model
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        full = model.encode(wavs, lens)
        assert full.shape == (6, 1000, 256) and torch.isfinite(full).all()
        alone = model.encode(wavs[4:5], lens[4:5])
        perm = torch.tensor([3, 5, 0, 4, 1, 2], device=DEV)
        shuffled = model.encode(wavs[perm], lens[perm])
    assert torch.equal(alone[0], full[4])
    assert torch.equal(shuffled, full[perm])
    old = fused.N_STREAMS
    try:
        fused.N_STREAMS = 1
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            single = model.encode(wavs, lens)
    finally:
        fused.N_STREAMS = old
    assert torch.equal(single, full)


def test_time_reversal_of_the_scan_at_full_size():
    """cm_scan_cl_fwd (row-group kernel) at B=8, E=512, T=1000: the reverse_time direction on time-flipped inputs equals
    the flipped forward direction with the same parameters, bit for bit (the recurrence visits the same values in the
    same order) -- the property the reference obtains with explicit .flip() copies (bimamba.py:237, 253).  Bit equality is
    a property of the unchunked launch (time_chunks=1); the chunked launch the size policy picks for this small batch cuts
    the two directions at different steps and agrees to bf16 rounding."""
    from mamba_asr_amd import ops
    b, l, e = 8, 1000, 512
    gen = torch.Generator(device=DEV).manual_seed(7)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    xz = rnd(b, l, 2 * e).bfloat16()
    u = rnd(b, l, e).bfloat16()
    xdbl = (rnd(b, l, 48) * 0.5).bfloat16()
    A = -torch.exp(rnd(e, 16) * 0.06)
    Wdt = ops.pad_dt_weight(rnd(e, 16) * 0.25)
    D, bias = torch.ones(e, device=DEV), rnd(e) - 4
    z = xz[:, :, e:]
    common = dict(A=A, D=D, delta_bias=bias, dt_weight=Wdt)
    (fwd,) = ops.scan_cl_fwd([dict(common, u=u, xdbl=xdbl, reverse=False)], z=z, time_chunks=1)
    flip = lambda t: t.flip(1).contiguous()
    (rev,) = ops.scan_cl_fwd([dict(common, u=flip(u), xdbl=flip(xdbl), reverse=True)], z=flip(z), time_chunks=1)
    assert torch.isfinite(fwd.float()).all()
    assert torch.equal(rev.flip(1), fwd)
    # both directions in one launch == the two single launches
    ycat = torch.empty(b, l, 2 * e, dtype=torch.bfloat16, device=DEV)
    ops.scan_cl_fwd([dict(common, u=u, xdbl=xdbl, reverse=False, out=ycat[:, :, :e]),
                     dict(common, u=flip(u), xdbl=flip(xdbl), reverse=True, out=ycat[:, :, e:])], z=z, time_chunks=1)
    assert torch.equal(ycat[:, :, :e], fwd)
    # (the second direction above was gated with the un-flipped z; check it against its own single launch)
    (rev2,) = ops.scan_cl_fwd([dict(common, u=flip(u), xdbl=flip(xdbl), reverse=True)], z=z, time_chunks=1)
    assert torch.equal(ycat[:, :, e:], rev2)
    # the chunked launch (what the size policy picks at 8 x 1000 x 512)
    from mamba_asr_amd import _native
    assert _native.lib().cm_scan_cl_fwd_auto_chunks(b, l, e, 1) > 1
    (cut,) = ops.scan_cl_fwd([dict(common, u=u, xdbl=xdbl, reverse=False)], z=z)
    torch.testing.assert_close(cut.float(), fwd.float(), rtol=8e-3, atol=1e-3)
    (cutr,) = ops.scan_cl_fwd([dict(common, u=flip(u), xdbl=flip(xdbl), reverse=True)], z=flip(z))
    torch.testing.assert_close(cutr.flip(1).float(), fwd.float(), rtol=8e-3, atol=1e-3)


@pytest.mark.parametrize("b,l,e,P", [(4, 4000, 1024, 32), (16, 1000, 512, 16)])
def test_backward_scan_time_chunks_at_full_size(b, l, e, P):
    """cm_scan_cl_bwd at BASELINE config 5's per-GPU size (4 x 160 s, E 1024, dt_rank 32: 128 workgroups, the library cuts it into
    8 time chunks) and at SURVEY's 16 x 40 s: the cut launch (adjoint summaries per chunk, carry fold, full pass from the
    carried-in adjoints) against the one-pass launch on the same inputs -- every output within bf16 rounding, parameter gradients
    within 2e-3 of their scale; utterances independent (utterance 1 alone == utterance 1 of the batch at the same chunk count, bit for bit)."""
    from mamba_asr_amd import ops, _native as N
    g = torch.Generator(device=DEV).manual_seed(b + l)
    rnd = lambda *s: torch.randn(*s, device=DEV, generator=g)
    dt, RW = torch.bfloat16, P + 32
    xz, ucat = rnd(b, l, 2 * e).to(dt), rnd(b, l, 2 * e).to(dt)
    xcat, dmix = (rnd(b, l, 2 * RW) * 0.5).to(dt), rnd(b, l, e).to(dt)
    z = xz[:, :, e:]
    params = [dict(A=-torch.exp(rnd(e, 16) * 0.06), D=torch.ones(e, device=DEV), delta_bias=rnd(e) - 4, dt_weight=ops.pad_dt_weight(rnd(e, P) * 0.25)) for _ in range(2)]

    def run(sl, chunks):
        bb = ucat[sl].shape[0]
        ycat = torch.empty(bb, l, 2 * e, device=DEV, dtype=dt)
        pcat = torch.empty(bb, l, 2 * e, device=DEV, dtype=dt)
        dirs = [dict(u=ucat[sl][:, :, e * i:e * (i + 1)], xdbl=xcat[sl][:, :, RW * i:RW * (i + 1)], reverse=bool(i), out=ycat[:, :, e * i:e * (i + 1)],
                     ypre=pcat[:, :, e * i:e * (i + 1)], ckpt=torch.empty(ops.scan_ckpt_shape(bb, l, e), device=DEV), **params[i]) for i in range(2)]
        ops.scan_cl_fwd(dirs, z=z[sl], time_chunks=1)
        for d in dirs:
            d["dout"] = dmix[sl]
        return ops.scan_cl_bwd(dirs, z[sl], time_chunks=chunks)

    assert N.lib().cm_scan_cl_bwd_auto_chunks(b, l, e, 2) > 1
    cut, one = run(slice(0, b), 0), run(slice(0, b), 1)
    for c, o in zip(cut, one):
        for k in ("du", "dz", "dxdbl"):
            err = float((c[k].float() - o[k].float()).abs().max()) / max(1.0, float(o[k].float().abs().max()))
            assert err < 2e-2, (k, err)
        for k in ("dA", "ddt_weight", "dD", "ddelta_bias"):
            err = float((c[k] - o[k]).abs().max()) / max(1e-6, float(o[k].abs().max()))
            assert err < 2e-3, (k, err)
    # (the automatic chunk count depends on the batch: fix it for the independence check)
    nck = N.lib().cm_scan_cl_bwd_auto_chunks(b, l, e, 2)
    both, alone = run(slice(0, b), nck), run(slice(1, 2), nck)
    for c, a in zip(both, alone):
        for k in ("du", "dz", "dxdbl"):
            assert torch.equal(c[k][1:2], a[k]), k
