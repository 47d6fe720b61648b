"""ops.attn_step (cm_attn_step) on the GPU against an fp64 restatement on the same, already rounded inputs.

Tolerance (the convention of DESIGN.md §4d): 4 x the distance of ops.attn_step_torch (same I/O dtype, fp32 arithmetic) from fp64 on
those inputs, and not less than one ulp of the output dtype at max|reference|.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
R = 5
T_CASES = [0, 1, 63, 64, 65, 130]                                  # the edges of a 64-lane pass over the positions
VARIANTS = ["random", "one_row", "peaked", "flat"]


def _ref64(qkv, kc, vc, anc, t, H):
    """The contract in fp64, one (row, head) at a time; a position whose ancestor is outside [0, R) is left out."""
    Rn, D = qkv.shape[0], qkv.shape[1] // 3
    dh = D // H
    q, k, v = (x.double().cpu() for x in qkv.split(D, dim=1))
    kc, vc, anc = kc.double().cpu(), vc.double().cpu(), anc.cpu().tolist()
    out = torch.zeros(Rn, D, dtype=torch.float64)
    for r in range(Rn):
        keep = [s for s in range(t) if 0 <= anc[s][r] < Rn]
        for h in range(H):
            sl = slice(h * dh, (h + 1) * dh)
            K = torch.stack([kc[s, anc[s][r], sl] for s in keep] + [k[r, sl]])
            Vv = torch.stack([vc[s, anc[s][r], sl] for s in keep] + [v[r, sl]])
            out[r, sl] = torch.softmax(K @ q[r, sl] / math.sqrt(dh), dim=0) @ Vv
    return out


def _ulp(dtype, m):
    return 2.0 ** (math.floor(math.log2(m)) - (23 if dtype == torch.float32 else 7))


def _case(H, dh, t, dtype, variant, seed=0, R=R):
    g = torch.Generator().manual_seed(seed * 7919 + H * 1000 + t * 10 + VARIANTS.index(variant))
    D, Lcap = H * dh, t + 3
    qkv = torch.randn(R, 3 * D, generator=g)
    kc, vc = torch.randn(Lcap, R, D, generator=g), torch.randn(Lcap, R, D, generator=g)
    anc = torch.randint(0, R, (Lcap, R), generator=g).int()
    if variant == "one_row":
        anc[:] = R - 2                                             # every row's whole prefix lives in one row (3 of 5)
    if variant == "flat":
        kc.zero_()
        qkv[:, D:2 * D] = 0.0                                      # every score is 0
    if variant == "peaked":
        kc.mul_(0.02)
        qkv[:, D:2 * D] *= 0.02
        q = qkv[:, :D].view(R, H, dh)
        peak = (q * (30.0 * math.sqrt(dh) / (q * q).sum(-1, keepdim=True))).reshape(R, D)   # q . peak / sqrt(dh) = 30
        if t == 0:
            qkv[:, D:2 * D] = peak
        else:
            s = t // 2
            anc[s] = torch.arange(R, dtype=torch.int32)
            kc[s] = peak
    kc[t:], vc[t:] = float("nan"), float("nan")                    # nothing at or behind position t may be read
    return qkv.to(dtype).to(DEV), kc.to(dtype).to(DEV), vc.to(dtype).to(DEV), anc.to(DEV)


def _check(H, dh, t, dtype, variant, R=R):
    from mamba_asr_amd import ops
    qkv, kc, vc, anc = _case(H, dh, t, dtype, variant, R=R)
    D = H * dh
    ref = _ref64(qkv, kc, vc, anc, t, H)
    kt, vt = kc.clone(), vc.clone()
    base = ops.attn_step_torch(qkv, kt, vt, anc, t, H)
    k1, v1 = kc.clone(), vc.clone()
    out = ops.attn_step(qkv, k1, v1, anc, t, H)
    torch.cuda.synchronize()
    assert out.dtype == dtype and out.shape == (R, D) and not bool(torch.isnan(out).any())
    d_torch = float((base.double().cpu() - ref).abs().max())
    d_native = float((out.double().cpu() - ref).abs().max())
    tol = max(4.0 * d_torch, _ulp(dtype, float(ref.abs().max())))
    print(f"R {R} H {H} dh {dh} t {t} {str(dtype)[6:]} {variant}: |native - fp64| {d_native:.3e}, |torch - fp64| {d_torch:.3e}, "
          f"tolerance {tol:.3e}, max|ref| {float(ref.abs().max()):.3f}")
    assert d_native <= tol
    # position t holds the bits of this step's k and v, and nothing else was written
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(k1[t].view(bits), qkv[:, D:2 * D].contiguous().view(bits))
    assert torch.equal(v1[t].view(bits), qkv[:, 2 * D:].contiguous().view(bits))
    keep = [s for s in range(kc.shape[0]) if s != t]
    assert torch.equal(k1[keep].view(bits), kc[keep].view(bits)) and torch.equal(v1[keep].view(bits), vc[keep].view(bits))
    assert torch.equal(k1.view(bits), kt.view(bits)) and torch.equal(v1.view(bits), vt.view(bits))
    # bit-identical from run to run
    again = ops.attn_step(qkv, kc.clone(), vc.clone(), anc, t, H)
    assert torch.equal(again.view(bits), out.view(bits))
    return qkv, kc, vc, anc, out, bits


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("t", T_CASES)
@pytest.mark.parametrize("H,dh", [(2, 32), (3, 64)])
def test_attn_step_matches_fp64(H, dh, t, dtype):
    for variant in VARIANTS:
        _check(H, dh, t, dtype, variant)


# A workgroup is 4 waves up to 1024 score slots, 2 up to 2048, 1 beyond; 4095 is the last t the contract takes.  R * H = 9 leaves
# the last 2-wave workgroup one idle wave.
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("t,R_,H,dh", [(1023, 3, 3, 32), (1024, 3, 3, 32), (1100, 3, 3, 32), (2047, 2, 2, 64), (2100, 2, 2, 64),
                                       (4095, 2, 2, 32)])
def test_long_prefixes_with_two_and_one_wave_per_workgroup(t, R_, H, dh, dtype):
    for variant in VARIANTS:
        _check(H, dh, t, dtype, variant, R=R_)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,dh", [(2, 32), (3, 64)])
def test_a_row_alone_equals_the_row_among_five(H, dh, dtype):
    from mamba_asr_amd import ops
    t = 65
    qkv, kc, vc, anc, out, bits = _check(H, dh, t, dtype, "random")
    for r in (0, 4):
        take = anc[:, r].long().view(-1, 1, 1).expand(-1, 1, H * dh)
        k1, v1 = kc.gather(1, take).contiguous(), vc.gather(1, take).contiguous()        # (Lcap, 1, D): the lines row r's column names
        alone = ops.attn_step(qkv[r:r + 1].contiguous(), k1, v1, torch.zeros_like(anc[:, :1]).contiguous(), t, H)
        assert torch.equal(alone.view(bits), out[r:r + 1].view(bits))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,dh", [(2, 32), (3, 64)])
def test_an_out_of_range_ancestor_contributes_nothing(H, dh, dtype):
    """The expected output is the restatement with those positions removed (_ref64 leaves them out)."""
    from mamba_asr_amd import ops
    t = 70
    qkv, kc, vc, anc = _case(H, dh, t, dtype, "random", seed=1)
    anc[3, 0], anc[64, 0], anc[10, 2], anc[69, 4], anc[0, 4] = -1, R, 2 ** 31 - 1, -2 ** 31, R + 1
    anc[t] = 2 ** 30                                               # anc[t] is not read
    ref = _ref64(qkv, kc, vc, anc, t, H)
    base = ops.attn_step_torch(qkv, kc.clone(), vc.clone(), anc, t, H)
    out = ops.attn_step(qkv, kc.clone(), vc.clone(), anc, t, H)
    torch.cuda.synchronize()
    d_torch, d_native = float((base.double().cpu() - ref).abs().max()), float((out.double().cpu() - ref).abs().max())
    tol = max(4.0 * d_torch, _ulp(dtype, float(ref.abs().max())))
    print(f"H {H} dh {dh} {str(dtype)[6:]}: |native - fp64| {d_native:.3e}, |torch - fp64| {d_torch:.3e}, tolerance {tol:.3e}")
    assert not bool(torch.isnan(out).any()) and d_native <= tol


def test_strided_caches_and_refusals():
    from mamba_asr_amd import ops
    H, dh, t = 2, 32, 5
    qkv, kc, vc, anc = _case(H, dh, t, torch.float32, "random", seed=2)
    wide_k, wide_v = (torch.zeros(kc.shape[0], 2 * R, H * dh, device=DEV) for _ in range(2))
    wide_k[:, :R], wide_v[:, :R] = kc, vc
    want = ops.attn_step(qkv, kc.clone(), vc.clone(), anc, t, H)
    got = ops.attn_step(qkv, wide_k[:, :R], wide_v[:, :R], anc, t, H)       # position stride 2 * R * D
    assert torch.equal(got, want) and torch.equal(wide_k[t, :R], qkv[:, H * dh:2 * H * dh]) and not bool(wide_k[:, R:].any())
    with pytest.raises(RuntimeError, match="head dimension 48"):
        ops.attn_step(torch.zeros(R, 3 * 96, device=DEV), torch.zeros(2, R, 96, device=DEV), torch.zeros(2, R, 96, device=DEV),
                      torch.zeros(2, R, dtype=torch.int32, device=DEV), 0, 2)
    with pytest.raises(RuntimeError, match="dtype"):
        ops.attn_step(qkv.half(), kc.half(), vc.half(), anc, t, H)
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.attn_step(qkv, kc, vc, anc, kc.shape[0], H)
