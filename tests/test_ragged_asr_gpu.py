"""Waveform to hypotheses on a ragged batch (GPU): a 2-layer bidirectional ConMambaASR (d_model 256, bf16), B = 4,
about 1 s of audio, ConMambaASR.encode(wavs, wav_lens, ragged=True).  The samples of wavs at and past every utterance's length are NaN.

  * row_lens is the host arithmetic (fused.frontend_rows_total), as a RowLens with its device tensor;
  * the front-end rows are torch.equal to cm_fbank_wav -> cm_fbank_finish -> cm_cnn_front on each utterance alone;
  * the encoder output meets the bound of tests/test_frontend_streaming_gpu.py::test_end_to_end_wav_to_hypotheses (mean < 2e-3,
    max < 6e-2: the src Linear between front end and encoder is a library GEMM, whose bits depend on the batch) against encode on
    each utterance alone;
  * each utterance against the fp64 oracle (oracle.conmamba_oracle.asr_encode) run on that utterance alone, at the tolerance of the
    existing 2-layer bf16 fused-vs-oracle comparison, tests/test_hip_modules.py::test_fused_frontend_and_encoder_match_unfused_and_oracle
    (rtol 3e-2, atol 5e-2);
  * CTCBeamSearcher(lp, lengths=row_lens) gives every utterance the hypotheses of its own rows decoded alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
HOP = 160
NS = [16000, 9977, 5283, 12346]
REL = [n / NS[0] for n in NS]


@pytest.fixture(scope="module")
def case():
    from mamba_asr_amd.asr import ASRConfig, ConMambaASR, synthetic_wavs
    model = ConMambaASR(ASRConfig("ragged", num_encoder_layers=2)).to(DEV).eval()
    wav, ones = synthetic_wavs(len(NS), NS[0], 7, DEV)
    with torch.no_grad():
        model.calibrate(wav, ones)
    ragged = wav.clone()
    for b, n in enumerate(NS):
        ragged[b, n:] = float("nan")
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
        enc, row_lens = model.encode(ragged, torch.tensor(REL, device=DEV), ragged=True)
        solo = [model.encode(wav[b:b + 1, :n].contiguous(), ones[:1]) for b, n in enumerate(NS)]
    return model, wav, ragged, enc, row_lens, solo


def test_row_lens_are_the_host_arithmetic(case):
    from mamba_asr_amd import fused
    model, wav, ragged, enc, row_lens, solo = case
    want = [fused.frontend_rows_total(n, HOP) for n in NS]
    assert isinstance(row_lens, fused.RowLens) and list(row_lens) == want == [s.shape[1] for s in solo]
    assert row_lens.dev.dtype == torch.int32 and row_lens.dev.is_cuda and row_lens.dev.tolist() == want
    assert enc.shape == (len(NS), max(want), 256) and enc.dtype == torch.float32
    with torch.no_grad(), torch.autocast("cuda", dtype=BF16):      # absolute sample counts give the same call
        enc2, rl2 = model.encode(ragged, torch.tensor(NS, device=DEV), ragged=True)
    assert list(rl2) == want and all(torch.equal(enc2[b, :r], enc[b, :r]) for b, r in enumerate(want))


def test_front_end_rows_equal_every_utterance_alone(case):
    from mamba_asr_amd import fused, ops
    model, wav, ragged, enc, row_lens, solo = case
    assert fused.frontend_ragged_native(model, ragged, BF16)
    ops.LAUNCH_LOG = []
    try:
        with torch.no_grad():
            rows, rl, frames = fused.frontend_ragged(model, ragged, NS, BF16)
        torch.cuda.synchronize()
        names = [e[0] for e in ops.LAUNCH_LOG]
    finally:
        ops.LAUNCH_LOG = None
    assert names == ["cm_fbank_wav_lens", "cm_fbank_finish_lens", "cm_cnn_front_lens"], names
    assert list(rl) == list(row_lens) and frames.tolist() == [1 + n // HOP for n in NS]
    c = fused._frontend_cache(model, BF16)
    b0 = model.CNN.blocks[0]
    n0 = b0.norm.norm
    for b, n in enumerate(NS):
        with torch.no_grad():
            feats = model.compute_features(wav[b:b + 1, :n].contiguous(), norm=(model.normalize.glob_mean, model.normalize.glob_std))
            alone = ops.cnn_front(feats, b0.conv.weight, b0.conv.bias, n0.weight, n0.bias, n0.eps, c["w2_ohwi"], c["b2f"], c["ln2"][0], c["ln2"][1],
                                  c["ln2"][2], 0.01)
        assert alone.shape[1] == rl[b] and bool(torch.isfinite(alone.float()).all())
        assert torch.equal(rows[b, :rl[b]], alone[0]), f"front-end rows, utterance {b}, {n} samples"


def test_encoder_output_against_every_utterance_alone(case):
    model, wav, ragged, enc, row_lens, solo = case
    for b, r in enumerate(row_lens):
        err = (enc[b, :r].float() - solo[b][0].float()).abs()
        print(f"utterance {b} ({NS[b]} samples, {r} rows): ragged against alone mean|err| {float(err.mean()):.3e}, max|err| {float(err.max()):.3e}")
        assert bool(torch.isfinite(enc[b, :r]).all()) and float(solo[b].float().std()) > 0.1
        assert float(err.mean()) < 2e-3 and float(err.max()) < 6e-2


def test_every_utterance_against_the_fp64_oracle_alone(case):
    from oracle import conmamba_oracle as O
    model, wav, ragged, enc, row_lens, solo = case
    p = {k: v.detach().double().cpu() for k, v in model.state_dict().items()}
    for b, n in enumerate(NS):
        want = O.asr_encode(p, wav[b:b + 1, :n].cpu(), torch.ones(1), 2, p["normalize.glob_mean"], p["normalize.glob_std"])
        assert want.shape[1] == row_lens[b] and want.dtype == torch.float64
        err = (enc[b, :row_lens[b]].cpu().double() - want[0]).abs()
        print(f"utterance {b}: against the fp64 oracle alone mean|err| {float(err.mean()):.3e}, max|err| {float(err.max()):.3e}")
        torch.testing.assert_close(enc[b, :row_lens[b]].cpu().double(), want[0], rtol=3e-2, atol=5e-2)


def test_ctc_beam_search_takes_row_lens(case):
    from mamba_asr_amd.ctc_decode import CTCBeamSearcher
    model, wav, ragged, enc, row_lens, solo = case
    searcher = CTCBeamSearcher(blank_index=0, vocab_list=["<b>"] + [f"t{i}" for i in range(1, 31)], beam_size=8, topk=4)
    with torch.no_grad():
        lp = torch.log_softmax(model.ctc_lin(enc.nan_to_num(0.0)), dim=-1).float()
        for b, r in enumerate(row_lens):                           # what lies behind an utterance's rows must not matter
            lp[b, r:] = 0.0
    hyps = searcher(lp, lengths=row_lens)
    assert len(hyps) == len(NS)
    for b, r in enumerate(row_lens):
        alone = searcher(lp[b:b + 1, :r].contiguous())[0]
        assert [h.text for h in hyps[b]] == [h.text for h in alone] and len(alone) >= 1, (b, hyps[b], alone)
        assert all(abs(x.score - y.score) < 1e-4 for x, y in zip(hyps[b], alone))
    with pytest.raises(ValueError, match="lengths"):
        searcher(lp, lengths=[1, 2, 3])
    # the relative lengths alone can miss an utterance's own row count: the reason for ``lengths``
    rounded = searcher.frame_counts(lp.shape[1], torch.tensor(REL), len(NS))
    print("rows per utterance:", list(row_lens), "round(rel * rows):", rounded)
