"""mamba_asr_amd.metrics on its host path, the recipe YAML's wer_computer / cer_computer, and CTCGreedyDecoder on CPU tensors,
against tests/ctc_score_ref.py.  Every comparison is exact.  No parity with speechbrain's I / D / S split is claimed:
the tie rule of the contract is what the hand-worked cases restate."""
import io
import os
import random
import re

import pytest
import torch

import ctc_score_ref as SR
from recipe_brain import load_recipe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = os.path.join(ROOT, "tests", "golden", "conmamba_large_ctc.yaml")


def _pairs(n, alphabet, seed, lo=0, hi=12):
    rng = random.Random(seed)
    return [([rng.randrange(alphabet) for _ in range(rng.randint(lo, hi))], [rng.randrange(alphabet) for _ in range(rng.randint(lo, hi))])
            for _ in range(n)]


# ------------------------------------------------------------------------------------------------------------------ edit distance
@pytest.mark.parametrize("ref, hyp, counts, path", [
    ("a b c", "a c", [0, 1, 0, 2], "=D="),                   # one deletion
    # a b vs b a: D[1][1] = 1 by substitution (1 < 2, 1 < 2); D[1][2]: sub = 1 + 0 = 1, del = 3, ins = 2 -> diagonal (hit);
    # D[2][1]: sub = 1 + 0 = 1 -> diagonal; D[2][2]: sub = D[1][1] + 1 = 2, del = D[1][2] + 1 = 2, ins = D[2][1] + 1 = 2: the
    # substitution does not win strictly, del < ins is false -> insert; from (2, 1) diagonal (b = b) to (1, 0), then a deletion
    ("a b", "b a", [1, 1, 0, 1], "D=I"),
    ("", "x y z", [3, 0, 0, 0], "III"),
    ("x y z", "", [0, 3, 0, 0], "DDD"),
    ("", "", [0, 0, 0, 0], ""),
    ("p q r s", "p q r s", [0, 0, 0, 4], "===="),
    ("a", "b", [0, 0, 1, 0], "S"),                           # 1 < 2 and 1 < 2: a lone substitution wins strictly
    ("a a", "a", [0, 1, 0, 1], "=D"),                        # D[2][1]: sub = 1, del = 1, ins = 3: del < ins -> delete at the end
])
def test_hand_worked_cases(ref, hyp, counts, path):
    from mamba_asr_amd import metrics
    a, b = ref.split(), hyp.split()
    assert SR.edit_ops(a, b) == (counts, sum(counts[:3]), path)
    assert metrics.edit_ops_host(a, b) == (counts, sum(counts[:3]), path)


@pytest.mark.parametrize("alphabet", [2, 30])
def test_host_path_equals_the_reference_and_keeps_the_invariants(alphabet):
    from mamba_asr_amd import metrics
    pairs = _pairs(200, alphabet, seed=alphabet)
    scored = metrics.score_pairs([a for a, _ in pairs], [b for _, b in pairs])
    for (a, b), (counts, path) in zip(pairs, scored):
        want = SR.edit_ops(a, b)
        assert (counts, path) == (want[0], want[2]) and metrics.edit_ops_host(a, b) == want
        SR.check_invariants(a, b, counts, want[1], path)
    if alphabet == 2:
        assert sum(1 for (a, b), (c, _) in zip(pairs, scored) if c[0] and c[1]) > 10       # ties decided both ways occur


def test_error_rate_stats_words_summary_and_empty_set():
    from mamba_asr_amd.metrics import ErrorRateStats
    s = ErrorRateStats()
    assert s.summarize("WER") == 0.0 and s.summarize()["num_scored_sents"] == 0 and s.summarize("SER") == 0.0
    assert all(v == 0 for v in s.summarize().values())
    refs = [["the", "cat", "sat"], ["hello"], ["a", "b", "c", "d"], []]
    hyps = [["the", "cat", "sat"], ["hallo", "there"], ["a", "c", "d"], []]
    s.append(["u1", "u2", "u3", "u4"], hyps, refs)
    m = s.summarize()
    assert set(m) == {"WER", "error_rate", "SER", "insertions", "deletions", "substitutions", "num_edits", "num_scored_tokens",
                      "num_ref_tokens", "num_hyp_tokens", "num_scored_sents", "num_erroneous_sents"}
    wer, (ins, dele, sub), n = SR.error_rates(refs, hyps)
    assert (m["WER"], m["insertions"], m["deletions"], m["substitutions"], m["num_ref_tokens"]) == (wer, ins, dele, sub, n)
    assert m["error_rate"] == m["WER"] == 100.0 * 3 / 8 and (ins, dele, sub) == (1, 1, 1) and m["num_edits"] == 3
    assert m["num_scored_tokens"] == 8 and m["num_hyp_tokens"] == 8 and m["num_scored_sents"] == 4 and m["num_erroneous_sents"] == 2
    assert m["SER"] == 50.0 and s.summarize("error_rate") == m["WER"]
    s.append(["u5"], [["x"]], [["y"]])                                      # a second append accumulates
    assert s.summarize("num_edits") == 4 and s.summarize("num_scored_sents") == 5
    only_ins = ErrorRateStats()
    only_ins.append(["e"], [["x"]], [[]])
    assert only_ins.summarize("WER") == 100.0 and only_ins.summarize("insertions") == 1


def test_split_and_merge_tokens():
    from mamba_asr_amd.metrics import ErrorRateStats
    refs, hyps = [["hello", "world"]], [["hallo", "word"]]
    cer = ErrorRateStats(split_tokens=True)
    cer.append(["u"], hyps, refs)
    a, b = list("hello_world"), list("hallo_word")
    want = SR.edit_ops(a, b)
    m = cer.summarize()
    assert (m["insertions"], m["deletions"], m["substitutions"]) == tuple(want[0][:3]) == (0, 1, 1)
    assert m["num_ref_tokens"] == 11 and m["WER"] == 100.0 * 2 / 11
    chars = [list("the_cat_sat")], [list("the_cats_at")]
    merged = ErrorRateStats(merge_tokens=True)
    merged.append(["u"], chars[1], chars[0])
    assert merged.scores[0]["ref_tokens"] == ["the", "cat", "sat"] and merged.scores[0]["hyp_tokens"] == ["the", "cats", "at"]
    assert merged.summarize("substitutions") == 2 and merged.summarize("WER") == 100.0 * 2 / 3
    both = ErrorRateStats(merge_tokens=True, split_tokens=True, space_token=" ")
    both.append(["u"], [list("ab  c")], [list("ab c")])                      # merged to words (empty ones dropped), then characters
    assert both.summarize("num_edits") == 0 and both.scores[0]["ref_tokens"] == list("ab c")


def test_tensors_relative_lengths_and_ind2lab():
    from mamba_asr_amd.metrics import ErrorRateStats
    lab = {0: "<pad>", 1: "a", 2: "b", 3: "c"}
    predict = torch.tensor([[1, 2, 3, 0], [2, 2, 0, 0]])
    target = torch.tensor([[1, 3, 0, 0, 0], [2, 2, 1, 3, 0]])
    s = ErrorRateStats()
    s.append(["x", "y"], predict, target, predict_len=torch.tensor([0.75, 0.5]), target_len=torch.tensor([0.4, 0.8]), ind2lab=lab)
    assert s.scores[0]["hyp_tokens"] == ["a", "b", "c"] and s.scores[0]["ref_tokens"] == ["a", "c"]
    assert s.scores[1]["hyp_tokens"] == ["b", "b"] and s.scores[1]["ref_tokens"] == ["b", "b", "a", "c"]
    assert (s.summarize("insertions"), s.summarize("deletions"), s.summarize("substitutions")) == (1, 2, 0)
    fn = ErrorRateStats()
    fn.append(["x", "y"], predict, target, torch.tensor([0.75, 0.5]), torch.tensor([0.4, 0.8]), ind2lab=lambda rows: [[lab[t] for t in r] for r in rows])
    assert fn.summarize() == s.summarize()
    with pytest.raises(ValueError, match="2 ids"):
        s.append(["x", "y"], [["a"]], [["a"]])


def test_oracle_picks_the_first_minimum():
    from mamba_asr_amd.metrics import ErrorRateStats
    target = [["a", "b", "c"], ["d"]]
    nbest = [[["a", "x", "c", "y"], ["a", "b"], ["b", "c"], ["a", "b", "c", "d", "e"]], [["e"], ["d"], ["d"]]]
    s = ErrorRateStats()
    recs = s.oracle(["u1", "u2"], nbest, target)
    assert [r["best_index"] for r in recs] == [1, 1] and [r["num_edits"] for r in recs] == [1, 0]       # 2, 1, 1, 2 and 1, 0, 0
    assert recs[0]["hyp_tokens"] == ["a", "b"] and recs[0]["key"] == "u1" and s.scores == []
    for u, hyps in enumerate(nbest):
        edits = [SR.edit_ops(target[u], h)[1] for h in hyps]
        assert recs[u]["best_index"] == edits.index(min(edits))
    top = ErrorRateStats()
    top.extend(recs)
    assert top.summarize("WER") == 25.0 and top.summarize("num_scored_sents") == 2
    with pytest.raises(ValueError, match="no hypotheses"):
        s.oracle(["u"], [[]], [["a"]])


def test_write_stats_round_trips_its_summary():
    from mamba_asr_amd.metrics import ErrorRateStats
    pairs = _pairs(12, 5, seed=7, lo=0, hi=7)
    s = ErrorRateStats()
    s.append([f"utt{k}" for k in range(12)], [[f"w{t}" for t in b] for _, b in pairs], [[f"w{t}" for t in a] for a, _ in pairs])
    buf = io.StringIO()
    s.write_stats(buf)
    lines = buf.getvalue().split("\n")
    m = s.summarize()
    g = re.fullmatch(r"%WER (\d+\.\d\d) \[ (\d+) / (\d+), (\d+) ins, (\d+) del, (\d+) sub \]", lines[0])
    assert g and [int(x) for x in g.groups()[1:]] == [m["num_edits"], m["num_scored_tokens"], m["insertions"], m["deletions"], m["substitutions"]]
    assert g.group(1) == f"{m['WER']:.2f}" and abs(float(g.group(1)) - 100.0 * int(g.group(2)) / int(g.group(3))) <= 0.005
    g = re.fullmatch(r"%SER (\d+\.\d\d) \[ (\d+) / (\d+) \]", lines[1])
    assert g and [int(x) for x in g.groups()[1:]] == [m["num_erroneous_sents"], 12] and lines[2] == ""
    blocks = buf.getvalue().split("\n\n")[1:-1]
    assert len(blocks) == 12
    edits = 0
    for k, (block, (a, b)) in enumerate(zip(blocks, pairs)):
        head, ref, op, hyp = block.split("\n")
        assert head.startswith(f"utt{k}, %WER ") and ref.startswith("ref: ") and op.startswith("op : ") and hyp.startswith("hyp: ")
        cols = [[c.strip() for c in row[5:].split(" ; ")] if row[5:] else [] for row in (ref, op, hyp)]
        assert len(cols[0]) == len(cols[1]) == len(cols[2])
        assert [c for c in cols[0] if c != "<eps>"] == [f"w{t}" for t in a] and [c for c in cols[2] if c != "<eps>"] == [f"w{t}" for t in b]
        assert "".join(cols[1]) == SR.edit_ops(a, b)[2]
        edits += sum(1 for c in cols[1] if c != "=")
    assert edits == m["num_edits"]


def test_accuracy_stats_padding_and_relative_lengths():
    from mamba_asr_amd.metrics import AccuracyStats
    g = torch.Generator().manual_seed(5)
    lp = torch.log_softmax(torch.randn(3, 8, 6, generator=g), dim=-1)
    best = lp.argmax(-1)
    targets = best.clone()
    targets[0, 2] = (targets[0, 2] + 1) % 6                                  # one miss inside utterance 0
    targets[1, 6] = (targets[1, 6] + 1) % 6                                  # a miss in the padding of utterance 1: not counted
    targets[2, 0] = (targets[2, 0] + 1) % 6
    length = torch.tensor([1.0, 0.75, 0.5])                                  # 8, 6, 4 positions
    acc = AccuracyStats()
    assert acc.summarize() == 0.0
    acc.append(lp, targets, length)
    assert (acc.correct, acc.total) == (16, 18) and acc.summarize() == 16 / 18
    acc.append(lp[:1], targets[:1])                                          # no lengths: every position
    assert (acc.correct, acc.total) == (23, 26)


def test_the_recipe_yaml_resolves_to_scorers():
    from mamba_asr_amd import metrics
    from mamba_asr_amd.hparams import Opaque
    hp = load_recipe(LARGE, num_encoder_layers=1)
    wer, cer = hp["wer_computer"](), hp["cer_computer"]()
    assert isinstance(wer, metrics.ErrorRateStats) and isinstance(cer, metrics.ErrorRateStats)
    assert not wer.split_tokens and cer.split_tokens and wer is not hp["wer_computer"]()
    assert isinstance(hp["checkpointer"], Opaque)                           # the other speechbrain paths stay inert
    refs, hyps = [["a", "bc"], ["de"]], [["a", "bd"], ["de", "f"]]
    for m in (wer, cer):
        m.append(["u1", "u2"], hyps, refs)
    assert wer.summarize("error_rate") == SR.error_rates(refs, hyps)[0] == 100.0 * 2 / 3
    chars = lambda rows: [list("_".join(r)) for r in rows]
    assert cer.summarize("error_rate") == SR.error_rates(chars(refs), chars(hyps))[0] == 100.0 * 3 / 6      # a_bc / a_bd: one substitution; de / de_f: two insertions


# ------------------------------------------------------------------------------------------------------------------ greedy decode
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_greedy_decoder_equals_dataio_and_the_reference(dtype):
    from mamba_asr_amd import dataio
    from mamba_asr_amd.ctc_decode import CTCGreedyDecoder
    g = torch.Generator().manual_seed(21)
    B, T, V, blank = 5, 37, 11, 3
    lp = torch.log_softmax(torch.randn(B, T, V, generator=g) * 3.0, dim=-1).to(dtype)
    wav_lens = torch.tensor([1.0, 0.5, 0.33, 0.0, 0.97])
    dec = CTCGreedyDecoder(blank)
    got = dec.tokens(lp, wav_lens)
    assert got == dataio.ctc_greedy_decode(lp.float(), wav_lens, blank) and any(got) and got[3] == []
    counts = [int(round(r * T)) for r in wav_lens.tolist()]
    want = SR.greedy_batch(lp.double().numpy(), counts, blank)
    hyps = dec(lp, wav_lens)
    for b, h in enumerate(hyps):
        k = int(want[1][b])
        assert h.tokens == want[0][b, :k].tolist() and h.text == "" and h.text_frames is None
        assert h.score == float(sum(want[4][b, :k].tolist()))
    assert dec.tokens(lp, lengths=counts) == got
    bad = lp.clone()
    bad[1, 30] = float("nan")                                               # past utterance 1's 18 frames: never read
    assert dec.tokens(bad, wav_lens) == got
    bad[4, 2, 5] = float("nan")
    with pytest.raises(ValueError, match="utterance 4"):
        dec.tokens(bad, wav_lens)


def test_cpu_greedy_decoder_text_and_word_frames():
    from mamba_asr_amd.ctc_decode import CTCGreedyDecoder
    vocab = ["<blank>", " ", "a", "b", "c"]
    path = [0, 2, 2, 0, 2, 3, 1, 1, 4, 0, 0, 3]                              # a | a b | space | c | b  ->  "aab cb"
    lp = torch.full((1, len(path), 5), -4.0)
    for t, v in enumerate(path):
        lp[0, t, v] = -0.25
    h = CTCGreedyDecoder(0, vocab)(lp)[0]
    assert h.tokens == [2, 2, 3, 1, 4, 3] and h.text == "aab cb" and h.text_frames == [(1, 6), (8, 12)]
    assert h.score == -0.25 * 8 and h.lm_score == h.score                   # eight non-blank frames
    ties = torch.zeros(1, 4, 5)                                              # every frame a five-way tie: index 0, the blank
    assert CTCGreedyDecoder(0, vocab).tokens(ties) == [[]] and CTCGreedyDecoder(1, vocab).tokens(ties) == [[0]]
    ninf = torch.full((1, 3, 5), float("-inf"))
    assert CTCGreedyDecoder(2, vocab).tokens(ninf) == [[0]]
