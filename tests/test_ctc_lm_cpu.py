"""CPU checks of n-gram LM fusion for the CTC beam search: the ARPA parser and the packed tables of mamba_asr_amd.ngram_lm
against the tests' dict scorer, the tests' restatement of the search (tests/ctc_lm_ref.py) against brute force, and the argument
refusals of cm_ctc_beam_lm_search."""
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctc_beam_ref as R  # noqa: E402
import ctc_lm_data as LD  # noqa: E402
import ctc_lm_ref as LR  # noqa: E402

INF = math.inf
VARIANTS = [dict(unk=True, bos=True, eos=True), dict(unk=False, bos=True, eos=True), dict(unk=True, bos=False, eos=False),
            dict(unk=False, bos=False, eos=False)]


def _lm_mod():
    from mamba_asr_amd import ngram_lm
    return ngram_lm


def test_hand_written_backoff_chains(tmp_path):
    path = LD.write_text(tmp_path / "hand.arpa", LD.HAND_ARPA)
    lm, ref = _lm_mod().NgramLM.from_arpa(path), LR.DictLM(path)
    assert lm.order == 3 and lm.words == ["<unk>", "A", "B", "C"] and (lm.bos, lm.eos, lm.unk) == (-1, -1, 0)
    for ctx, w, want in LD.HAND_CASES:
        got, nxt = lm.score(ctx, w)
        assert abs(got - want) < 1e-6, (ctx, w, got, want)
        assert abs(ref.step(ref.trunc(ctx), w, 0.0)[0] - want) < 1e-6, (ctx, w)
        assert nxt == (tuple(ctx) + (w if w != "Z" else "<unk>",))[-2:]


@pytest.mark.parametrize("gz", [False, True])
def test_parser_plain_and_gz(tmp_path, gz):
    path, words = LD.make_arpa(tmp_path / ("m.arpa.gz" if gz else "m.arpa"), seed=3, gz=gz)
    lm = _lm_mod().NgramLM.from_arpa(path)
    order, vocab, prob, bo = LR.read_arpa(path)
    assert lm.order == order == 3 and lm.words == vocab and set(words) < set(vocab)
    assert lm.n_entries == len(prob) and lm.words[lm.unk] == "<unk>" and lm.words[lm.bos] == "<s>" and lm.words[lm.eos] == "</s>"
    for cap, n in ((lm.word_cap, len(vocab)), (lm.ngram_cap, len(prob) - len(vocab))):
        assert cap & (cap - 1) == 0 and cap >= 2 * n
    assert lm.prefix_cap & (lm.prefix_cap - 1) == 0
    for w in vocab:
        assert lm.words[lm.lookup_word(w)] == w and float(lm.prob[lm.lookup_word(w)]) == prob[(w,)]
    t = lm.tables(torch.device("cpu"))
    assert t["word_keys"].shape == (lm.word_cap, 2) and t["ngram_keys"].dtype == torch.int64 and t["prob"].dtype == torch.float32


def test_parser_refuses_malformed_files(tmp_path):
    NgramLM = _lm_mod().NgramLM
    good = LD.HAND_ARPA

    def refuse(name, text, line, raw=None):
        path = str(tmp_path / name)
        if raw is None:
            LD.write_text(path, text)
        else:
            with open(path, "wb") as f:
                f.write(raw)
        with pytest.raises(ValueError) as e:
            NgramLM.from_arpa(path)
        assert path in str(e.value) and f"line {line}" in str(e.value), str(e.value)

    refuse("binary.arpa", None, 1, raw=b"mmap lm http://kheafield.com/code format version 5\n\x00\x01\xff\xfe")
    refuse("bytes.arpa", None, 2, raw=b"\\data\\\n\xff\xfe\x00garbage\n")
    refuse("nohead.arpa", good.replace("\\data\\\n", ""), 1)
    refuse("number.arpa", good.replace("-0.75\tB", "-0.7x5\tB"), 9)
    refuse("fields.arpa", good.replace("-0.6\tB C", "-0.6\tB C D E"), 14)
    refuse("count.arpa", good.replace("ngram 2=2", "ngram 2=3"), 16)
    refuse("word.arpa", good.replace("-0.6\tB C", "-0.6\tB Q"), 14)
    refuse("context.arpa", good.replace("-0.1\tA B C", "-0.1\tC B A"), 17)
    refuse("twice.arpa", good.replace("-0.6\tB C", "-0.3\tA B"), 14)
    refuse("inf.arpa", good.replace("-1.5\tC", "-inf\tC"), 10)
    refuse("end.arpa", good.replace("\\end\\\n", ""), 19)
    refuse("order.arpa", "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 7)), 7)


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_packed_tables_against_dict_scorer(tmp_path, variant):
    """NgramLM.score reads the packed tables: every (context of up to two words, word) over a sample of the vocabulary plus
    out-of-vocabulary words, in the context and as the word."""
    path, words = LD.make_arpa(tmp_path / "m.arpa", seed=10 + variant, **VARIANTS[variant])
    lm, ref = _lm_mod().NgramLM.from_arpa(path), LR.DictLM(path)
    stored = [g for g in ref.prob if len(g) == 3][:2] + [g for g in ref.prob if len(g) == 2][:2]
    sample = sorted({w for g in stored for w in g} | set(words[:2]) | set(ref.vocab_list[:3])) + ["QQQ", "ZZ"]
    n = 0
    for k in (0, 1, 2):
        for ctx in itertools.product(sample, repeat=k):
            rctx = ()
            for cw in ctx:                                  # the context as the scorer keeps it: OOV words read as <unk> / empty it
                rctx = ref.step(rctx, cw, 0.0)[1]
            for w in sample:
                want, want_next = ref.step(rctx, w, 0.0)
                got, got_next = lm.score(ctx, w)
                assert abs(got - want) <= 1e-12 and got_next == want_next, (ctx, w, got, want, got_next, want_next)
                n += 1
    assert n > 1000
    for g in ref.prob:                                      # every stored n-gram is found as itself
        assert lm.score(g[:-1], g[-1])[0] == ref.prob[g], g


@pytest.mark.parametrize("order", [1, 2, 4, 5])
def test_packed_tables_at_other_orders(tmp_path, order):
    """Orders 1, 2, 4 and 5: random contexts of up to five words, half of them the stem of a stored n-gram."""
    import random
    path, words = LD.make_arpa(tmp_path / "m.arpa", seed=40 + order, order=order, n_words=(6, 8, 4), n_bigrams=60, n_trigrams=60)
    lm, ref = _lm_mod().NgramLM.from_arpa(path), LR.DictLM(path)
    assert lm.order == ref.order == order and max(len(g) for g in ref.prob) == order
    rng, pool, grams = random.Random(order), ref.vocab_list + ["QQQ"], sorted(ref.prob)
    for i in range(1500):
        ctx = tuple(rng.choice(pool) for _ in range(rng.randrange(6)))
        if i % 2:
            g = rng.choice(grams)
            ctx, w = ctx[:rng.randrange(3)] + g[:-1], (g[-1] if rng.random() < 0.7 else rng.choice(pool))
        else:
            w = rng.choice(pool)
        rctx = ()
        for cw in ctx:
            rctx = ref.step(rctx, cw, 0.0)[1]
        want, want_next = ref.step(rctx, w, 0.0)
        got, got_next = lm.score(ctx, w)
        assert abs(got - want) <= 1e-12 and got_next == want_next, (ctx, w, got, want, got_next, want_next)
    for g in ref.prob:
        assert lm.score(g[:-1], g[-1])[0] == ref.prob[g], g


def test_prefix_set_against_brute_force(tmp_path):
    path, words = LD.make_arpa(tmp_path / "m.arpa", seed=5)
    lm = _lm_mod().NgramLM.from_arpa(path)
    given = _lm_mod().NgramLM.from_arpa(path, unigrams=["HELLO", "HE'S", "A"])
    for k in (1, 2, 3, 4):
        for p in ("".join(t) for t in itertools.islice(itertools.product(LD.LETTERS, repeat=k), 0, 3000, 1 if k < 3 else 7)):
            assert lm.is_prefix(p) == any(w.startswith(p) for w in words), p
    for p in ("<", "<s>", "<unk", "</s>"):
        assert not lm.is_prefix(p)                          # the specials are not unigram-list words
    for p in ("H", "HELLO", "HE'", "HELLOS", "A", "AB", "E", words[0]):
        assert given.is_prefix(p) == any(u.startswith(p) for u in ("HELLO", "HE'S", "A")), p


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("score_boundary", [True, False])
def test_restatement_matches_brute_force_plus_lm(tmp_path, variant, score_boundary):
    """Pruning off, every beam kept: each text's acoustic score is the brute-force CTC likelihood and its total that plus
    LM(text) computed from the text alone."""
    vocab = ["<b>", "▁", "A", "▁B"]
    path, _ = LD.make_arpa(tmp_path / "m.arpa", seed=20 + variant, letters=["A", "B"], n_bigrams=12, n_trigrams=10, **VARIANTS[variant])
    lm = LR.DictLM(path)
    lp = torch.log_softmax(torch.randn(5, 4, generator=torch.Generator().manual_seed(variant), dtype=torch.float64) * 1.5, -1).tolist()
    kw = dict(alpha=0.7, beta=1.1, unk_score_offset=-3.0, score_boundary=score_boundary)
    got, _ = LR.beam_search_lm(lp, 5, vocab, lm, beam_size=10 ** 9, beam_prune_logp=-INF, token_prune_min_logp=-INF, topk=10 ** 9, **kw)
    want = R.brute_force(lp, vocab)
    assert {t for t, _, _ in got} == set(want) and len(got) == len(want)
    for text, ac, total in got:
        assert abs(ac - want[text]) <= 1e-12
        assert abs(total - LR.final_total(lm, text, want[text], **kw)) <= 1e-12, text
    assert [t for _, _, t in got] == sorted((t for _, _, t in got), reverse=True)
    assert any(w not in lm.vocab for t, _, _ in got for w in t.split()) and any(" " in t for t, _, _ in got)
    # the package's host LM(text) agrees with the dict scorer's
    plm = _lm_mod().NgramLM.from_arpa(path)
    for text, ac, total in got:
        assert abs(ac + plm.lm_of_text(text, kw["alpha"], kw["beta"], kw["unk_score_offset"], score_boundary, finish=True) - total) <= 1e-12


def _lm_args(N):
    a = N.CtcBeamLmArgs()
    a.batch, a.T, a.V, a.beam_size, a.topk, a.lp_ts = 2, 10, 31, 100, 1, 31
    import ctypes as C
    for f, t in a._fields_:
        if t is C.c_void_p and f != "stream":
            setattr(a, f, 64)                               # any non-NULL value: validation runs on the host and launches nothing
    a.stream = None
    a.hash_base[0], a.hash_base[1], a.hash_sep = 3, 5, 7
    a.blank_skip_threshold = 1.0
    a.order, a.n_words, a.n_entries, a.word_cap, a.prefix_cap, a.ngram_cap = 3, 10, 30, 32, 64, 64
    a.lm_bos, a.lm_eos, a.lm_unk = 1, 2, 0
    a.alpha, a.beta, a.unk_score_offset = 0.5, 1.5, -10.0
    return a


def test_abi_refuses_bad_lm_arguments_without_gpu():
    import ctypes as C
    import mamba_asr_amd._native as N
    lib = N.lib()
    assert N.ABI_VERSION == 12
    assert lib.cm_ctc_beam_lm_search(None) == -1
    assert lib.cm_ctc_beam_lm_search(C.byref(N.CtcBeamLmArgs())) == -1 and b"bad sizes" in lib.cm_last_error()
    ws = lib.cm_ctc_beam_lm_workspace_bytes(C.byref(_lm_args(N)))
    assert ws == 2 * (10 * 100 * 4 + 4 * 8 * 4096)           # the LM-free search's slab: history, then the global sort arrays

    def refused(msg, **fields):
        a = _lm_args(N)
        a.workspace_bytes = ws
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.cm_ctc_beam_lm_search(C.byref(a)) == -1, fields
        assert msg in lib.cm_last_error(), (fields, lib.cm_last_error())

    refused(b"NULL", tok_len=None)
    refused(b"NULL", lm_scores=None)
    refused(b"NULL LM table", ngram_keys=None)
    refused(b"NULL LM table", lm_backoff=None)
    refused(b"order", order=0)
    refused(b"order", order=6)
    refused(b"powers of two", word_cap=33)
    refused(b"powers of two", prefix_cap=0)
    refused(b"powers of two", ngram_cap=-64)
    refused(b"n_entries", n_entries=5)
    refused(b"n_entries", n_entries=1 << 31)
    refused(b"word id", lm_bos=10)
    refused(b"word id", lm_unk=-2)
    refused(b"finite", alpha=float("nan"))
    refused(b"finite", beta=float("nan"))
    refused(b"finite", unk_score_offset=float("nan"))
    refused(b"NaN", beam_prune_logp=float("nan"))
    refused(b"workspace", workspace_bytes=ws - 1)


def test_searcher_with_a_path_parses_it_and_stream_refuses(tmp_path):
    from mamba_asr_amd import ctc_decode as M
    import ctc_beam_data as D
    path, words = LD.make_arpa(tmp_path / "m.arpa", seed=1)
    s = M.CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path, alpha=0.4)
    assert s.lm.order == 3 and s.alpha == 0.4 and s.beta == 1.5 and s.unk_score_offset == -10.0 and s.score_boundary
    assert s.tok_len.tolist() == [len(c) for c in s.clean] and s.tok_len[1] == 3
    u = M.CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path, unigrams=["ZEBRA"])
    assert u.lm.is_prefix("ZEB") and not u.lm.is_prefix(words[0])
    # T = 0: the one empty hypothesis, lm_score = LM("") = the </s> term alone
    ref = LR.DictLM(path)
    with pytest.raises(RuntimeError, match="GPU"):
        s(torch.zeros(1, 3, 31))
    with pytest.raises(ValueError, match="finite"):
        M.CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path, beta=float("nan"))
    with pytest.raises(ValueError, match="line 1"):
        M.CTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=LD.write_text(tmp_path / "bad.arpa", "hello\n"))
    assert abs(s.lm.lm_of_text("", 0.4, 1.5, -10.0, True, finish=True) - LR.final_total(ref, "", 0.0, 0.4, 1.5, -10.0, True)) <= 1e-12
    with pytest.raises(NotImplementedError, match="streamed"):
        M.StreamingCTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, kenlm_model_path=path)
    assert M.StreamingCTCBeamSearcher(**D.RECIPE, vocab_list=D.SPM_VOCAB, alpha=0.1).lm is None      # without a path: as before
