"""Seeded small ARPA files for the LM-fused CTC beam search tests: order-3 models (other orders on request) over words of 1 to
3 letters, with some words absent, some bigrams and trigrams present and some backoffs omitted; with or without <unk>, <s>, </s>.  Plus one hand-written
ten-line file whose backoff chains the tests check against literal numbers."""
import gzip
import itertools
import random

LETTERS = [chr(ord("A") + i) for i in range(26)] + ["'"]           # the characters of ctc_beam_data.SPM_VOCAB

HAND_ARPA = """\\data\\
ngram 1=4
ngram 2=2
ngram 3=1

\\1-grams:
-1.0\t<unk>
-0.5\tA\t-0.25
-0.75\tB\t-0.125
-1.5\tC

\\2-grams:
-0.3\tA B\t-0.0625
-0.6\tB C

\\3-grams:
-0.1\tA B C

\\end\\
"""
# log10 p(word | context) of HAND_ARPA (to compare within fp32 rounding of the file's numbers):
#   C after A B: the trigram;  C after C B: bigram B C (context C B is not stored: no backoff);  A after A B: backoff(A B) +
#   backoff(B) + p(A);  B after B: backoff(B) + p(B);  C after A: backoff(A) + p(C);  Z after A B: <unk> through both backoffs
HAND_CASES = [(("A", "B"), "C", -0.1), (("C", "B"), "C", -0.6), (("A", "B"), "A", -0.0625 - 0.125 - 0.5),
              (("B",), "B", -0.125 - 0.75), (("A",), "C", -0.25 - 1.5), ((), "B", -0.75), (("A", "B"), "Z", -0.0625 - 0.125 - 1.0)]


def write_text(path, text, gz=False):
    path = str(path)
    if gz:
        with gzip.open(path, "wt", encoding="utf-8") as f:
            f.write(text)
    else:
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
    return path


def arpa_text(seed, letters=LETTERS, unk=True, bos=True, eos=True, n_words=(20, 40, 30), n_bigrams=120, n_trigrams=80, order=3,
              n_more=(60, 40)):
    """-> (ARPA text, the ordinary words).  n_words: how many words of 1, 2 and 3 letters (capped by how many exist); ``order``
    1 to 5, n_more the 4-gram and 5-gram counts.  Every n-gram extends a listed (n-1)-gram, as the packed tables need."""
    rng = random.Random(seed)
    words = []
    for k, want in zip((1, 2, 3), n_words):
        pool = ["".join(t) for t in itertools.product(letters, repeat=k)]
        words += rng.sample(pool, min(want, max(1, len(pool) * 2 // 3)))          # some words of every length stay absent
    rng.shuffle(words)
    vocab = (["<unk>"] if unk else []) + (["<s>"] if bos else []) + (["</s>"] if eos else []) + words
    firsts = [w for w in vocab if w != "</s>"]
    lasts = [w for w in vocab if w != "<s>"]
    levels = [[(w,) for w in vocab]]
    for n, want in zip(range(2, order + 1), (n_bigrams, n_trigrams) + tuple(n_more)):
        grams = set()
        if n == 2:
            while len(grams) < min(want, len(firsts) * len(lasts) // 2):
                grams.add((rng.choice(firsts), rng.choice(lasts)))
        else:
            stems = [g for g in levels[-1] if g[-1] != "</s>"]
            while stems and len(grams) < min(want, len(stems) * len(lasts) // 2):
                grams.add(rng.choice(stems) + (rng.choice(lasts),))
        grams = sorted(grams)
        rng.shuffle(grams)
        levels.append(grams)

    def line(gram, backoff):
        s = f"{-rng.uniform(0.1, 4.0):.4f}\t{' '.join(gram)}"
        return s + f"\t{-rng.uniform(0.0, 1.5):.4f}" if backoff and rng.random() < 0.7 else s          # some backoffs omitted

    out = ["\\data\\"] + [f"ngram {n}={len(g)}" for n, g in enumerate(levels, 1)]
    for n, grams in enumerate(levels, 1):
        out += ["", f"\\{n}-grams:"] + [line(g, n < order and g[-1] != "</s>") for g in grams]
    out += ["", "\\end\\", ""]
    return "\n".join(out), words


def make_arpa(path, seed, gz=False, **kw):
    """Write the seeded model to ``path`` -> (path, the ordinary words)."""
    text, words = arpa_text(seed, **kw)
    return write_text(path, text, gz), words


LARGEST = dict(n_words=(27, 600, 3000), n_bigrams=20000, n_trigrams=20000)       # the generator's largest file (pack-time figure)
