"""The chrF reference of the tests (tests/chrf_ref.py, Counter on strings) against a brute-force positional restatement of the rule
that shares nothing with it -- its own scan for words, its own punctuation list, matches counted position by position -- over every
text of up to five characters over {a, b, ' ', '.'} on both sides; the anchors and punctuation cases of DESIGN.md 5j by hand; and
five wrong twins of the rule, each of which must differ from the reference on these texts."""
import itertools

import pytest

import chrf_ref as R

ALPHABET = "ab ."
ASCII_PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


# ---------------------------------------------------------------------------------------------- the restatement
def brute_streams(text):
    """(characters without breaks, words after the punctuation split), by a scan of its own"""
    chars, words, cur = [], [], []
    for c in text + " ":
        if c == " ":
            if cur:
                if len(cur) > 1 and cur[-1] in ASCII_PUNCT:
                    words += ["".join(cur[:-1]), cur[-1]]
                elif len(cur) > 1 and cur[0] in ASCII_PUNCT:
                    words += [cur[0], "".join(cur[1:])]
                else:
                    words.append("".join(cur))
            cur = []
        else:
            chars.append(c)
            cur.append(c)
    return tuple(chars), tuple(words)


def positions(seq, n):
    """per position that has an n-gram: (the n-gram, how many earlier positions hold the same one)"""
    out = []
    for i in range(len(seq) - n + 1):
        g = seq[i:i + n]
        out.append((g, sum(1 for k in range(i) if seq[k:k + n] == g)))
    return out


def occurrences(seq, n):
    table = {}
    for i in range(len(seq) - n + 1):
        table[seq[i:i + n]] = table.get(seq[i:i + n], 0) + 1
    return table


class Side:
    def __init__(self, streams):
        chars, words = streams
        self.pos = [positions(chars, n) for n in range(1, 7)] + [positions(words, n) for n in range(1, 3)]
        self.occ = [occurrences(chars, n) for n in range(1, 7)] + [occurrences(words, n) for n in range(1, 3)]


def brute_stats(h, r):
    out = []
    for k in range(8):
        out += [len(h.pos[k]), len(r.pos[k]), sum(1 for g, rank in h.pos[k] if rank < r.occ[k].get(g, 0))]
    return out


TEXTS = ["".join(t) for n in range(6) for t in itertools.product(ALPHABET, repeat=n)]


def test_the_reference_equals_the_positional_restatement_on_every_small_text():
    assert len(TEXTS) == 1365
    classes = {}
    for t in TEXTS:                                             # the statistics are a function of the two streams of a side ...
        streams = brute_streams(t)
        assert "".join(streams[0]) == "".join(t.split()) and list(streams[1]) == R.words_of(t), t   # as pair_stats derives them
        classes.setdefault(streams, t)                          # texts with the same streams ("a." and "a .") are one class
    sides = [(Side(s), norm) for s, norm in classes.items()]
    checked = 0
    for h, ht in sides:                                         # ... so every pair of texts is a pair of classes, raw breaks included
        for r, rt in sides:
            assert brute_stats(h, r) == R.pair_stats(ht, rt, 6, 2), (ht, rt)
            checked += 1
    assert checked == len(classes) ** 2 and checked > 100000


def test_orders_above_the_configured_ones_are_zeros():
    full = R.pair_stats("ab ab.", "ab. ab", 6, 2)
    for co in range(1, 7):
        for wo in range(3):
            got = R.pair_stats("ab ab.", "ab. ab", co, wo)
            assert got[:3 * co] == full[:3 * co] and got[3 * co:18] == [0] * (18 - 3 * co)
            assert got[18:18 + 3 * wo] == full[18:18 + 3 * wo] and got[18 + 3 * wo:] == [0] * (6 - 3 * wo)


def test_the_four_anchors():
    for co, wo in ((6, 0), (6, 2), (1, 0), (3, 1)):
        assert R.score(R.pair_stats("ab c. d", "ab c. d", co, wo), co, wo) == 100.0
        assert R.score(R.pair_stats("abc ab", "xyz x", co, wo), co, wo) == 0.0
        assert R.score(R.pair_stats("", "", co, wo), co, wo) == 0.0 and R.score(R.pair_stats(" ", "  ", co, wo), co, wo) == 0.0
    s = R.pair_stats("abc", "abd", 6, 0)
    assert s[:9] == [3, 3, 2, 2, 2, 1, 1, 1, 0] and s[9:] == [0] * 15
    assert R.score(s, 6, 0) == pytest.approx(100 * (2 / 3 + 1 / 2 + 0) / 3, rel=1e-15) == pytest.approx(38.88888888888889, rel=1e-13)
    assert R.score(R.pair_stats("abc", "", 6, 0), 6, 0) == 0.0, "no order has n-grams on both sides"
    # beta weighs recall: a hypothesis that is a part of the reference has P = 1 and R < 1
    part = R.pair_stats("ab", "abab", 1, 0)
    assert part[:3] == [2, 4, 2] and R.score(part, 1, 0, beta=2.0) == pytest.approx(100 * 5 * 1 * 0.5 / (4 * 1 + 0.5), rel=1e-15)
    assert R.corpus_score([R.pair_stats("ab", "abab", 1, 0), R.pair_stats("abab", "ab", 1, 0)], 1, 0) == pytest.approx(100 * 4 / 6, rel=1e-15)


def test_the_punctuation_cases():
    want = {"a.": ["a", "."], ".a": [".", "a"], ".": ["."], "a.b": ["a.b"], "..": [".", "."], "(a)": ["(a", ")"],
            "a": ["a"], "ab,": ["ab", ","], "'ab": ["'", "ab"], "a-b c": ["a-b", "c"], "¿a?": ["¿a", "?"], "a…": ["a…"]}
    for text, words in want.items():
        assert R.words_of(text) == words and list(brute_streams(text)[1]) == words, text
    assert sorted(R.PUNCT) == sorted(ASCII_PUNCT) and len(R.PUNCT) == 32
    assert R.words_of("  a.  .a ") == ["a", ".", ".", "a"]
    assert R.pair_stats("(a)", "(a )", 6, 2)[18:] == [2, 3, 1, 1, 2, 0]


def test_every_wrong_twin_differs_from_the_reference():
    texts = [t for t in TEXTS if len(t) <= 3 and t == " ".join(t.split())] + ["a. .a", " a", "ab  ab", ".a a.", "abab", "a.b."]
    differs = dict.fromkeys(R.TWINS, 0)
    pairs = 0
    for h in texts:
        for r in texts:
            pairs += 1
            base = R.pair_stats(h, r, 6, 2)
            for twin in ("keep_space", "no_clip", "first_rule_first"):
                differs[twin] += R.pair_stats(h, r, 6, 2, twin=twin) != base
            for twin in ("all_orders", "beta_other_side"):
                differs[twin] += abs(R.score(base, 6, 2, twin=twin) - R.score(base, 6, 2)) > 1e-9
    print("pairs %d, differing per twin: %s" % (pairs, differs))
    assert sorted(differs) == sorted(R.TWINS) and len(R.TWINS) >= 5
    assert all(n > 0 for n in differs.values()), differs


def test_characters_of_one_code_point_a_token_count_as_bleu_tokens():
    """the identity tests/test_ngram_match_gpu.py holds the two kernels to, on its own pairs and on the two references alone: with one
    character a token and nothing trimmed, chrF's character statistics of the orders 1 to 4 are BLEU's; and BLEU's two forms agree"""
    import bleu_ref
    import ngram_cases as G
    n = 0
    for call in range(len(G.HYP_LENS)):
        hyps, refs, bleu, chrf = G.case(call)
        for h, r, b in zip(hyps, refs, bleu):
            assert list(b) == bleu_ref.stats_positional(h, r, G.PAD, G.EOS, -1)
        assert (chrf[:, 0] == bleu[:, 1]).all() and (chrf[:, 1] == bleu[:, 0]).all()
        for k in range(4):
            assert (chrf[:, 3 * k + 2] == bleu[:, 2 + 2 * k]).all() and (chrf[:, 3 * k] == bleu[:, 3 + 2 * k]).all()
        n += len(hyps)
    assert n == 210
