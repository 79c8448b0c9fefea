"""The Python reference of WER / CER (tests/text_error_ref.py) against an independently written two-row Levenshtein distance and hand
cases, and how often each wrong twin differs from it on the random cases of the GPU test: a twin that never differed there would
show that those cases cannot tell it from the rule."""
import itertools

import pytest

import text_error_ref as R

D = R.make_dictionary()
T = lambda *s: [D.indices[x] for x in s]


def levenshtein(a, b):
    """two rows, nothing stored but the distance"""
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def test_error_counts_equal_an_independent_levenshtein():
    seqs = [list(s) for n in range(5) for s in itertools.product("ab", repeat=n)]
    assert len(seqs) == 31
    for h in seqs:
        for r in seqs:
            p = R.pair_of_texts(" ".join(h), " ".join(r), "word")
            assert p["errors"] == levenshtein(h, r), (h, r)
            assert p["matches"] + p["substitutions"] + p["deletions"] == len(r) and p["matches"] + p["substitutions"] + p["insertions"] == len(h)
            c = R.pair_of_texts("".join(h), "".join(r), "char")
            assert c["errors"] == p["errors"], "one-letter words: the characters without spaces are the words"


def test_hand_cases():
    p = R.pair_of_texts("a b c", "a x c d", "word")
    assert (p["substitutions"], p["deletions"], p["insertions"], p["ref_units_n"], p["rate"]) == (1, 1, 0, 4, 50.0)
    assert p["hyp_units"] == [0, 1, 2] and p["ref_units"] == [0, 4, 2, 6], "first-occurrence ids over hypothesis, then reference"
    same = R.pair_of_texts("ab cd", "ab cd", "word")
    assert same["errors"] == 0 and same["rate"] == 0.0 and same["accuracy"] == 100.0 and same["ops"] == [0, 0]
    none = R.pair_of_texts("", "a b", "word")
    assert (none["deletions"], none["errors"], none["rate"], none["accuracy"]) == (2, 2, 100.0, 0.0)
    over = R.pair_of_texts("a b", "", "word")
    assert (over["insertions"], over["rate"], over["accuracy"]) == (2, 200.0, 0.0)
    assert R.pair_of_texts("", "", "word")["rate"] == 0.0
    c = R.pair_of_texts("ab c", "abc", "char")
    assert (c["insertions"], c["hyp_units_n"], c["ref_units_n"], c["hyp_units"]) == (1, 4, 3, [97, 98, 32, 99])
    assert R.pair_of_texts("ab c", "abc", "char_nospace")["errors"] == 0
    # through the dictionary: pads and eos out, breaks folded, the reference's unk escaped
    p = R.pair(D, T("▁", "▁a", "b", "▁▁", "c", "</s>", "<pad>"), T("▁ab", "▁c", "▁"), "word")
    assert p["errors"] == 0 and p["hyp_units_n"] == 2
    u = R.pair(D, T("▁a", "<unk>"), T("▁a", "<unk>"), "word")
    assert u["substitutions"] == 1, "a<unk> against a<<unk>>"
    two = R.pair(D, T("a▁b▁c", "d"), T("▁a", "▁b", "▁c", "d"), "word")
    assert two["errors"] == 0 and two["ref_units_n"] == 3
    corpus = R.corpus([R.pair_of_texts("a b c", "a x c d", "word"), over])
    assert corpus == dict(errors=4, substitutions=1, insertions=2, deletions=1, ref_units=4, hyp_units=5, pairs=2, rate=100.0, accuracy=0.0)
    assert R.expected_accuracy(D, [T("▁a", "▁b")], [T("▁a", "▁b"), T("▁a")], "word") == [50.0]
    assert R.expected_accuracy(D, [T("▁a", "▁b")], [T("▁a", "▁b"), T("▁a")], "word", weights=[3.0, 1.0]) == [75.0]


@pytest.mark.parametrize("twin", sorted(R.TWINS))
def test_every_twin_differs_on_the_random_cases(twin):
    pairs = R.random_pairs(D, 11, 200)
    units = (R.TWINS[twin],) if R.TWINS[twin] else R.UNITS
    differs = sum(R.counts(R.pair(D, h, r, unit)) != R.counts(R.pair(D, h, r, unit, twin=twin)) for h, r in pairs for unit in units)
    print("%s: differs on %d of %d comparisons" % (twin, differs, len(pairs) * len(units)))
    assert differs >= 1, twin
