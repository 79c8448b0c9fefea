"""chrF / chrF++ in plain Python, on strings with collections.Counter: the rule of DESIGN.md 5j, as the reference the kernel and the
piece table are tested against.  Token rows become text through `Dictionary.string` (pads stripped first, as generate.py does), never
through the piece table.  The `twin` argument switches on one deliberate mistake, for the tests that show the comparisons can fail."""
import functools
import string
from collections import Counter

PUNCT = set(string.punctuation)
TWINS = ("keep_space", "no_clip", "first_rule_first", "all_orders", "beta_other_side")


def text_of(dictionary, row, bpe, reference_side=False):
    """the normalised text of a token row: pads out, Dictionary.string (eos and bos dropped, unk escaped on the reference side),
    whitespace runs folded"""
    toks = [int(t) for t in row if int(t) != dictionary.pad()]
    return " ".join(dictionary.string(toks, bpe, escape_unk=reference_side).split())


def split_word(w, twin=None):
    if len(w) == 1:
        return [w]
    last, first = w[-1] in PUNCT, w[0] in PUNCT
    if twin == "first_rule_first":
        if first:
            return [w[0], w[1:]]
        if last:
            return [w[:-1], w[-1]]
        return [w]
    if last:
        return [w[:-1], w[-1]]
    if first:
        return [w[0], w[1:]]
    return [w]


def words_of(text, twin=None):
    return [p for w in text.split() for p in split_word(w, twin)]


def ngrams(seq, n):
    return Counter(tuple(seq[i:i + n]) for i in range(len(seq) - n + 1))


@functools.lru_cache(maxsize=4096)
def side_counts(text, twin=None):
    """the eight n-gram tables of one side: characters of the orders 1 .. 6, then words of the orders 1 .. 2"""
    chars = " ".join(text.split()) if twin == "keep_space" else "".join(text.split())
    words = words_of(text, twin)
    return tuple(ngrams(chars, n) for n in range(1, 7)) + tuple(ngrams(words, n) for n in range(1, 3))


def pair_stats(hyp_text, ref_text, char_order=6, word_order=0, twin=None):
    """-> 24 integers: (hyp_n, ref_n, match_n) of the character orders 1 .. 6, then of the word orders 1 .. 2; zeros above the
    configured orders"""
    out = [0] * 24
    hc, rc = side_counts(hyp_text, twin), side_counts(ref_text, twin)
    for k in list(range(char_order)) + list(range(6, 6 + word_order)):
        ca, cb = hc[k], rc[k]
        match = sum(c if twin == "no_clip" else min(c, cb[g]) for g, c in ca.items() if g in cb)
        out[3 * k:3 * k + 3] = [sum(ca.values()), sum(cb.values()), match]
    return out


def score(stats, char_order=6, word_order=0, beta=2.0, twin=None):
    """24 integers -> chrF in percent, float64"""
    idx = list(range(char_order)) + list(range(6, 6 + word_order))
    ps, rs = [], []
    for k in idx:
        hyp, ref, match = stats[3 * k:3 * k + 3]
        if hyp > 0 and ref > 0:
            ps.append(match / hyp)
            rs.append(match / ref)
        elif twin == "all_orders":
            ps.append(0.0)
            rs.append(0.0)
    if not ps:
        return 0.0
    p, r = sum(ps) / len(ps), sum(rs) / len(rs)
    if twin == "beta_other_side":
        p, r = r, p
    if p + r == 0:
        return 0.0
    return 100.0 * (1 + beta * beta) * p * r / (beta * beta * p + r)


def row_stats(dictionary, hyp_row, ref_row, bpe, char_order=6, word_order=0, twin=None):
    return pair_stats(text_of(dictionary, hyp_row, bpe, False), text_of(dictionary, ref_row, bpe, True), char_order, word_order, twin)


def corpus_score(rows, char_order=6, word_order=0, beta=2.0):
    """the score of the sums of several pairs' statistics"""
    sums = [sum(r[k] for r in rows) for k in range(24)]
    return score(sums, char_order, word_order, beta)


def expected_chrf(dictionary, cands, pseudo, bpe, weights=None, char_order=6, word_order=0, beta=2.0):
    """MBR gains of one sentence: for every candidate row the weighted mean over the pseudo-reference rows of the pair's score"""
    w = [1.0] * len(pseudo) if weights is None else [float(x) for x in weights[:len(pseudo)]]
    gains = []
    for c in cands:
        us = [score(row_stats(dictionary, c, q, bpe, char_order, word_order), char_order, word_order, beta) for q in pseudo]
        mass = sum(w)
        gains.append(sum(a * u for a, u in zip(w, us)) / mass if mass > 0 else 0.0)
    return gains


# ---------------------------------------------------------------------------------------------- a dictionary for the tests
SYMBOLS = ("a", "b", "▁a", "▁b", "▁", "a▁b", ".", "▁.", "(", ")", "▁ab", "c", "▁▁", "e\u0301",
           "\U0001d4b3", "▁\U0001f600x", "abcdefgh", "wxyz", "xyz", "b▁", "▁c,")


def make_dictionary():
    """sentencepiece-style symbols (ids from 4, in the order of SYMBOLS): single characters, word starts, a bare break, a piece that
    holds two words, punctuation, a doubled break, a combining sequence, code points above U+FFFF, pieces of 8, 4 and 3 characters
    (to reach a character count with few tokens), a trailing break"""
    from fbk_fairseq_st_amd.data import Dictionary
    d = Dictionary()
    for s in SYMBOLS:
        d.add_symbol(s)
    return d


def tok(d, *symbols):
    return [d.indices[s] for s in symbols]
