"""WER / CER of detokenised token rows in plain Python: the rule of DESIGN.md 5k, as the reference the unit kernel and TextErrorRate are
tested against.  Token rows become text through `chrf_ref.text_of` (`Dictionary.string`), never through the piece table; words are
`text.split()`, characters `list(text)` or `list(text.replace(" ", ""))`; the alignment and its counts come from `edit_ref.align`
with the costs (1, 1, 1), tie rule included.  The `twin` argument switches on one deliberate mistake, for the tests that show the
comparisons can fail."""
import numpy as np

import chrf_ref as C
import edit_ref as E

UNITS = ("word", "char", "char_nospace")
TWINS = {"punct_split": "word", "drop_space": "char", "ids_per_side": "word", "same_length_equal": "word", "unk_matches": None}   # -> its unit
COUNTS = ("matches", "substitutions", "deletions", "insertions", "errors", "hyp_units_n", "ref_units_n")
BPE = "sentencepiece"


def texts_of(dictionary, hyp_row, ref_row, bpe=BPE, twin=None):
    return C.text_of(dictionary, hyp_row, bpe, False), C.text_of(dictionary, ref_row, bpe, twin != "unk_matches")


def _first_ids(words, key, base=0, seen=None):
    seen = {} if seen is None else seen
    out = []
    for k, w in enumerate(words):
        out.append(seen.setdefault(key(w), base + k))
    return out, seen


def unit_rows(hyp_text, ref_text, unit, twin=None):
    """the two unit rows as lists of integers: for words the index of a word's first equal occurrence in "hypothesis words, then
    reference words", for characters the code points"""
    if unit == "word":
        split = (lambda t: C.words_of(t)) if twin == "punct_split" else (lambda t: t.split())
        hw, rw = split(hyp_text), split(ref_text)
        key = (lambda w: (len(w), w[0])) if twin == "same_length_equal" else (lambda w: w)
        hu, seen = _first_ids(hw, key)
        ru, _ = _first_ids(rw, key, len(hw), None if twin == "ids_per_side" else seen)
        return hu, ru
    if unit == "char" and twin != "drop_space":
        return [ord(c) for c in hyp_text], [ord(c) for c in ref_text]
    if unit in ("char", "char_nospace"):
        return [ord(c) for c in hyp_text.replace(" ", "")], [ord(c) for c in ref_text.replace(" ", "")]
    raise ValueError(unit)


def align(a, b):
    return E.align(a, b) if len(a) * len(b) <= 40000 else E.align_np(a, b)


def pair_of_texts(hyp_text, ref_text, unit, twin=None):
    """-> dict: the COUNTS, `ops`, the unit rows, `rate` and `accuracy`"""
    hu, ru = unit_rows(hyp_text, ref_text, unit, twin)
    _, (m, s, b, a), ops = align(hu, ru)
    out = dict(matches=m, substitutions=s, deletions=b, insertions=a, errors=s + b + a, hyp_units_n=len(hu), ref_units_n=len(ru),
               ops=ops, hyp_units=hu, ref_units=ru)
    out["rate"] = rate(out["errors"], len(ru))
    out["accuracy"] = accuracy(out["rate"])
    return out


def pair(dictionary, hyp_row, ref_row, unit, bpe=BPE, twin=None):
    return pair_of_texts(*texts_of(dictionary, hyp_row, ref_row, bpe, twin), unit, twin)


def counts(p):
    return [p[k] for k in COUNTS]


def rate(errors, ref_n):
    return 100.0 * errors / max(ref_n, 1)


def accuracy(r):
    return 100.0 - min(r, 100.0)


def corpus(pairs):
    """the sums TextErrorRate.result() holds, with rate and accuracy"""
    out = {k: sum(p[k] for p in pairs) for k in ("errors", "substitutions", "insertions", "deletions")}
    out.update(ref_units=sum(p["ref_units_n"] for p in pairs), hyp_units=sum(p["hyp_units_n"] for p in pairs), pairs=len(pairs))
    out["rate"] = rate(out["errors"], out["ref_units"])
    out["accuracy"] = accuracy(out["rate"])
    return out


def expected_accuracy(dictionary, cands, pseudo, unit, bpe=BPE, weights=None):
    """MBR gains of one sentence: for every candidate row the weighted mean over the pseudo-reference rows of the pair's accuracy"""
    w = [1.0] * len(pseudo) if weights is None else [float(x) for x in weights[:len(pseudo)]]
    gains = []
    for c in cands:
        us = [pair(dictionary, c, q, unit, bpe)["accuracy"] for q in pseudo]
        mass = sum(w)
        gains.append(sum(a * u for a, u in zip(w, us)) / mass if mass > 0 else 0.0)
    return gains


# ---------------------------------------------------------------------------------------------- a dictionary and cases for the tests
SYMBOLS = C.SYMBOLS + ("▁a▁b", "a▁b▁c", "d", "▁ab▁", "▁x", "▁c")


def make_dictionary():
    """chrf_ref's symbols, then pieces with two breaks (leading and inner, two inner, leading and trailing), a letter that makes words
    differ in their last character, and one more word start"""
    from fbk_fairseq_st_amd.data import Dictionary
    d = Dictionary()
    for s in SYMBOLS:
        d.add_symbol(s)
    return d


RANDOM_SYMBOLS = ("a", "b", "▁a", "▁b", "▁", ".", "▁.", "c", "d", "▁ab", "a▁b", "▁a▁b", "a▁b▁c", "▁c,", "b▁", "<unk>", "▁x", "e\u0301")


def random_pairs(dictionary, seed, n, longest=24):
    """n pairs of token rows over a small alphabet: a reference, and a hypothesis that is the reference with a few tokens replaced,
    dropped or inserted (every tenth pair: two unrelated rows; some rows empty)"""
    rng = np.random.default_rng(seed)
    ids = [dictionary.indices[s] if s in dictionary.indices else dictionary.unk() for s in RANDOM_SYMBOLS]
    draw = lambda k: [ids[int(i)] for i in rng.integers(0, len(ids), size=k)]
    pairs = []
    for p in range(n):
        ref = draw(int(rng.integers(0, longest + 1)))
        if p % 10 == 9:
            hyp = draw(int(rng.integers(0, longest + 1)))
        else:
            hyp = list(ref)
            for _ in range(int(rng.integers(0, 5))):
                u, at = rng.random(), int(rng.integers(0, len(hyp) + 1))
                if u < 0.4 and at < len(hyp):
                    hyp[at] = draw(1)[0]
                elif u < 0.7 and at < len(hyp):
                    del hyp[at]
                elif len(hyp) < longest:
                    hyp.insert(at, draw(1)[0])
        pairs.append((hyp, ref))
    return pairs


def table_text(table, row, reference_side=False):
    """the text a piece table gives a row, read the way the kernel reads it: the row's pieces in order, SEP as a space, whitespace
    folded; None for a token outside the table"""
    pieces, off, out = table["pieces"], table["piece_off"], []
    for t in row:
        t = int(t)
        if not 0 <= t < table["V"]:
            return None
        e = table["V"] if reference_side and t == table["unk"] else t
        out += [" " if c == 0xffffffff else chr(c) for c in pieces[off[e]:off[e + 1]].tolist()]
    return " ".join("".join(out).split())
