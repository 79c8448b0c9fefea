"""The unit kernel (csrc/text_units.hip), TextErrorRate and MBRDecoder(utility=TextErrorRate) on the GPU against the rule in plain
Python (tests/text_error_ref.py, which goes through Dictionary.string and never through the piece table, and tests/edit_ref.py).
Unit rows, counts and steps are integers: every comparison of them is exact, the slots behind a row's length included -- raw calls
fill the outputs with sentinels first and the sentinels must survive.  Token rows are padded behind their lengths with ordinary
symbols that are the same on both sides: a kernel that read past a length would find units there.  Character counts sit on both
sides of every wave boundary that matters (the kernel's waves take 64 positions each, the 256- and the 1,024-thread workgroup wrap
at 256 and 1,024), word counts on both sides of the id loop's wave steps, token widths on both sides of S2T_CHRF_GROUP_LEN, and at
the limits.  Rates are held to 1e-12 relative against Python float64 (two roundings), MBR gains to the 1e-9 of tests/test_mbr_gpu.py.
`python tests/test_text_error_gpu.py OUT.json` writes the worst rate and gain errors of a run (tests/golden/text_error_measured.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # as a script: the package lies one level up
import edit_ref as E  # noqa: E402
import text_error_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
S_INT = -7                            # sentinel of the int32 outputs
NP = {4: np.int32, 8: np.int64}
ELEMS = ((4, 4), (4, 8), (8, 4), (8, 8))
MODES = {"word": 0, "char": 1, "char_nospace": 2}
REL_RATE = 1e-12                      # the issue's bound on rates: two float64 roundings
REL_GAIN = 1e-9                       # the issue's bound on MBR gains: the one tests/test_mbr_gpu.py uses
FULL = 4095
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text_error_measured.json")
WORST = {"rate": 0.0, "rates": 0, "gain": 0.0, "gains": 0}
D = R.make_dictionary()
V, UNK, PAD, EOS = len(D), D.unk(), D.pad(), D.eos()
T = lambda *s: [D.indices[x] for x in s]
_TABLE = {}
_REFERENCE = {}


def table():
    if not _TABLE:
        from fbk_fairseq_st_amd import chrf_scorer as CS
        t = CS.piece_table(D, R.BPE)
        _TABLE["host"] = t
        _TABLE["dev"] = (torch.from_numpy(t["pieces"].view(np.int32).copy()).to(DEV), torch.from_numpy(t["piece_off"].copy()).to(DEV))
    return _TABLE


def scorer(unit="word", **kw):
    from fbk_fairseq_st_amd import text_error_rate as TE
    return TE.TextErrorRate(table()["host"], unit, **kw)


# ---------------------------------------------------------------------------------------------- calling the kernel
def padded(rows, width, elem):
    """rows behind their lengths: ordinary symbols, the same on both sides"""
    junk = T("a", "▁b", "a", ".", "▁ab", "c")
    out = np.empty((len(rows), width), NP[elem])
    for s, r in enumerate(rows):
        out[s] = [junk[(s + i) % 6] for i in range(width)]
        out[s, :len(r)] = r
    return out


def call_raw(hyp, hyp_len, ref, ref_len, mode, Uh=FULL, Ur=FULL, hyp_row=None, ref_row=None, unk=UNK, same=False):
    """s2t_text_units on numpy operands and sentinel-filled outputs -> (hyp_units, hyp_n, ref_units, ref_n, status) as numpy; same:
    ref is hyp's own memory"""
    from fbk_fairseq_st_amd import lib as L
    lib = L.load()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    th, thl = dev(hyp), dev(np.asarray(hyp_len, hyp.dtype))
    tr, trl = (th, thl) if same else (dev(ref), dev(np.asarray(ref_len, ref.dtype)))
    mh = None if hyp_row is None else dev(np.asarray(hyp_row, np.int32))
    mr = None if ref_row is None else dev(np.asarray(ref_row, np.int32))
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else hyp.shape[0]
    pieces, off = table()["dev"]
    outs = [torch.full(shape, S_INT, dtype=torch.int32, device=DEV) for shape in ((P, Uh), (P,), (P, Ur), (P,), (P,))]
    fill = torch.zeros((2,), dtype=torch.int64, device=DEV)
    p = lambda t: L.ptr(t if t.numel() else fill)
    L.check(lib.s2t_text_units(p(th), p(thl), hyp.dtype.itemsize, p(tr), p(trl), ref.dtype.itemsize, L.ptr(mh), L.ptr(mr), P, hyp.shape[1],
                               ref.shape[1], hyp.shape[0], ref.shape[0], L.ptr(pieces), L.ptr(off), pieces.shape[0], V, unk, mode, Uh, Ur,
                               p(outs[0]), p(outs[2]), L.ptr(outs[1]), L.ptr(outs[3]), L.ptr(outs[4]), L.stream()), "s2t_text_units")
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in outs)


def want_of(hyps, refs, mode, Uh=FULL, Ur=FULL, hyp_row=None, ref_row=None, twin=None, refused=()):
    """what call_raw must return: the reference's unit rows, sentinels behind them; a pair in `refused`, or with more units than a
    width, has status 2, zero lengths and sentinels"""
    unit = [u for u, m in MODES.items() if m == mode][0]
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else len(hyps)
    hr = range(P) if hyp_row is None else hyp_row
    rr = range(P) if ref_row is None else ref_row
    hu, ru = np.full((P, Uh), S_INT, np.int32), np.full((P, Ur), S_INT, np.int32)
    hn, rn, status = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32)
    for p, (h, r) in enumerate(zip(hr, rr)):
        if p in refused:
            status[p] = 2
            continue
        a, b = R.unit_rows(*R.texts_of(D, hyps[h], refs[r], twin=twin), unit, twin)
        if len(a) > Uh or len(b) > Ur:
            status[p] = 2
            continue
        hu[p, :len(a)], ru[p, :len(b)], hn[p], rn[p] = a, b, len(a), len(b)
    return hu, hn, ru, rn, status


NAMES = ("hyp_units", "hyp_n", "ref_units", "ref_n", "status")


def differs(got, want):
    """None, or the first output and pair where two results differ"""
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.nonzero((g != w).reshape(g.shape[0], -1).any(-1))[0]
        if len(bad):
            s = int(bad[0])
            at = np.nonzero(np.atleast_1d(g[s] != w[s]))[0][:4].tolist()
            return name, s, at, np.atleast_1d(g[s])[at].tolist(), np.atleast_1d(w[s])[at].tolist()
    return None


def check(hyps, refs, modes=(0, 1, 2), Uh=FULL, Ur=FULL, hyp_row=None, ref_row=None, Hmax=None, Rmax=None, elems=((8, 8),), what=""):
    """every pair in one call, for the given modes and element sizes, against the reference; returns the last mode's expectation"""
    Hmax = max([len(h) for h in hyps] + [0]) if Hmax is None else Hmax
    Rmax = max([len(r) for r in refs] + [0]) if Rmax is None else Rmax
    for mode in modes:
        want = want_of(hyps, refs, mode, Uh, Ur, hyp_row, ref_row)
        for he, re in elems:
            got = call_raw(padded(hyps, Hmax, he), [len(h) for h in hyps], padded(refs, Rmax, re), [len(r) for r in refs], mode, Uh, Ur, hyp_row, ref_row)
            assert differs(got, want) is None, (what, mode, he, re, differs(got, want))
    return want


def chars(rng, n, breaks=0.25):
    """a token row whose text has exactly n characters: single letters and word-starting letters over a small alphabet"""
    row = []
    for _ in range(n):
        u = rng.random()
        row += T("▁a" if u < breaks / 2 else "▁b" if u < breaks else "." if u < breaks + 0.05 else "a" if u < 0.65 else "b")
    return row


def long_chars(rng, n, breaks=0.2):
    """n characters in few tokens: pieces of 8, 4, 3 and 1 characters, breaks in between"""
    row = []
    while n > 0:
        s = "abcdefgh" if n >= 8 and rng.random() < 0.9 else "wxyz" if n >= 4 and rng.random() < 0.5 else "xyz" if n >= 3 and rng.random() < 0.5 else "a"
        row += T(s)
        n -= len(s)
        if rng.random() < breaks:
            row += T("▁")
    return row


def words(rng, n):
    """a token row of exactly n words over a small vocabulary with repeats: a word start, then up to two more letters"""
    row = []
    for _ in range(n):
        row += T(("▁a", "▁b", "▁ab", "▁x", "▁c")[int(rng.integers(0, 5))])
        for _ in range(int(rng.integers(0, 3))):
            row += T(("a", "b", "c", "d")[int(rng.integers(0, 4))])
    return row


def n_chars(row):
    return len("".join(R.C.text_of(D, row, R.BPE).split()))


def n_words(row):
    return len(R.C.text_of(D, row, R.BPE).split())


# ---------------------------------------------------------------------------------------------- character counts
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025))
def test_character_counts_around_every_wave_boundary(n):
    rng = np.random.default_rng(100 + n)
    for width in (None, 65):                    # the rows' own width, or at least 65 tokens: the 1,024-thread form
        hyps = [chars(rng, n), chars(rng, 70), long_chars(rng, n), chars(rng, n)[:1024]]
        refs = [chars(rng, 70), chars(rng, n), long_chars(rng, max(n - 1, 0)), long_chars(rng, n + 1)]
        hyps, refs = [h[:1024] for h in hyps], [r[:1024] for r in refs]
        assert n_chars(hyps[2]) == n and n_chars(refs[1]) == min(n, 1024)
        Hmax = max(len(h) for h in hyps) if width is None else max(width, max(len(h) for h in hyps))
        check(hyps, refs, Hmax=Hmax, what=(n, width))
    short = [long_chars(rng, n)[:64] for _ in range(3)]        # at most 64 tokens wide on both sides: the 256-thread form
    check(short, short[::-1], Hmax=64, Rmax=64, what=(n, "256 threads"))


def test_the_limits_4095_units_and_the_widest_rows():
    rng = np.random.default_rng(7)
    at, over = long_chars(rng, 4095, breaks=0.0), long_chars(rng, 4096, breaks=0.0)
    many = long_chars(rng, 3000)
    wide = chars(rng, 1024)
    assert n_chars(at) == 4095 and n_chars(over) == 4096 and n_words(at) == 1 and len(wide) == 1024 and max(len(at), len(over), len(many)) <= 1024
    hyps, refs = [at, over, at, wide, many], [at, at, over, wide[::-1], wide]
    for mode in (0, 1, 2):
        want = want_of(hyps, refs, mode, refused=(1, 2))
        got = call_raw(padded(hyps, 1024, 8), [len(h) for h in hyps], padded(refs, 1024, 4), [len(r) for r in refs], mode)
        assert differs(got, want) is None, (mode, differs(got, want))
        assert got[4].tolist() == [0, 2, 2, 0, 0] and got[1][0] == (1 if mode == 0 else 4095)
    # with spaces the spaces count: 4,000 characters in 96 words are 4,095 units, in 97 words 4,096
    def spaced(n_words_):
        row = T("abcdefgh") * 500
        for k in range(1, n_words_):
            row.insert(k * 5 + (k - 1), D.indices["▁"])
        return row
    fits, not_ = spaced(96), spaced(97)
    assert (n_chars(fits), n_words(fits), n_chars(not_), n_words(not_)) == (4000, 96, 4000, 97)
    hyps, refs = [fits, not_, fits, many[:600]], [fits, fits, not_, many[:600]]
    got = call_raw(padded(hyps, 600, 8), [len(h) for h in hyps], padded(refs, 600, 8), [len(r) for r in refs], 1)
    assert differs(got, want_of(hyps, refs, 1)) is None and got[4].tolist() == [0, 2, 2, 0] and got[1].tolist()[:2] == [4095, 0]
    for mode in (0, 2):                                                           # without spaces both fit
        got = call_raw(padded(hyps, 600, 8), [len(h) for h in hyps], padded(refs, 600, 8), [len(r) for r in refs], mode)
        assert differs(got, want_of(hyps, refs, mode)) is None and got[4].tolist() == [0] * 4
    from fbk_fairseq_st_amd import lib as L
    L.load()
    z = torch.zeros((1, 1025), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        scorer().score(z, torch.tensor([3], device=DEV), z[:, :5], torch.tensor([3], device=DEV))


# ---------------------------------------------------------------------------------------------- word counts
@pytest.mark.parametrize("total", (63, 64, 65, 255, 256, 257))
def test_word_counts_around_the_id_loops_wave_steps(total):
    rng = np.random.default_rng(200 + total)
    splits = [(total // 2, total - total // 2), (total - 1, 1), (1, total - 1), (0, total), (total, 0), (64, total - 64), (total - 64, 64)]
    splits = [(a, b) for a, b in splits if a >= 0 and b >= 0]
    hyps, refs = [words(rng, a) for a, _ in splits], [words(rng, b) for _, b in splits]
    assert all(n_words(h) + n_words(r) == total for h, r in zip(hyps, refs))
    want = check(hyps, refs, modes=(0,), what=total)
    assert want[1].tolist() == [a for a, _ in splits]
    check(hyps, refs, modes=(0,), Hmax=max(65, max(len(h) for h in hyps)), what=(total, "1,024 threads"))
    check([h[:64] for h in hyps], [r[:64] for r in refs], modes=(0, 1), Hmax=64, Rmax=64, what=(total, "256 threads"))


@pytest.mark.parametrize("widths", ((64, 64), (64, 65), (65, 64), (1024, 1024), (3, 1024)))
def test_token_widths_on_both_sides_of_the_thread_count_switch(widths):
    rng = np.random.default_rng(sum(widths))
    hyps = [words(rng, 9)[:widths[0]], chars(rng, widths[0]), [], long_chars(rng, 300)[:widths[0]]]
    refs = [words(rng, 7)[:widths[1]], chars(rng, widths[1]), chars(rng, widths[1]), []]
    check(hyps, refs, Hmax=widths[0], Rmax=widths[1], elems=((4, 8),), what=widths)


# ---------------------------------------------------------------------------------------------- the rule's corners
CASES = {
    "one word": (("▁ab",), ("▁ab",)),
    "no word": ((), ("▁a",)),
    "no word on either side": ((), ()),
    "a row of breaks only": (("▁", "▁▁", "▁"), ("▁▁",)),
    "leading, trailing and doubled breaks": (("▁", "▁▁", "a", "▁▁", "▁", "b▁", "▁"), ("▁a", "▁b")),
    "a piece with two breaks": (("a▁b▁c", "d"), ("▁a", "▁b", "▁c", "d")),
    "a piece with two breaks, joined on both sides": (("b", "a▁b▁c", "a"), ("▁b", "a", "▁b", "▁c", "a")),
    "a leading and an inner break": (("c", "▁a▁b", "c"), ("▁c", "▁a", "▁b", "c")),
    "a leading and a trailing break": (("c", "▁ab▁", "c"), ("▁c", "▁ab", "▁c")),
    "a word split across pieces": (("▁a", "b", "c"), ("▁ab", "c")),
    "words that differ in their last character": (("▁ab", "c", "▁ab", "d"), ("▁ab", "d", "▁ab", "c")),
    "a word that is a prefix of another": (("▁ab", "▁ab", "c", "▁a"), ("▁ab", "c", "▁a", "▁ab")),
    "three times on one side, once on the other": (("▁ab", "▁x", "▁ab", "▁ab"), ("▁b", "▁ab")),
    "three times on the other side": (("▁x", "▁b"), ("▁b", "▁b", "▁a", "▁b")),
    "no punctuation split": (("▁a", ".", "▁c,"), ("▁a", "▁.", "▁c", "▁c,")),
    "above U+FFFF": (("\U0001d4b3", "▁\U0001f600x", "e\u0301"), ("▁\U0001f600x", "\U0001d4b3", "e\u0301", "e\u0301")),
    "specials anywhere": (("<s>", "▁a", "<pad>", "b", "</s>", "c", "</s>"), ("▁ab", "<pad>", "c", "</s>")),
    "unk in the hypothesis": (("▁a", "▁", "<unk>", "▁b"), ("▁a", "▁b")),
    "unk in the reference": (("▁a", "▁b"), ("▁a", "▁", "<unk>", "▁b")),
    "unk on both sides": (("▁a", "▁", "<unk>", "▁", "<unk>"), ("▁a", "▁", "<unk>", "▁", "<unk>")),
    "identical": (("▁ab", "c", "▁a", "."), ("▁ab", "c", "▁a", ".")),
    "nothing in common": (("▁a", "a"), ("▁b", "c")),
}


def test_the_rules_corners():
    hyps, refs = [T(*h) for h, _ in CASES.values()], [T(*r) for _, r in CASES.values()]
    for mode in (0, 1, 2):
        check(hyps, refs, modes=(mode,), elems=ELEMS)
    hu, hn, ru, rn, _ = want_of(hyps, refs, 0)
    row = {k: (hu[s, :hn[s]].tolist(), ru[s, :rn[s]].tolist()) for s, k in enumerate(CASES)}
    assert row["a row of breaks only"] == ([], []) and row["one word"] == ([0], [0]) and row["no word"] == ([], [0])
    assert row["a piece with two breaks"] == ([0, 1, 2], [0, 1, 2]) and row["leading, trailing and doubled breaks"] == ([0, 1], [0, 1])
    assert row["words that differ in their last character"] == ([0, 1], [1, 0])
    assert row["a word that is a prefix of another"] == ([0, 1, 2], [1, 2, 0])
    assert row["three times on one side, once on the other"] == ([0, 1, 0, 0], [4, 0]) and row["three times on the other side"] == ([0, 1], [1, 1, 4, 1])
    assert row["no punctuation split"] == ([0, 1], [2, 3, 4, 1]) and row["unk on both sides"] == ([0, 1, 1], [0, 4, 4]), "<unk> is not <<unk>>"
    c = want_of(hyps, refs, 1)
    s = list(CASES).index("leading, trailing and doubled breaks")
    assert c[0][s, :c[1][s]].tolist() == [97, 32, 98] and c[1][list(CASES).index("a row of breaks only")] == 0


def test_unit_widths_n_accepted_and_n_minus_1_refused_beside_ordinary_pairs():
    rng = np.random.default_rng(9)
    hyps = [words(rng, 3), words(rng, 20), words(rng, 2), []]
    refs = [words(rng, 4), words(rng, 6), words(rng, 30), words(rng, 2)]
    for mode, unit in ((0, "word"), (1, "char"), (2, "char_nospace")):
        size = lambda row: len(R.unit_rows(R.C.text_of(D, row, R.BPE), "", unit)[0])
        nh, nr = max(size(h) for h in hyps), max(size(r) for r in refs)
        assert [size(h) == nh for h in hyps] == [False, True, False, False] and [size(r) == nr for r in refs] == [False, False, True, False]
        for Uh, Ur, status in ((nh, nr, [0, 0, 0, 0]), (nh - 1, nr, [0, 2, 0, 0]), (nh, nr - 1, [0, 0, 2, 0]), (nh - 1, nr - 1, [0, 2, 2, 0])):
            want = want_of(hyps, refs, mode, Uh, Ur)
            got = call_raw(padded(hyps, 64, 8), [len(h) for h in hyps], padded(refs, 96, 4), [len(r) for r in refs], mode, Uh, Ur)
            assert want[4].tolist() == status and differs(got, want) is None, (mode, Uh, Ur, differs(got, want))
    got = call_raw(padded(hyps, 64, 8), [len(h) for h in hyps], padded(refs, 96, 4), [len(r) for r in refs], 0, 0, 0)
    assert got[4].tolist() == [2, 2, 2, 2] and got[0].shape == (4, 0), "no room at all"
    got = call_raw(padded([[], []], 3, 8), [0, 0], padded([[], []], 3, 8), [0, 0], 0, 0, 0)
    assert got[4].tolist() == [0, 0] and got[1].tolist() == [0, 0], "nothing needs no room"


def test_refusals_beside_ordinary_pairs():
    rng = np.random.default_rng(3)
    rows = [chars(rng, 9) for _ in range(6)]
    hyp, ref = padded(rows, 12, 8), padded(rows[::-1], 12, 4)
    hyp[1, 3], hyp[2, 5], ref[1, 0] = V, -1, V + 5                                  # tokens outside [0, V): inside the lengths
    hyp[4, 10] = V + 1                                                             # behind the length: never read
    hlen, rlen = [9, 9, 9, 13, 9, 9], [9, 9, 9, 9, -1, 9]
    hyp_row, ref_row = [0, 1, 2, 3, 4, 5, 0, 6, -1, 5, 4, 0], [5, 5, 5, 5, 5, 5, 1, 0, 0, 6, 4, -2]
    refused = [s for s, st in enumerate([0, 2, 2, 2, 0, 0, 2, 2, 2, 2, 2, 2]) if st]
    for mode in (0, 1, 2):
        got = call_raw(hyp, hlen, ref, rlen, mode, 20, 20, hyp_row, ref_row)
        want = want_of(rows, rows[::-1], mode, 20, 20, [min(max(h, 0), 5) for h in hyp_row], [min(max(r, 0), 5) for r in ref_row], refused=refused)
        assert differs(got, want) is None, (mode, differs(got, want))
    # a reference-side unk without a special rendering is an ordinary token
    u = call_raw(padded([T("▁a", "<unk>")], 2, 8), [2], padded([T("▁a", "<unk>")], 2, 8), [2], 0, unk=-1)
    assert u[0][0, :1].tolist() == [0] and u[2][0, :1].tolist() == [0]


def test_maps_and_one_matrix_as_both_sides():
    rng = np.random.default_rng(4)
    rows = [words(rng, int(n)) for n in rng.integers(0, 12, size=7)]
    others = [words(rng, int(n)) for n in rng.integers(0, 12, size=5)]
    hr, rr = [6, 0, 3, 3, 1, 2, 5, 4, 0], [4, 4, 0, 1, 2, 3, 3, 0, 1]
    check(rows, others, hyp_row=hr, ref_row=rr, elems=ELEMS, what="both maps")
    check(rows, others, hyp_row=None, ref_row=[4, 3, 2, 1, 0, 0, 2], elems=ELEMS, what="the reference's map")
    check(rows, others, hyp_row=[6, 5, 4, 3, 2], ref_row=None, elems=ELEMS, what="the hypothesis' map")
    check(rows, rows[::-1], elems=ELEMS, what="no map")
    width = max(len(r) for r in rows) + 1
    for elem in (4, 8):                                                            # one matrix, its own memory, as both sides
        m, n = padded(rows, width, elem), [len(r) for r in rows]
        pairs = [(i, j) for i in range(7) for j in range(7)]
        for mode in (0, 1):
            got = call_raw(m, n, m, n, mode, 80, 80, [i for i, _ in pairs], [j for _, j in pairs], same=True)
            assert differs(got, want_of(rows, rows, mode, 80, 80, [i for i, _ in pairs], [j for _, j in pairs])) is None
        got = call_raw(m, n, m, n, 0, 80, 80, same=True)
        assert differs(got, want_of(rows, rows, 0, 80, 80)) is None


def test_a_pair_alone_and_inside_a_batch():
    rng = np.random.default_rng(5)
    hyps = [chars(rng, int(n)) for n in rng.integers(0, 120, size=64)]
    refs = [chars(rng, int(n)) for n in rng.integers(0, 120, size=64)]
    Hmax, Rmax = max(len(h) for h in hyps), max(len(r) for r in refs)
    for mode in (0, 1, 2):
        whole = call_raw(padded(hyps, Hmax, 8), [len(h) for h in hyps], padded(refs, Rmax, 8), [len(r) for r in refs], mode, 130, 130)
        assert differs(whole, want_of(hyps, refs, mode, 130, 130)) is None
        for s in (0, 17, 63):
            one = call_raw(padded(hyps, Hmax, 8)[s:s + 1], [len(hyps[s])], padded(refs, Rmax, 8)[s:s + 1], [len(refs[s])], mode, 130, 130)
            assert all(a.tobytes() == b[s:s + 1].tobytes() for a, b in zip(one, whole)), (mode, s)


# ---------------------------------------------------------------------------------------------- TextErrorRate end to end
def reference(unit):
    """the random pairs and their reference results: computed once, shared, never changed"""
    if "pairs" not in _REFERENCE:
        _REFERENCE["pairs"] = R.random_pairs(D, 11, 200)
    if unit not in _REFERENCE:
        _REFERENCE[unit] = [R.pair(D, h, r, unit) for h, r in _REFERENCE["pairs"]]
    return _REFERENCE["pairs"], _REFERENCE[unit]


def rel(g, w):
    return abs(g - w) / abs(w) if w else abs(g)


def compare_scores(out, want, te=None, record=True):
    """counts exactly, rates and accuracies within REL_RATE; returns the first difference instead of asserting when asked to"""
    ints = ("matches", "substitutions", "deletions", "insertions", "errors", "hyp_units_n", "ref_units_n")
    got = np.stack([out[k].cpu().numpy() for k in ints], 1)
    exp = np.array([[w[k] for k in ints] for w in want])
    if (got != exp).any():
        return "counts", int(np.nonzero((got != exp).any(1))[0][0])
    pairs = [(g, w["rate"]) for g, w in zip(out["sentence_rate"].tolist(), want)] + \
            [(g, w["accuracy"]) for g, w in zip(out["sentence_accuracy"].tolist(), want)]
    if te is not None:
        res, cor = te.result(), R.corpus(want)
        if {k: res[k] for k in cor if k not in ("rate", "accuracy")} != {k: cor[k] for k in cor if k not in ("rate", "accuracy")}:
            return "sums", res
        pairs += [(res["rate"], cor["rate"]), (res["accuracy"], cor["accuracy"])]
    for g, w in pairs:
        err = rel(g, w)
        if record:
            WORST["rate"], WORST["rates"] = max(WORST["rate"], err), WORST["rates"] + 1
        if err > REL_RATE:
            return "rate", g, w
    return None


@pytest.mark.parametrize("unit,ref_width", (("word", 24), ("word", 512), ("char", 24), ("char_nospace", 24), ("char", 200)))
def test_text_error_rate_end_to_end_on_random_pairs(unit, ref_width):
    """ref_width 24: unit rows of at most 64 words, the alignment's one-wave form; 512 (words) and 200 (characters): unit rows wider
    than 1,023, its workgroup form"""
    pairs, want = reference(unit)
    hyps, refs = [h for h, _ in pairs], [r for _, r in pairs]
    te = scorer(unit)
    Ur = te.unit_width(ref_width, "ref")
    assert Ur <= 64 if (unit, ref_width) == ("word", 24) else Ur > 1023 if ref_width > 24 else True
    h = torch.from_numpy(padded(hyps, 24, 8)).to(DEV)
    r = torch.from_numpy(padded(refs, ref_width, 4)).to(DEV)
    hl = torch.tensor([len(x) for x in hyps], device=DEV)
    rl = torch.tensor([len(x) for x in refs], dtype=torch.int32, device=DEV)
    out = te.score(h, hl, r, rl, ops=True)
    assert out["status"].eq(0).all() and out["sentence_rate"].dtype == torch.float64 and out["sentence_rate"].is_cuda
    assert compare_scores(out, want, te) is None, compare_scores(out, want, te)
    print("%s, reference width %d: worst relative rate error so far %.3g over %d" % (unit, ref_width, WORST["rate"], WORST["rates"]))
    ops, n_ops, hu, ru = (out[k].cpu().numpy() for k in ("ops", "n_ops", "hyp_units", "ref_units"))
    for s, w in enumerate(want):
        a, b, path = hu[s, :w["hyp_units_n"]].tolist(), ru[s, :w["ref_units_n"]].tolist(), ops[s, :n_ops[s]].tolist()
        assert a == w["hyp_units"] and b == w["ref_units"] and path == w["ops"] and E.replay(a, b, path), s
    plain = scorer(unit).score(h, hl, r, rl)
    assert sorted(plain) == sorted(k for k in out if k not in ("ops", "n_ops", "hyp_units", "ref_units"))
    assert all(torch.equal(plain[k], out[k]) for k in plain), "without ops: the same numbers"
    assert te.result_string().startswith("WER = " if unit == "word" else "CER = ")


def test_score_nbest_oracle_and_the_other_methods():
    pairs, want = reference("word")
    refs = [r for _, r in pairs[:6]]
    r = torch.from_numpy(padded(refs, 24, 8)).to(DEV)
    rl = torch.tensor([len(x) for x in refs], device=DEV)
    idx = ([0, 1, 2, 60], [], [2], [3, 3, 40], [4, 70, 4], [90, 5])
    hypos = [[{"tokens": torch.tensor(pairs[i][0], dtype=torch.int64, device=DEV)} for i in ii] for ii in idx]
    te = scorer()
    out = te.score_nbest(hypos, r, rl, accumulate="oracle")
    chosen = []
    for b, ii in enumerate(idx):
        rates = []
        for k, i in enumerate(ii):
            w = R.pair(D, pairs[i][0], refs[b], "word")
            assert int(out["errors"][b, k]) == w["errors"] and int(out["ref_units_n"][b, k]) == w["ref_units_n"]
            assert rel(float(out["sentence_rate"][b, k]), w["rate"]) <= REL_RATE and rel(float(out["sentence_accuracy"][b, k]), w["accuracy"]) <= REL_RATE
            rates.append(w["rate"])
        assert out["sentence_rate"][b, len(ii):].eq(-1).all() and out["errors"][b, len(ii):].eq(0).all()
        best = min(range(len(ii)), key=lambda k: (rates[k], k)) if ii else 0
        assert int(out["oracle"][b]) == best and int(out["n_hyp"][b]) == len(ii)
        if ii:
            chosen.append(R.pair(D, pairs[ii[best]][0], refs[b], "word"))
    assert {k: te.result()[k] for k in ("errors", "ref_units", "pairs")} == \
        {k: R.corpus(chosen)[k] for k in ("errors", "ref_units", "pairs")}
    top = scorer().score_hypotheses(hypos, r, rl)
    assert top["errors"].tolist() == [R.pair(D, pairs[ii[0]][0] if ii else [], refs[b], "word")["errors"] for b, ii in enumerate(idx)]
    # score_pairs on maps equals score on repeated rows, bit for bit
    hyps = [h for h, _ in pairs[:6]]
    h, hl = torch.from_numpy(padded(hyps, 24, 4)).to(DEV), torch.tensor([len(x) for x in hyps], dtype=torch.int32, device=DEV)
    hr, rr = [0, 1, 2, 3, 4, 5, 5, 0], [0, 0, 1, 1, 2, 3, 0, 3]
    a, b = scorer("char"), scorer("char")
    got = a.score_pairs(h, hl, torch.tensor(hr, device=DEV), r, rl, torch.tensor(rr, dtype=torch.int32, device=DEV))
    rep = b.score(h[hr], hl[hr], r[rr], rl[rr])
    assert all(torch.equal(got[k], rep[k]) for k in got) and a.result() == b.result() and a.result()["ref_units"] > 0


# ---------------------------------------------------------------------------------------------- MBR with the text utility
def mbr_lists(seed, sizes):
    rng = np.random.default_rng(seed)
    lists = []
    for n in sizes:
        base = words(rng, 8)
        rows = []
        for _ in range(n):
            row = list(base)
            for _ in range(int(rng.integers(0, 5))):
                row[int(rng.integers(0, len(row)))] = T("a", "b", "▁a", "▁b", ".", "c", "▁x")[int(rng.integers(0, 7))]
            rows.append(row[:int(rng.integers(max(len(row) - 4, 1), len(row) + 1))] + [EOS])
        lists.append(rows)
    return lists


def check_rerank(out, lists, want, hypos):
    for b, (hs, gains) in enumerate(zip(out, want)):
        assert sorted(h["mbr_index"] for h in hs) == list(range(len(lists[b])))
        got = [float(h["mbr_score"]) for h in hs]
        assert got == sorted(got, reverse=True) and all(h is hypos[b][h["mbr_index"]] and h["mbr_score"].is_cuda for h in hs)
        for h in hs:
            err = rel(float(h["mbr_score"]), gains[h["mbr_index"]])
            WORST["gain"], WORST["gains"] = max(WORST["gain"], err), WORST["gains"] + 1
            assert err <= REL_GAIN, (b, h["mbr_index"], float(h["mbr_score"]), gains[h["mbr_index"]])
        order = sorted(range(len(gains)), key=lambda i: (-gains[i], i))
        near = any(0 < abs(gains[i] - gains[j]) <= REL_GAIN * gains[i] for i in order for j in order)
        assert [h["mbr_index"] for h in hs] == order or near, (b, order)


def test_mbr_with_the_text_error_utility():
    from fbk_fairseq_st_amd import mbr as MB
    lists = mbr_lists(41, (1, 2, 3, 4, 0, 40))
    lists[3][2] = list(lists[3][0])                                                # a planted duplicate: an exact tie
    hypos = [[{"tokens": torch.tensor(t, device=DEV)} for t in ts] for ts in lists]
    for unit in ("word", "char"):
        want = [R.expected_accuracy(D, ts, ts, unit) for ts in lists]
        dec = MB.MBRDecoder(None, PAD, EOS, UNK, utility=scorer(unit))
        check_rerank(dec.rerank(hypos), lists, want, hypos)
    # separate pseudo-references and weights
    pseudo = mbr_lists(42, (3, 3, 2, 5, 4, 7))
    w = [0.5, 2.0, 1.0, 0.0, 3.0, 1.5, 0.25]
    want = [R.expected_accuracy(D, ts, ps, "word", weights=w) for ts, ps in zip(lists, pseudo)]
    out = MB.MBRDecoder(None, PAD, EOS, UNK, utility=scorer()).rerank(hypos, pseudo=[[{"tokens": torch.tensor(t, device=DEV)} for t in ps]
                                                                                    for ps in pseudo], weights=w)
    check_rerank(out, lists, want, hypos)
    print("worst relative gain error so far %.3g over %d" % (WORST["gain"], WORST["gains"]))


def test_generate_through_the_task_on_the_device_search():
    """fixture case `c` through the device-resident sampling search, 8 samples per sentence, reordered by expected word accuracy of
    the dictionary's words (bpe None: every symbol is a word)"""
    import test_model_gpu as TM
    from fbk_fairseq_st_amd import mbr as MB
    from fbk_fairseq_st_amd import text_error_rate as TE
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    task, model, src, lens, opts, exp, _ = TM.build_gen("c")
    d = task.target_dictionary
    sample = dict(net_input=dict(src_tokens=src, src_lengths=lens))
    opts = dict(opts, beam_size=8)
    mk = lambda: SequenceGenerator([model], d, search_strategy=Sampling(d, sampling_topk=10, seed=5), **opts)
    plain = mk().generate([model], sample)
    gen = mk()
    dec = MB.MBRDecoder.for_dictionary(gen, d, utility=TE.TextErrorRate.for_dictionary(d, bpe=None, unit="word"))
    out = task.inference_step(dec, [model], sample)
    assert "launches_per_step" in gen.last_stats, "the search did not take the device route"
    lists = [[h["tokens"].tolist() for h in hs] for hs in plain]
    want = [R.expected_accuracy(d, ts, ts, "word", bpe=None) for ts in lists]
    for b, (hs, gains) in enumerate(zip(out, want)):
        assert sorted(h["mbr_index"] for h in hs) == list(range(8)), "a permutation of the generator's list"
        for h in hs:
            assert h["tokens"].tolist() == lists[b][h["mbr_index"]] and h["mbr_score"].is_cuda and h["mbr_score"].dtype == torch.float64
            assert rel(float(h["mbr_score"]), gains[h["mbr_index"]]) <= REL_GAIN, (b, h["mbr_index"])
        order = sorted(range(8), key=lambda i: (-gains[i], i))
        near = any(0 < abs(gains[i] - gains[j]) <= REL_GAIN * gains[i] for i in order for j in order)
        assert [h["mbr_index"] for h in hs] == order or near, (b, order, gains)


# ---------------------------------------------------------------------------------------------- the comparisons can fail
def test_wrong_twins_fail_this_files_comparisons():
    pairs, _ = reference("word")
    hyps, refs = [h for h, _ in pairs], [r for _, r in pairs]
    Hmax = Rmax = 24
    raw = {mode: call_raw(padded(hyps, Hmax, 8), [len(h) for h in hyps], padded(refs, Rmax, 8), [len(r) for r in refs], mode, 200, 200) for mode in (0, 1, 2)}
    outs = {}
    for unit in MODES:
        outs[unit] = scorer(unit).score(torch.from_numpy(padded(hyps, Hmax, 8)).to(DEV), torch.tensor([len(h) for h in hyps], device=DEV),
                                        torch.from_numpy(padded(refs, Rmax, 8)).to(DEV), torch.tensor([len(r) for r in refs], device=DEV))
        assert differs(raw[MODES[unit]], want_of(hyps, refs, MODES[unit], 200, 200)) is None
        assert compare_scores(outs[unit], reference(unit)[1], record=False) is None
    for twin, unit in R.TWINS.items():
        for u in ((unit,) if unit else tuple(MODES)):
            assert differs(raw[MODES[u]], want_of(hyps, refs, MODES[u], 200, 200, twin=twin)) is not None, (twin, u)
            wrong = [R.pair(D, h, r, u, twin=twin) for h, r in pairs]
            assert compare_scores(outs[u], wrong, record=False) is not None, (twin, u)
    good = raw[0]
    assert differs(good, (good[0], good[1] + (np.arange(200) == 5), good[2], good[3], good[4])) is not None
    assert differs(good, good[:4] + (2 - good[4],)) is not None and differs(good, (good[0] + (good[0] == S_INT),) + good[1:]) is not None
    off = [dict(w, rate=w["rate"] * (1 + 1e-11)) for w in reference("word")[1]]
    assert compare_scores(outs["word"], off, record=False) is not None, "a rate 1e-11 away is outside the bound"


# ---------------------------------------------------------------------------------------------- the measured file
def test_measured_file_lies_within_the_bounds():
    """tests/golden/text_error_measured.json: the worst relative rate and gain errors of a run of this file on an MI355X (written by
    running the file as a script).  It sets no bound -- the bounds are REL_RATE and REL_GAIN -- but it must lie within them."""
    with open(MEASURED) as f:
        m = json.load(f)
    assert m["rate_bound"] == REL_RATE and 0 <= m["rate_worst"] <= REL_RATE and m["rates"] > 0
    assert m["gain_bound"] == REL_GAIN and 0 <= m["gain_worst"] <= REL_GAIN and m["gains"] > 0


if __name__ == "__main__":
    rc = pytest.main([os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"])
    W = sys.modules["test_text_error_gpu"].WORST                           # the module pytest imported holds the run's figures
    out = {"rate_worst": W["rate"], "rates": W["rates"], "rate_bound": REL_RATE, "gain_worst": W["gain"], "gains": W["gains"], "gain_bound": REL_GAIN,
           "note": "worst relative error of TextErrorRate's sentence_rate, sentence_accuracy and result() rates, and of MBRDecoder's gains "
                   "under the TextErrorRate utility, against Python float64 (tests/text_error_ref.py) over the cases of "
                   "tests/test_text_error_gpu.py on an MI355X; the tests hold every rate and gain to the bounds"}
    if len(sys.argv) > 1 and W["rates"] and W["gains"]:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))
