"""The chrF statistics kernel (csrc/chrf_stats.hip), ChrfScorer and MBRDecoder(utility=scorer) on the GPU against the rule in plain
Python (tests/chrf_ref.py, which goes through Dictionary.string and never through the piece table).  The statistics are integers:
every comparison of them is exact.  Raw calls fill the outputs with sentinels first, and rows are padded behind their lengths with
ordinary symbols that are the same on both sides: a kernel that read past a length would find matches there.  Character counts sit
on both sides of every wave boundary that matters (the kernel's waves take 64 positions each: 63 / 64 / 65, and 255 / 256 / 257 and
1,023 / 1,024 / 1,025 where the 256- and the 1,024-thread workgroup wrap around), widths on both sides of S2T_CHRF_GROUP_LEN, and
at the limits.  Scores are held to 1e-9 relative against Python float64.
`python tests/test_chrf_gpu.py OUT.json` writes the worst score error of a run (tests/golden/chrf_measured.json)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))     # as a script: the package lies one level up
import chrf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
S_INT = -7                            # sentinel of the int32 outputs
NP = {4: np.int32, 8: np.int64}
ELEMS = ((4, 4), (4, 8), (8, 4), (8, 8))
REL = 1e-9                            # the issue's bound: the one the MBR gains carry
BPE = "sentencepiece"
MEASURED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chrf_measured.json")
WORST = {"score": 0.0, "scores": 0}
D = R.make_dictionary()
V, UNK, PAD, EOS = len(D), D.unk(), D.pad(), D.eos()
T = lambda *s: R.tok(D, *s)
_TABLE = {}


def table():
    if not _TABLE:
        from fbk_fairseq_st_amd import chrf_scorer as CS
        t = CS.piece_table(D, BPE)
        _TABLE["host"] = t
        _TABLE["dev"] = (torch.from_numpy(t["pieces"].view(np.int32).copy()).to(DEV), torch.from_numpy(t["piece_off"].copy()).to(DEV))
    return _TABLE


def scorer(**kw):
    from fbk_fairseq_st_amd import chrf_scorer as CS
    return CS.ChrfScorer(table()["host"], **kw)


# ---------------------------------------------------------------------------------------------- calling the kernel
def padded(rows, width, elem):
    """rows behind their lengths: ordinary symbols, the same on both sides"""
    junk = T("a", "▁b", "a", ".", "▁ab", "c")
    out = np.empty((len(rows), width), NP[elem])
    for s, r in enumerate(rows):
        out[s] = [junk[(s + i) % 6] for i in range(width)]
        out[s, :len(r)] = r
    return out


def call_raw(hyp, hyp_len, ref, ref_len, hyp_row=None, ref_row=None, co=6, wo=2, unk=UNK, same=False, v=None):
    """s2t_chrf_stats on numpy operands and sentinel-filled outputs -> (stats, status) as numpy; same: ref is hyp's own memory"""
    from fbk_fairseq_st_amd import lib as L
    lib = L.load()
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    th, thl = dev(hyp), dev(np.asarray(hyp_len, hyp.dtype))
    tr, trl = (th, thl) if same else (dev(ref), dev(np.asarray(ref_len, ref.dtype)))
    mh = None if hyp_row is None else dev(np.asarray(hyp_row, np.int32))
    mr = None if ref_row is None else dev(np.asarray(ref_row, np.int32))
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else hyp.shape[0]
    pieces, off = table()["dev"]
    stats = torch.full((P, 24), S_INT, dtype=torch.int32, device=DEV)
    status = torch.full((P,), S_INT, dtype=torch.int32, device=DEV)
    fill = torch.zeros((2,), dtype=torch.int64, device=DEV)
    p = lambda t: L.ptr(t if t.numel() else fill)
    L.check(lib.s2t_chrf_stats(p(th), p(thl), hyp.dtype.itemsize, p(tr), p(trl), ref.dtype.itemsize, L.ptr(mh), L.ptr(mr), P, hyp.shape[1],
                               ref.shape[1], hyp.shape[0], ref.shape[0], L.ptr(pieces), L.ptr(off), pieces.shape[0], V if v is None else v,
                               unk, co, wo, L.ptr(stats), L.ptr(status), L.stream()), "s2t_chrf_stats")
    torch.cuda.synchronize()
    return stats.cpu().numpy(), status.cpu().numpy()


def differs(got, want, got_status=None, want_status=None):
    """None, or the first pair where two sets of statistics differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = np.nonzero((got != want).any(-1))[0]
    if len(bad):
        return int(bad[0]), got[bad[0]].tolist(), want[bad[0]].tolist()
    if got_status is not None and (np.asarray(got_status) != np.asarray(want_status)).any():
        return "status", np.asarray(got_status).tolist(), np.asarray(want_status).tolist()
    return None


def want_of(hyps, refs, hyp_row=None, ref_row=None, co=6, wo=2, twin=None):
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else len(hyps)
    hr = range(P) if hyp_row is None else hyp_row
    rr = range(P) if ref_row is None else ref_row
    return np.array([R.row_stats(D, hyps[h], refs[r], BPE, co, wo, twin) for h, r in zip(hr, rr)], np.int32).reshape(P, 24)


def check(hyps, refs, hyp_row=None, ref_row=None, co=6, wo=2, Hmax=None, Rmax=None, elems=((8, 8),), what=""):
    """every pair in one call, for the given element sizes, against the reference; returns the statistics"""
    Hmax = max([len(h) for h in hyps] + [0]) if Hmax is None else Hmax
    Rmax = max([len(r) for r in refs] + [0]) if Rmax is None else Rmax
    want = want_of(hyps, refs, hyp_row, ref_row, co, wo)
    for he, re in elems:
        got, status = call_raw(padded(hyps, Hmax, he), [len(h) for h in hyps], padded(refs, Rmax, re), [len(r) for r in refs], hyp_row, ref_row, co, wo)
        assert differs(got, want, status, np.zeros(len(want), np.int32)) is None, (what, he, re, differs(got, want, status, np.zeros(len(want), np.int32)))
    return want


def chars(rng, n, breaks=0.25):
    """a token row whose text has exactly n characters: single letters and word-starting letters over a small alphabet, with a
    sprinkling of punctuation"""
    row = []
    for _ in range(n):
        u = rng.random()
        row += T("▁a" if u < breaks / 2 else "▁b" if u < breaks else "." if u < breaks + 0.05 else "a" if u < 0.65 else "b")
    return row


def long_chars(rng, n):
    """n characters in few tokens: pieces of 8, 4, 3 and 1 characters, breaks in between"""
    row = []
    while n > 0:
        s = "abcdefgh" if n >= 8 and rng.random() < 0.9 else "wxyz" if n >= 4 and rng.random() < 0.5 else "xyz" if n >= 3 and rng.random() < 0.5 else "a"
        row += T(s)
        n -= len(s)
        if rng.random() < 0.2:
            row += T("▁")
    return row


def n_chars(row):
    return len("".join(R.text_of(D, row, BPE).split()))


def check_scores(hyps, refs, co, wo, beta=2.0):
    """ChrfScorer.score on device matrices: statistics exactly, sentence and corpus score within REL"""
    sc = scorer(char_order=co, word_order=wo, beta=beta)
    Hmax, Rmax = max(len(h) for h in hyps), max(len(r) for r in refs)
    out = sc.score(torch.from_numpy(padded(hyps, Hmax, 8)).to(DEV), torch.tensor([len(h) for h in hyps], device=DEV),
                   torch.from_numpy(padded(refs, Rmax, 4)).to(DEV), torch.tensor([len(r) for r in refs], dtype=torch.int32, device=DEV))
    want = want_of(hyps, refs, co=co, wo=wo)
    assert differs(out["stats"].cpu().numpy(), want, out["status"].cpu().numpy(), np.zeros(len(want))) is None
    assert out["sentence_chrf"].dtype == torch.float64 and out["sentence_chrf"].is_cuda
    pairs = [(float(g), R.score(w.tolist(), co, wo, beta)) for g, w in zip(out["sentence_chrf"].cpu(), want)]
    pairs.append((sc.result()["chrf"], R.corpus_score(want.tolist(), co, wo, beta)))
    for g, w in pairs:
        err = abs(g - w) / w if w else abs(g)
        print("chrf %.15g reference %.15g relative error %.3g" % (g, w, err))
        WORST["score"], WORST["scores"] = max(WORST["score"], err), WORST["scores"] + 1
        assert err <= REL, (g, w)
    return out


# ---------------------------------------------------------------------------------------------- character counts
def test_character_counts_0_to_8_on_both_sides():
    """orders vanish one by one; all 81 combinations in one call, for every order configuration"""
    rng = np.random.default_rng(1)
    side = [chars(rng, n) for n in range(9)]
    hyps, refs = [side[i] for i in range(9) for _ in range(9)], [chars(rng, j) for _ in range(9) for j in range(9)]
    assert [n_chars(s) for s in side] == list(range(9))
    for co, wo in ((6, 2), (6, 0), (1, 1), (3, 0)):
        want = check(hyps, refs, co=co, wo=wo, elems=ELEMS if co == 6 else ((4, 8),), what=(co, wo))
        assert (want[:, 3 * co:18] == 0).all() and (want[:, 18 + 3 * wo:] == 0).all(), "zeros above the configured orders"
    assert want_of(hyps, refs)[9 * 3 + 8, :18:3].tolist() == [3, 2, 1, 0, 0, 0], "three characters have three orders"
    check_scores(hyps, refs, 6, 2)
    check_scores(hyps, refs, 6, 0)


@pytest.mark.parametrize("n", (63, 64, 65, 255, 256, 257, 1023, 1024, 1025))
def test_character_counts_around_every_wave_boundary(n):
    rng = np.random.default_rng(n)
    for width in (None, 65):                    # the rows' own width, or at least 65 tokens: the 1,024-thread form
        hyps = [chars(rng, n), chars(rng, 70), long_chars(rng, n), chars(rng, n)[:1024]]
        refs = [chars(rng, 70), chars(rng, n), long_chars(rng, n - 1), long_chars(rng, n + 1)]
        hyps, refs = [h[:1024] for h in hyps], [r[:1024] for r in refs]
        assert n_chars(hyps[2]) == n
        Hmax = max(len(h) for h in hyps) if width is None else max(width, max(len(h) for h in hyps))
        check(hyps, refs, Hmax=Hmax, what=(n, width))
    short = [long_chars(rng, n)[:64] for _ in range(3)]        # at most 64 tokens wide: the 256-thread form
    check(short, [long_chars(rng, n) for _ in range(3)], Hmax=64, what=(n, "256 threads"))
    check(short, short, Hmax=len(max(short, key=len)), wo=0, what=(n, "itself"))


def test_the_character_limit_and_the_widest_rows():
    rng = np.random.default_rng(7)
    at, over = long_chars(rng, 4095), long_chars(rng, 4096)
    wide = chars(rng, 1024)
    assert n_chars(at) == 4095 and n_chars(over) == 4096 and len(wide) == 1024 and max(len(at), len(over)) <= 1024
    hyps, refs = [at, over, at, wide, at], [at, at, over, wide[::-1], wide]
    want = want_of(hyps, refs)
    want[1] = want[2] = 0
    got, status = call_raw(padded(hyps, 1024, 8), [len(h) for h in hyps], padded(refs, 1024, 4), [len(r) for r in refs])
    assert differs(got, want, status, [0, 2, 2, 0, 0]) is None, differs(got, want, status, [0, 2, 2, 0, 0])
    assert got[0, 2] == 4095 and got[0, 17] == 4090
    from fbk_fairseq_st_amd import lib as L
    L.load()
    z = torch.zeros((1, 1025), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        scorer().score(z, torch.tensor([3], device=DEV), z[:, :5], torch.tensor([3], device=DEV))


# ---------------------------------------------------------------------------------------------- the rule's corners
CASES = {
    "clipping": (("▁a", "a", "a", "a"), ("▁a", "a")),
    "clipping back": (("▁a", "a"), ("▁a", "a", "a", "a")),
    "leading, trailing and doubled breaks": (("▁", "▁▁", "a", "▁▁", "▁", "b▁", "▁"), ("▁a", "▁b")),
    "only breaks": (("▁", "▁▁"), ("▁a",)),
    "a word split across pieces": (("▁a", "b", "c"), ("▁ab", "c")),
    "a piece holding two words": (("a▁b",), ("▁a", "▁b")),
    "a piece holding two words, joined on both sides": (("b", "a▁b", "a"), ("▁ab", "▁b", "a")),
    "a.": (("▁a", "."), ("▁a", "▁.")),
    ".a": (("▁.", "a"), ("▁.", "▁a")),
    ".": (("▁.",), (".",)),
    "a.b": (("▁a", ".", "b"), ("▁a", "▁.", "▁b")),
    "..": (("▁.", "."), ("▁.", "▁.")),
    "(a)": (("▁", "(", "a", ")"), ("▁", "(", "a", "▁", ")")),
    "(a) the other way": (("▁", "(", "a", ")"), ("▁", "(", "▁a", ")")),
    "c, and a trailing comma": (("▁c,", "▁c,"), ("c", "▁c,")),
    "above U+FFFF": (("\U0001d4b3", "▁\U0001f600x", "é"), ("▁\U0001f600x", "\U0001d4b3", "é", "é")),
    "specials anywhere": (("<s>", "▁a", "<pad>", "b", "</s>", "c", "</s>"), ("▁ab", "<pad>", "c", "</s>")),
    "unk in the hypothesis": (("▁a", "<unk>", "▁b"), ("▁a", "▁b")),
    "unk in the reference": (("▁a", "▁b"), ("▁a", "<unk>", "▁b")),
    "unk on both sides": (("▁a", "<unk>", "▁", "<unk>"), ("▁a", "<unk>", "▁", "<unk>")),
    "identical": (("▁ab", "c", "▁a", "."), ("▁ab", "c", "▁a", ".")),
    "nothing in common": (("▁a", "a"), ("▁b", "c")),
    "both empty": ((), ()),
}


def test_the_rules_corners():
    hyps, refs = [T(*h) for h, _ in CASES.values()], [T(*r) for _, r in CASES.values()]
    want = check(hyps, refs, elems=ELEMS)
    row = dict(zip(CASES, want.tolist()))
    assert row["clipping"][:3] == [4, 2, 2] and row["clipping back"][:3] == [2, 4, 2] and row["clipping"][3:6] == [3, 1, 1]
    assert row["(a)"][18:21] == [2, 3, 1] and row["(a) the other way"][18:21] == [2, 3, 1], "the last-character rule comes first"
    assert row["a."][18:] == [2, 2, 2, 1, 1, 1] and row[".a"][18:21] == [2, 2, 2] and row["a.b"][18:21] == [1, 3, 0] and row[".."][18:21] == [2, 2, 2]
    assert row["unk in the reference"][2] == 2 and row["unk on both sides"][:3] == [11, 15, 11], "the reference's unk is <<unk>>"
    assert row["both empty"] == [0] * 24 and row["only breaks"][:3] == [0, 1, 0]
    for co, wo in ((1, 0), (6, 1), (2, 2)):
        check(hyps, refs, co=co, wo=wo, what=(co, wo))
    out = check_scores(hyps, refs, 6, 2)
    s = dict(zip(CASES, out["sentence_chrf"].tolist()))
    assert s["identical"] == 100.0 and s["nothing in common"] == 0.0 and s["both empty"] == 0.0
    abc = scorer(char_order=6).score(torch.tensor([T("▁ab", "c")], device=DEV), torch.tensor([2], device=DEV),
                                     torch.tensor([T("▁ab", ".")], device=DEV), torch.tensor([2], device=DEV))
    assert float(abc["sentence_chrf"][0]) == pytest.approx(100 * (2 / 3 + 1 / 2 + 0) / 3, rel=REL)
    check_scores(hyps, refs, 6, 0, beta=1.0)
    check_scores(hyps, refs, 4, 1, beta=3.0)


def test_refusals_beside_ordinary_pairs():
    rng = np.random.default_rng(3)
    rows = [chars(rng, 9) for _ in range(6)]
    hyp, ref = padded(rows, 12, 8), padded(rows[::-1], 12, 4)
    hyp[1, 3], hyp[2, 5], ref[1, 0] = V, -1, V + 5                                  # tokens outside [0, V): inside the lengths
    hyp[4, 10] = V + 1                                                             # behind the length: never read
    hlen, rlen = [9, 9, 9, 13, 9, 9], [9, 9, 9, 9, -1, 9]
    hyp_row, ref_row = [0, 1, 2, 3, 4, 5, 0, 6, -1, 5, 4, 0], [5, 5, 5, 5, 5, 5, 1, 0, 0, 6, 4, -2]
    got, status = call_raw(hyp, hlen, ref, rlen, hyp_row, ref_row)
    want_status = [0, 2, 2, 2, 0, 0, 2, 2, 2, 2, 2, 2]
    want = want_of(rows, rows[::-1], hyp_row=[h if s == 0 else 0 for h, s in zip(hyp_row, want_status)],
                   ref_row=[r if s == 0 else 0 for r, s in zip(ref_row, want_status)])
    want[np.array(want_status) == 2] = 0
    assert differs(got, want, status, want_status) is None, differs(got, want, status, want_status)
    # a reference-side unk without a special rendering is an ordinary token
    u = call_raw(padded([T("▁a", "<unk>")], 2, 8), [2], padded([T("▁a", "<unk>")], 2, 8), [2], unk=-1)[0]
    assert u[0, :3].tolist() == [6, 6, 6]


def test_maps_and_one_matrix_as_both_sides():
    rng = np.random.default_rng(4)
    rows = [chars(rng, int(n)) for n in rng.integers(0, 40, size=7)]
    others = [chars(rng, int(n)) for n in rng.integers(0, 40, size=5)]
    hr, rr = [6, 0, 3, 3, 1, 2, 5, 4, 0], [4, 4, 0, 1, 2, 3, 3, 0, 1]
    check(rows, others, hyp_row=hr, ref_row=rr, elems=ELEMS, what="both maps")
    check(rows, others, hyp_row=None, ref_row=[4, 3, 2, 1, 0, 0, 2], elems=ELEMS, what="the reference's map")
    check(rows, others, hyp_row=[6, 5, 4, 3, 2], ref_row=None, elems=ELEMS, what="the hypothesis' map")
    check(rows, rows[::-1], elems=ELEMS, what="no map")
    for elem in (4, 8):                                                            # one matrix, its own memory, as both sides
        m, n = padded(rows, 41, elem), [len(r) for r in rows]
        pairs = [(i, j) for i in range(7) for j in range(7)]
        got, status = call_raw(m, n, m, n, [i for i, _ in pairs], [j for _, j in pairs], same=True)
        want = want_of(rows, rows, [i for i, _ in pairs], [j for _, j in pairs])
        assert differs(got, want, status, np.zeros(49)) is None
        got, status = call_raw(m, n, m, n, same=True)
        assert differs(got, want_of(rows, rows), status, np.zeros(7)) is None


def test_a_pair_alone_and_inside_a_batch():
    rng = np.random.default_rng(5)
    hyps = [chars(rng, int(n)) for n in rng.integers(0, 120, size=64)]
    refs = [chars(rng, int(n)) for n in rng.integers(0, 120, size=64)]
    Hmax, Rmax = max(len(h) for h in hyps), max(len(r) for r in refs)
    whole = call_raw(padded(hyps, Hmax, 8), [len(h) for h in hyps], padded(refs, Rmax, 8), [len(r) for r in refs])
    assert differs(whole[0], want_of(hyps, refs), whole[1], np.zeros(64)) is None
    for s in (0, 17, 63):
        one = call_raw(padded(hyps, Hmax, 8)[s:s + 1], [len(hyps[s])], padded(refs, Rmax, 8)[s:s + 1], [len(refs[s])])
        assert one[0].tobytes() == whole[0][s:s + 1].tobytes() and one[1][0] == whole[1][s]


def test_score_pairs_equals_score_on_repeated_rows_and_the_other_methods():
    rng = np.random.default_rng(6)
    rows = [chars(rng, int(n)) for n in rng.integers(1, 50, size=6)]
    refs = [chars(rng, int(n)) for n in rng.integers(1, 50, size=4)]
    hr, rr = [0, 1, 2, 3, 4, 5, 5, 0], [0, 0, 1, 1, 2, 3, 0, 3]
    t = lambda rows_, elem: (torch.from_numpy(padded(rows_, max(len(r) for r in rows_), elem)).to(DEV),
                             torch.tensor([len(r) for r in rows_], dtype=torch.int32 if elem == 4 else torch.int64, device=DEV))
    (h, hl), (r, rl) = t(rows, 8), t(refs, 4)
    a, b = scorer(word_order=2), scorer(word_order=2)
    pairs = a.score_pairs(h, hl, torch.tensor(hr, device=DEV), r, rl, torch.tensor(rr, dtype=torch.int32, device=DEV))
    (h2, hl2), (r2, rl2) = t([rows[i] for i in hr], 8), t([refs[j] for j in rr], 4)
    rep = b.score(h2, hl2, r2, rl2)
    assert torch.equal(pairs["stats"], rep["stats"]) and torch.equal(pairs["status"], rep["status"])
    assert torch.equal(pairs["sentence_chrf"], rep["sentence_chrf"]) and a.result() == b.result() and a.result()["char1_hyp"] > 0
    assert a.result_string().startswith("chrF2++ = ") and scorer().result_string() == "chrF2 = 0.00"
    # an n-best list through a row map, and the best hypothesis of every sentence
    hypos = [[{"tokens": torch.tensor(rows[i], device=DEV)} for i in idx] for idx in ([0, 1, 2], [], [3], [4, 5])]
    nb = scorer(word_order=2)
    out = nb.score_nbest(hypos, r, rl, accumulate="oracle")
    for bi, idx in enumerate(([0, 1, 2], [], [3], [4, 5])):
        for k, i in enumerate(idx):
            w = R.row_stats(D, rows[i], refs[bi], BPE, 6, 2)
            assert out["stats"][bi, k].tolist() == w and float(out["sentence_chrf"][bi, k]) == pytest.approx(R.score(w, 6, 2), rel=REL)
        best = max(range(len(idx)), key=lambda k: (float(out["sentence_chrf"][bi, k]), -k)) if idx else 0
        assert int(out["oracle"][bi]) == best and int(out["n_hyp"][bi]) == len(idx)
    top = scorer(word_order=2).score_hypotheses(hypos, r, rl)
    assert top["stats"].tolist() == [R.row_stats(D, rows[i] if i is not None else [], refs[bi], BPE, 6, 2) for bi, i in enumerate((0, None, 3, 4))]


# ---------------------------------------------------------------------------------------------- MBR with the chrF utility
def mbr_lists(seed, sizes):
    rng = np.random.default_rng(seed)
    lists = []
    for n in sizes:
        base = chars(rng, 30)
        rows = []
        for _ in range(n):
            row = list(base)
            for _ in range(int(rng.integers(0, 6))):
                row[int(rng.integers(0, len(row)))] = T("a", "b", "▁a", "▁b", ".", "c")[int(rng.integers(0, 6))]
            rows.append(row[:int(rng.integers(20, 31))] + [EOS])
        lists.append(rows)
    return lists


def check_rerank(out, lists, want, hypos):
    for b, (hs, gains) in enumerate(zip(out, want)):
        assert sorted(h["mbr_index"] for h in hs) == list(range(len(lists[b])))
        got = [float(h["mbr_score"]) for h in hs]
        assert got == sorted(got, reverse=True) and all(h is hypos[b][h["mbr_index"]] and h["mbr_score"].is_cuda for h in hs)
        for h in hs:
            assert float(h["mbr_score"]) == pytest.approx(gains[h["mbr_index"]], rel=REL, abs=0), (b, h["mbr_index"])
        order = sorted(range(len(gains)), key=lambda i: (-gains[i], i))
        near = any(0 < abs(gains[i] - gains[j]) <= REL * gains[i] for i in order for j in order)
        assert [h["mbr_index"] for h in hs] == order or near, (b, order)


def test_mbr_with_the_chrf_utility():
    from fbk_fairseq_st_amd import mbr as MB
    lists = mbr_lists(41, (1, 2, 3, 4, 0, 40))
    lists[3][2] = list(lists[3][0])                                                # a planted duplicate: an exact tie
    hypos = [[{"tokens": torch.tensor(t, device=DEV)} for t in ts] for ts in lists]
    for wo in (0, 2):
        want = [R.expected_chrf(D, ts, ts, BPE, word_order=wo) for ts in lists]
        dec = MB.MBRDecoder(None, PAD, EOS, UNK, utility=scorer(word_order=wo))
        check_rerank(dec.rerank(hypos), lists, want, hypos)
    # separate pseudo-references and weights
    pseudo = mbr_lists(42, (3, 3, 2, 5, 4, 7))
    w = [0.5, 2.0, 1.0, 0.0, 3.0, 1.5, 0.25]
    want = [R.expected_chrf(D, ts, ps, BPE, weights=w) for ts, ps in zip(lists, pseudo)]
    out = MB.MBRDecoder(None, PAD, EOS, UNK, utility=scorer()).rerank(hypos, pseudo=[[{"tokens": torch.tensor(t, device=DEV)} for t in ps]
                                                                                    for ps in pseudo], weights=w)
    check_rerank(out, lists, want, hypos)


def test_generate_through_the_task_on_the_device_search():
    """fixture case `c` through the device-resident sampling search, 8 samples per sentence, reordered by expected chrF++ of the
    dictionary's words (bpe None: every symbol is a word)"""
    import test_model_gpu as TM
    from fbk_fairseq_st_amd import chrf_scorer as CS
    from fbk_fairseq_st_amd import mbr as MB
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    task, model, src, lens, opts, exp, _ = TM.build_gen("c")
    d = task.target_dictionary
    sample = dict(net_input=dict(src_tokens=src, src_lengths=lens))
    opts = dict(opts, beam_size=8)
    mk = lambda: SequenceGenerator([model], d, search_strategy=Sampling(d, sampling_topk=10, seed=5), **opts)
    plain = mk().generate([model], sample)
    gen = mk()
    dec = MB.MBRDecoder.for_dictionary(gen, d, utility=CS.ChrfScorer.for_dictionary(d, bpe=None, word_order=2))
    out = task.inference_step(dec, [model], sample)
    assert "launches_per_step" in gen.last_stats, "the search did not take the device route"
    lists = [[h["tokens"].tolist() for h in hs] for hs in plain]
    want = [R.expected_chrf(d, ts, ts, None, word_order=2) for ts in lists]
    for b, (hs, gains) in enumerate(zip(out, want)):
        assert sorted(h["mbr_index"] for h in hs) == list(range(8)), "a permutation of the generator's list"
        for h in hs:
            assert h["tokens"].tolist() == lists[b][h["mbr_index"]] and h["mbr_score"].is_cuda and h["mbr_score"].dtype == torch.float64
            assert float(h["mbr_score"]) == pytest.approx(gains[h["mbr_index"]], rel=REL, abs=0), (b, h["mbr_index"])
        order = sorted(range(8), key=lambda i: (-gains[i], i))
        near = any(0 < abs(gains[i] - gains[j]) <= REL * gains[i] for i in order for j in order)
        assert [h["mbr_index"] for h in hs] == order or near, (b, order, gains)


# ---------------------------------------------------------------------------------------------- the comparisons can fail
def test_wrong_twins_fail_this_files_comparisons():
    hyps, refs = [T(*h) for h, _ in CASES.values()], [T(*r) for _, r in CASES.values()]
    got, status = call_raw(padded(hyps, 8, 8), [len(h) for h in hyps], padded(refs, 8, 8), [len(r) for r in refs])
    assert differs(got, want_of(hyps, refs), status, np.zeros(len(hyps))) is None
    for twin in ("keep_space", "no_clip", "first_rule_first"):
        assert differs(got, want_of(hyps, refs, twin=twin)) is not None, twin
    mine = [R.score(g.tolist(), 6, 2) for g in got]
    for twin in ("all_orders", "beta_other_side"):
        other = [R.score(g.tolist(), 6, 2, twin=twin) for g in got]
        assert any(abs(a - b) > REL * max(a, b) for a, b in zip(mine, other)), twin
    assert differs(got, got + (np.arange(24) == 5), status, status) is not None and differs(got, got, status, 2 - status) is not None


# ---------------------------------------------------------------------------------------------- the measured file
def test_measured_file_lies_within_the_bound():
    """tests/golden/chrf_measured.json: the worst relative score error of a run of this file on an MI355X (written by running the
    file as a script).  It sets no bound -- the bound is REL -- but it must lie within it."""
    with open(MEASURED) as f:
        m = json.load(f)
    assert m["bound"] == REL and 0 <= m["score_worst"] <= REL and m["scores"] > 0


if __name__ == "__main__":
    rc = pytest.main([os.path.abspath(__file__), "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"])
    W = sys.modules["test_chrf_gpu"].WORST                                # the module pytest imported holds the run's figures
    out = {"score_worst": W["score"], "scores": W["scores"], "bound": REL,
           "note": "worst relative error of ChrfScorer's sentence_chrf and result()['chrf'] against Python float64 (tests/chrf_ref.py) "
                   "over the score cases of tests/test_chrf_gpu.py on an MI355X; the tests hold every score to `bound`"}
    if len(sys.argv) > 1 and W["scores"]:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(int(rc))
