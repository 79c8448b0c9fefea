"""The chrF entry point and its Python layers without a GPU: s2t_chrf_stats is exported, bound and refuses bad arguments before
anything is launched; the constants are the same in the header, in kernels and in the class; kernels.chrf_stats and ChrfScorer
refuse what they should; `piece_table` rebuilds the text of `Dictionary.string` for every bpe mode; and the host logic of ChrfScorer
and of MBRDecoder(utility=...) with kernels.chrf_stats replaced by a stand-in kept in this file, which reads the piece table the
way the kernel does and counts with the Python reference (tests/chrf_ref.py; the kernel has its own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import chrf_ref as R
from fbk_fairseq_st_amd import chrf_scorer as CS
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd import mbr as MB
from fbk_fairseq_st_amd.data import Dictionary

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
ARGS = (("hyp", FAKE), ("hyp_len", FAKE), ("hyp_elem", 4), ("ref", FAKE), ("ref_len", FAKE), ("ref_elem", 8), ("hyp_row", None),
        ("ref_row", None), ("P", 2), ("Hmax", 7), ("Rmax", 5), ("Hrows", 2), ("Rrows", 2), ("pieces", FAKE), ("piece_off", FAKE),
        ("n_pieces", 40), ("V", 9), ("unk", 3), ("char_order", 6), ("word_order", 2), ("stats", FAKE), ("status", FAKE), ("stream", None))
D = R.make_dictionary()
PAD, EOS, UNK = D.pad(), D.eos(), D.unk()
T = lambda *s: R.tok(D, *s)


def test_export_binding_and_constants():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert "s2t_chrf_stats" in L.SIGNATURES and hasattr(raw, "s2t_chrf_stats") and hasattr(lib, "s2t_chrf_stats")
    assert len(L.SIGNATURES["s2t_chrf_stats"]) == 23 == len(ARGS) and "s2t_chrf_stats" not in L._SIZE_T_RESULT
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    for name, value in (("MAX_LEN", K.CHRF_MAX_LEN), ("MAX_CHARS", K.CHRF_MAX_CHARS), ("GROUP_LEN", K.CHRF_GROUP_LEN),
                        ("MAX_CHAR_ORDER", K.CHRF_MAX_CHAR_ORDER), ("MAX_WORD_ORDER", K.CHRF_MAX_WORD_ORDER)):
        assert "#define S2T_CHRF_%s %d\n" % (name, value) in text, name
    assert "#define S2T_CHRF_SEP 0x%xu\n" % K.CHRF_SEP in text
    assert (K.CHRF_MAX_LEN, K.CHRF_MAX_CHARS, K.CHRF_MAX_CHAR_ORDER, K.CHRF_MAX_WORD_ORDER, K.CHRF_STATS) == (1024, 4095, 6, 2, 24)
    assert (CS.MAX_LEN, CS.MAX_CHARS, CS.SEP) == (K.CHRF_MAX_LEN, K.CHRF_MAX_CHARS, K.CHRF_SEP) and len(CS._SUMS) == 24


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("hyp", "hyp_len", "ref", "ref_len", "pieces", "piece_off", "stats", "status"):
        assert f(**{name: None}) == -22, name                             # required pointers
    assert f(Hmax=-1) == -22 and f(Rmax=-1) == -22 and f(V=-1, unk=-1) == -22 and f(n_pieces=-1) == -22
    for name in ("hyp_elem", "ref_elem"):
        assert f(**{name: 2}) == -22 and f(**{name: 0}) == -22 and f(**{name: 16}) == -22, name
    assert f(Hrows=3) == -22 and f(Rrows=1) == -22, "a side without a map has one row per pair"
    assert f(Hrows=-1, hyp_row=FAKE) == -22 and f(Rrows=-1, ref_row=FAKE) == -22
    assert f(unk=9) == -22 and f(unk=100) == -22
    assert f(char_order=0) == -22 and f(char_order=7) == -22 and f(word_order=-1) == -22 and f(word_order=3) == -22
    assert f(Hmax=1025) == -95 and f(Rmax=1025) == -95 and f(Rmax=1025, Rrows=9, ref_row=FAKE) == -95
    assert f(P=0) == 0 and f(P=-3) == 0 and f(P=0, hyp=None, char_order=9, Hmax=10 ** 6) == 0     # an empty problem: nothing is looked at


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_chrf_stats)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_chrf_stats.argtypes = L.SIGNATURES["s2t_chrf_stats"]
    check_refusals(fast.s2t_chrf_stats)
    check_refusals(raw.s2t_chrf_stats)


def test_kernels_chrf_stats_checks_its_operands():
    t = CS.piece_table(D, "sentencepiece")
    pc, off = torch.from_numpy(t["pieces"].view(np.int32).copy()), torch.from_numpy(t["piece_off"].copy())
    h, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([5, 5], dtype=torch.int32)
    r, m = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    rows = torch.zeros(2, dtype=torch.int32)
    call = lambda *a, **kw: K.chrf_stats(*a, **dict(dict(pieces=pc, piece_off=off, unk=UNK), **kw))
    for bad in (lambda: call(h[0], n, r, m), lambda: call(h.float(), n, r, m), lambda: call(h, n.long(), r, m),
                lambda: call(h, n, r, m.int()), lambda: call(h, n[:1], r, m), lambda: call(h, n, r, m[:1]),
                lambda: call(h, n, r[:1], m[:1]), lambda: call(h, n, r, m, ref_row=rows.long()), lambda: call(h, n, r, m, hyp_row=rows.long()),
                lambda: call(h, n, r, m, hyp_row=rows, ref_row=rows[:1]), lambda: call(h, n, r, m, ref_row=torch.zeros(3, dtype=torch.int32)),
                lambda: call(h, n, r, m, hyp_row=rows[None]),
                lambda: call(h, n, r, m, char_order=0), lambda: call(h, n, r, m, char_order=7), lambda: call(h, n, r, m, word_order=3),
                lambda: call(h, n, r, m, word_order=-1), lambda: call(h, n, r, m, unk=len(D)),
                lambda: call(h, n, r, m, pieces=pc.float()), lambda: call(h, n, r, m, piece_off=off.long()), lambda: call(h, n, r, m, piece_off=off[:1]),
                lambda: call(h, n, r, m, pieces=pc[None]),
                lambda: call(torch.zeros(2, 1025, dtype=torch.int32), n, r, m),
                lambda: call(h, n, torch.zeros(2, 1025, dtype=torch.int64), m)):
        with pytest.raises(ValueError, match="chrf_stats"):
            bad()
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        call(torch.zeros(2, 1025, dtype=torch.int32), n, r, m)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_CHAR_ORDER"):
        call(h, n, r, m, char_order=7)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_WORD_ORDER"):
        call(h, n, r, m, word_order=3)
    stats, status = call(h[:0], n[:0], r[:0], m[:0])                           # no pairs: nothing is launched
    assert tuple(stats.shape) == (0, 24) and tuple(status.shape) == (0,) and stats.dtype == status.dtype == torch.int32
    stats, _ = call(h, n, r, m, hyp_row=rows[:0], ref_row=rows[:0])
    assert tuple(stats.shape) == (0, 24)


# ------------------------------------------------------------------ the piece table
def table_text(table, row, reference_side=False):
    """the text the kernel sees: the row's pieces in order, SEP as a space, whitespace folded; None for a token outside the table"""
    pieces, off, out = table["pieces"], table["piece_off"], []
    for t in row:
        t = int(t)
        if not 0 <= t < table["V"]:
            return None
        e = table["V"] if reference_side and t == table["unk"] else t
        out += [" " if c == CS.SEP else chr(c) for c in pieces[off[e]:off[e + 1]].tolist()]
    return " ".join("".join(out).split())


def bpe_dictionary():
    d = Dictionary()
    for s in ("he@@", "llo", "wor@@", "ld", "@@", "@@@", "a@@b", "x", "\U0001f600@@", "é", "▁", "@"):
        d.add_symbol(s)
    return d


@pytest.mark.parametrize("bpe", (None, "sentencepiece", "@@ "))
def test_piece_table_rebuilds_the_text_of_dictionary_string(bpe):
    d = D if bpe == "sentencepiece" else bpe_dictionary()
    table = CS.piece_table(d, bpe)
    assert table["pieces"].dtype == np.uint32 and table["piece_off"].dtype == np.int32 and table["piece_off"].shape == (len(d) + 2,)
    assert table["V"] == len(d) and table["unk"] == d.unk() and table["bpe"] == bpe
    off = table["piece_off"]
    for special in (d.pad(), d.eos(), d.bos()):
        assert off[special] == off[special + 1], "pad, eos and bos have empty pieces"
    rng = np.random.default_rng(0)
    rows = [rng.integers(0, len(d), size=int(n)).tolist() for n in rng.integers(0, 24, size=300)]     # specials and unk anywhere
    if bpe == "@@ ":
        i = d.indices
        rows += [[i["@@"]], [i["x"], i["@@"], i["x"]], [i["he@@"], i["llo"], i["wor@@"]], [i["x"], i["he@@"], d.eos()], [i["@@@"], i["x"]],
                 [i["a@@b"], i["\U0001f600@@"], i["é"]], [i["he@@"], d.pad(), i["llo"]], [d.unk(), i["he@@"], d.unk()]]
    for row in rows:
        for side in (False, True):
            assert table_text(table, row, side) == R.text_of(d, row, bpe, side), (row, side)
    if bpe == "@@ ":
        assert table_text(table, [i["he@@"], i["llo"], i["wor@@"]]) == "hello wor" and table_text(table, [i["x"], i["@@"], i["x"]]) == "x x"
        assert table_text(table, [d.unk()], True) == "<<unk>>" and table_text(table, [d.unk()]) == "<unk>"
    if bpe == "sentencepiece":
        assert table_text(table, T("b", "a▁b", "\U0001d4b3", "▁\U0001f600x", "é")) == "ba b\U0001d4b3 \U0001f600xé"
        e = d.indices["▁\U0001f600x"]
        assert table["pieces"][off[e]:off[e + 1]].tolist() == [CS.SEP, 0x1f600, ord("x")], "one code point, not two surrogates"


def test_piece_table_refuses_whitespace_and_other_bpe_values():
    for sym in ("a b", "a\tb", "a b", "　", "a\n"):
        d = Dictionary()
        d.add_symbol(sym)
        for bpe in (None, "sentencepiece", "@@ "):
            with pytest.raises(ValueError, match="whitespace"):
                CS.piece_table(d, bpe)
    for bpe in ("@@", "subword_nmt", "", " ", "@ @ ", 5):
        with pytest.raises(ValueError, match="bpe"):
            CS.piece_table(D, bpe)


# ------------------------------------------------------------------ host logic on a stand-in for the kernel call
@pytest.fixture
def calls(monkeypatch):
    c = []

    def chrf_stats(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk=-1, char_order=6, word_order=0, hyp_row=None, ref_row=None):
        assert hyp.dtype == hyp_len.dtype and ref.dtype == ref_len.dtype and hyp.dtype in (torch.int32, torch.int64)
        assert pieces.dtype == torch.int32 and piece_off.dtype == torch.int32
        for m in (hyp_row, ref_row):
            assert m is None or (m.dtype == torch.int32 and m.dim() == 1)
        table = {"pieces": pieces.numpy().view(np.uint32), "piece_off": piece_off.numpy(), "V": piece_off.shape[0] - 2, "unk": unk}
        P = hyp_row.shape[0] if hyp_row is not None else ref_row.shape[0] if ref_row is not None else hyp.shape[0]
        c.append((tuple(hyp.shape), tuple(ref.shape), (unk, char_order, word_order), None if hyp_row is None else hyp_row.tolist(),
                  None if ref_row is None else ref_row.tolist(), ref is hyp))
        stats, status = np.zeros((P, 24), np.int32), np.zeros((P,), np.int32)
        for p in range(P):
            hr, rr = (p if hyp_row is None else int(hyp_row[p])), (p if ref_row is None else int(ref_row[p]))
            ok = 0 <= hr < hyp.shape[0] and 0 <= rr < ref.shape[0] and 0 <= int(hyp_len[hr]) <= hyp.shape[1] and 0 <= int(ref_len[rr]) <= ref.shape[1]
            ht = table_text(table, hyp[hr, :int(hyp_len[hr])].tolist()) if ok else None
            rt = table_text(table, ref[rr, :int(ref_len[rr])].tolist(), True) if ok else None
            if ht is None or rt is None or len(ht.replace(" ", "")) > 4095 or len(rt.replace(" ", "")) > 4095:
                status[p] = 2
            else:
                stats[p] = R.pair_stats(ht, rt, char_order, word_order)
        return torch.from_numpy(stats), torch.from_numpy(status)
    monkeypatch.setattr(CS.K, "chrf_stats", chrf_stats)
    return c


HYP = [T("▁a", "b", "▁a", "."), T("▁b", "</s>", "<pad>"), [PAD] * 3, T("a▁b", "c", "▁c,", "</s>")]
REF = [T("▁ab", "▁a", "▁."), T("▁b", "b", "</s>"), T("▁a", "</s>"), T("▁a", "▁b", "c", "▁c,")]
KEYS = ["sentence_chrf", "stats", "status"]


def mat(rows, dtype=torch.int64):
    width = max(len(r) for r in rows)
    return torch.tensor([list(r) + [PAD] * (width - len(r)) for r in rows], dtype=dtype), torch.tensor([len(r) for r in rows], dtype=dtype)


def want_rows(hyp=HYP, ref=REF, co=6, wo=2):
    return [R.row_stats(D, h, r, "sentencepiece", co, wo) for h, r in zip(hyp, ref)]


def empty_result(orders):
    out = dict.fromkeys(CS._SUMS, 0)
    out.update(chrf=0.0, precisions=[0.0] * orders, recalls=[0.0] * orders, effective_order=0)
    return out


def test_score_fields_sums_and_result(calls):
    sc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    assert sc.result() == empty_result(8) and sc.result_string() == "chrF2++ = 0.00", "an empty accumulator: zeros, nothing divided"
    (h, hl), (r, rl) = mat(HYP), mat(REF, torch.int32)
    out = sc.score(h, hl, r, rl)
    assert sorted(out) == KEYS and calls == [((4, 4), (4, 4), (UNK, 6, 2), None, None, False)]
    want = want_rows()
    assert out["stats"].tolist() == want and out["stats"].dtype == torch.int32 and tuple(out["stats"].shape) == (4, 24)
    assert out["status"].tolist() == [0] * 4 and out["sentence_chrf"].dtype == torch.float64 and out["sentence_chrf"][2] == 0.0
    for s, w in enumerate(want):
        assert float(out["sentence_chrf"][s]) == pytest.approx(R.score(w, 6, 2), rel=1e-12, abs=0), s
    sums = np.array(want).sum(0).tolist()
    res = sc.result()
    assert [res[k] for k in CS._SUMS] == sums and all(isinstance(res[k], int) for k in CS._SUMS)
    assert res["chrf"] == pytest.approx(R.score(sums, 6, 2), rel=1e-14) and len(res["precisions"]) == 8
    assert res["effective_order"] == sum(1 for k in range(8) if sums[3 * k] > 0 and sums[3 * k + 1] > 0) >= 7
    assert res["precisions"][0] == sums[2] / sums[0] and res["recalls"][0] == sums[2] / sums[1] and res["recalls"][7] == sums[23] / sums[22]
    assert sc.result_string() == "chrF2++ = %.2f" % R.score(sums, 6, 2)
    sc.score(h[:2], hl[:2], r[:2], rl[:2])
    twice = (np.array(sums) + np.array(want[:2]).sum(0)).tolist()
    assert [sc.result()[k] for k in CS._SUMS] == twice, "calls add up"
    sc.reset()
    assert sc.result() == empty_result(8)
    # other orders and beta: fewer entries, another name
    one = CS.ChrfScorer.for_dictionary(D, char_order=2, beta=3.0)
    out = one.score(h, hl, r, rl)
    assert out["stats"].tolist() == want_rows(co=2, wo=0) and calls[-1][2] == (UNK, 2, 0) and len(one.result()["recalls"]) == 2
    assert one.result_string() == "chrF3 = %.2f" % R.score(np.array(want_rows(co=2, wo=0)).sum(0).tolist(), 2, 0, 3.0)
    assert CS.ChrfScorer.for_dictionary(D, beta=0.5).result_string() == "chrF0.5 = 0.00"
    short = CS.ChrfScorer.for_dictionary(D)
    short.score(*mat([T("▁a", "b")]), *mat([T("▁a", "b")]))
    assert short.result()["effective_order"] == 2 and short.result()["chrf"] == 100.0 and short.result()["precisions"] == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]


def test_sentence_chrf_on_stats():
    rows = want_rows() + [[0] * 24, R.pair_stats("abc", "abd", 6, 0), R.pair_stats("aa", "bc", 6, 2)]
    for co, wo, beta in ((6, 2, 2.0), (6, 0, 2.0), (1, 1, 1.0), (4, 0, 3.0)):
        cut = [[v if (k // 3 < co or 6 <= k // 3 < 6 + wo) else 0 for k, v in enumerate(r)] for r in rows]
        got = CS.sentence_chrf(torch.tensor(cut), co, wo, beta)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(rows),)
        for g, r in zip(got.tolist(), cut):
            assert g == pytest.approx(R.score(r, co, wo, beta), rel=1e-12, abs=0)
    assert float(CS.sentence_chrf(torch.tensor(R.pair_stats("abc", "abd", 6, 0)))) == pytest.approx(100 * (2 / 3 + 1 / 2) / 3, rel=1e-14)
    assert tuple(CS.sentence_chrf(torch.zeros(2, 3, 24, dtype=torch.int32)).shape) == (2, 3)


def test_refused_pairs_add_nothing(calls):
    sc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    h, _ = mat(HYP, torch.int32)
    r, _ = mat(REF)
    h[1, 0] = len(D)                                                         # a token outside the dictionary
    out = sc.score(h, torch.tensor([4, 3, 4, -1]), r, torch.tensor([3, 3, 9, 4]))
    assert out["status"].tolist() == [0, 2, 2, 2] and out["stats"][1:].eq(0).all() and out["sentence_chrf"][1:].eq(0).all()
    assert [sc.result()[k] for k in CS._SUMS] == want_rows()[0] and calls[0][0] == (4, 4)


def test_unk_on_either_side(calls):
    sc = CS.ChrfScorer.for_dictionary(D, word_order=1)
    one = sc.score(*mat([T("<unk>", "▁a")]), *mat([T("<unk>", "▁a")]))
    assert one["stats"][0, :3].tolist() == [6, 8, 6] and one["stats"][0, 18:21].tolist() == [3, 3, 2], "<unk> against <<unk>>"
    assert float(one["sentence_chrf"][0]) < 100.0


def test_score_hypotheses_takes_the_best(calls):
    t = lambda *s: torch.tensor(T(*s))
    hypos = [[{"tokens": t("▁a", "b", "</s>")}, {"tokens": t("▁ab", "▁a", "▁.", "</s>")}], [{"tokens": t("▁b", "</s>")}], [], [{"tokens": t("</s>")}]]
    sc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    r, rl = mat(REF)
    out = sc.score_hypotheses(hypos, r, rl)
    assert calls == [((4, 3), (4, 4), (UNK, 6, 2), None, None, False)] and sorted(out) == KEYS
    want = want_rows([T("▁a", "b"), T("▁b"), [], []])
    assert out["stats"].tolist() == want and [sc.result()[k] for k in CS._SUMS] == np.array(want).sum(0).tolist()
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 4 references"):
        sc.score_hypotheses(hypos[:3], r, rl)


def test_score_nbest_ragged_lists_and_both_accumulate_modes(calls):
    t = lambda *s: torch.tensor(T(*s))
    hypos = [[{"tokens": t("▁a", "b", "</s>")}, {"tokens": t("▁ab", "▁a", "▁.", "</s>")}, {"tokens": t("c", "</s>")}],   # the second is the reference
             [{"tokens": t("▁b", "</s>")}],
             [],
             [{"tokens": t("▁a", "▁b", "</s>")}, {"tokens": t("▁a", "▁b", "</s>")}]]                                     # a tie: the first wins
    r, rl = mat(REF)
    sc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    out = sc.score_nbest(hypos, r, rl)
    assert calls == [((6, 4), (4, 4), (UNK, 6, 2), None, [0, 0, 0, 1, 3, 3], False)]
    assert sorted(out) == sorted(KEYS + ["n_hyp", "oracle"]) and sc.result() == empty_result(8), "accumulate=None adds nothing"
    assert out["n_hyp"].tolist() == [3, 1, 0, 2] and out["oracle"].tolist() == [1, 0, 0, 0] and out["oracle"].dtype == torch.int64
    assert tuple(out["stats"].shape) == (4, 3, 24) and tuple(out["sentence_chrf"].shape) == (4, 3)
    for b, hs in enumerate(hypos):
        for k in range(3):
            if k < len(hs):
                w = R.row_stats(D, hs[k]["tokens"].tolist(), REF[b], "sentencepiece", 6, 2)
                assert out["stats"][b, k].tolist() == w and float(out["sentence_chrf"][b, k]) == pytest.approx(R.score(w, 6, 2), rel=1e-12, abs=0)
            else:
                assert out["stats"][b, k].eq(0).all() and out["sentence_chrf"][b, k] == -1.0 and out["status"][b, k] == 0
    assert float(out["sentence_chrf"][0, 1]) == 100.0
    pick = lambda idx: np.array([out["stats"][b, k].tolist() for b, k in enumerate(idx) if len(hypos[b])]).sum(0).tolist()
    best = CS.ChrfScorer.for_dictionary(D, word_order=2)
    best.score_nbest(hypos, r, rl, accumulate="best")
    assert [best.result()[k] for k in CS._SUMS] == pick([0, 0, 0, 0])
    orc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    orc.score_nbest(hypos, r, rl, accumulate="oracle")
    assert [orc.result()[k] for k in CS._SUMS] == pick([1, 0, 0, 0]) and orc.result()["chrf"] > best.result()["chrf"]
    orc.score_nbest(hypos, r, rl, accumulate="oracle")
    assert orc.result()["char1_match"] == 2 * pick([1, 0, 0, 0])[2], "calls add up"
    with pytest.raises(ValueError, match="accumulate"):
        sc.score_nbest(hypos, r, rl, accumulate="all")
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 4 references"):
        sc.score_nbest(hypos[:3], r, rl)
    nothing = sc.score_nbest([[], []], r[:2], rl[:2], accumulate="best")
    assert tuple(nothing["stats"].shape) == (2, 1, 24) and nothing["n_hyp"].tolist() == [0, 0] and nothing["sentence_chrf"].tolist() == [[-1.0], [-1.0]]
    assert sc.result() == empty_result(8)


def test_score_pairs_maps_and_one_matrix(calls):
    sc = CS.ChrfScorer.for_dictionary(D)
    h, hl = mat(HYP)
    r, rl = mat(REF)
    hr, rr = [3, 0, 0, 1], [0, 0, 3, 9]
    out = sc.score_pairs(h, hl, torch.tensor(hr), r, rl, torch.tensor(rr))
    assert calls[-1][3:] == (hr, rr, False) and out["status"].tolist() == [0, 0, 0, 2]
    assert out["stats"][:3].tolist() == [R.row_stats(D, HYP[i], REF[j], "sentencepiece", 6, 0) for i, j in zip(hr[:3], rr[:3])]
    own = sc.score_pairs(h, hl, torch.tensor([0, 1]), h, hl, torch.tensor([0, 0]))
    assert calls[-1][5] is True and own["sentence_chrf"][0] == 100.0, "one matrix as both sides stays one matrix"
    only_ref = sc.score_pairs(h, hl, None, r, rl, torch.tensor([0, 0, 0, 0]))
    assert calls[-1][3] is None and only_ref["stats"][0].tolist() == R.row_stats(D, HYP[0], REF[0], "sentencepiece", 6, 0)


def test_value_errors_of_the_class(calls):
    table = CS.piece_table(D, "sentencepiece")
    for kw in (dict(char_order=0), dict(char_order=7), dict(word_order=-1), dict(word_order=3), dict(beta=0.0), dict(beta=-1.0)):
        with pytest.raises(ValueError, match="ChrfScorer"):
            CS.ChrfScorer(table, **kw)
    for bad in (dict(table, pieces=table["pieces"].astype(np.int64)), dict(table, piece_off=table["piece_off"][:-1]), dict(table, unk=len(D)),
                dict(table, piece_off=table["piece_off"][::-1].copy()), dict(table, pieces=table["pieces"][:-1])):
        with pytest.raises(ValueError, match="ChrfScorer"):
            CS.ChrfScorer(bad)
    sc = CS.ChrfScorer(table)
    ok, n1 = torch.zeros(1, 3).long(), torch.tensor([3])
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        sc.score(torch.zeros(1, 1025).long(), n1, ok, n1)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        sc.score_pairs(ok, n1, None, torch.zeros(1, 1025).long(), n1, None)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        sc.score_hypotheses([[{"tokens": torch.zeros(1025).long()}]], ok, n1)
    with pytest.raises(ValueError, match="one B"):
        sc.score(ok, n1, torch.zeros(2, 3).long(), torch.tensor([3, 3]))
    with pytest.raises(ValueError, match="matrices"):
        sc.score_pairs(ok[0], n1, None, ok, n1, None)
    assert calls == [] and sc.result() == empty_result(6), "nothing was scored"


# ------------------------------------------------------------------ MBRDecoder(utility=...)
def hyp_lists(lists):
    return [[{"tokens": torch.tensor(t), "score": torch.tensor(-0.5 * k)} for k, t in enumerate(ts)] for ts in lists]


LISTS = [[T("▁a", "b", "▁a", "</s>"), T("▁a", "b", "▁b", "</s>"), T("▁a", "b", "▁a", "</s>"), T("▁b", "c", "</s>")],
         [],
         [T("▁c,", "</s>")],
         [T("▁a", "▁b", "</s>"), T("▁ab", "</s>"), T("▁a", "▁b", "▁.", "</s>")]]


def check_order(out, want, hypos):
    for b, (hs, gains) in enumerate(zip(out, want)):
        assert [h["mbr_index"] for h in hs] == sorted(range(len(gains)), key=lambda i: (-gains[i], i)), (b, gains)
        assert all(h is hypos[b][h["mbr_index"]] for h in hs)
        for h in hs:
            assert h["mbr_score"].dtype == torch.float64 and float(h["mbr_score"]) == pytest.approx(gains[h["mbr_index"]], rel=1e-12, abs=0)


def test_mbr_with_a_chrf_utility(calls, monkeypatch):
    monkeypatch.setattr(MB.K, "bleu_pairs", lambda *a, **kw: pytest.fail("the BLEU route was taken"))
    sc = CS.ChrfScorer.for_dictionary(D, word_order=2)
    dec = MB.MBRDecoder(None, PAD, EOS, UNK, utility=sc)
    hypos = hyp_lists(LISTS)
    out = dec.rerank(hypos)
    want = [R.expected_chrf(D, ts, ts, "sentencepiece", word_order=2) for ts in LISTS]
    check_order(out, want, hypos)
    assert [h["mbr_index"] for h in out[0]] == [0, 2, 1, 3], "the two equal hypotheses tie and keep their order"
    assert len(calls) == 1 and calls[0][5] is True, "one call, one matrix as both sides"
    assert calls[0][3] == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] + [5] * 3 + [6] * 3 + [7] * 3
    assert calls[0][4] == [0, 1, 2, 3] * 4 + [4] + [5, 6, 7] * 3, "candidate row and pseudo-reference row of every pair of a sentence"
    assert sc.result()["char1_hyp"] > 0, "the pairs went through score_pairs"
    # separate pseudo-references, and the weights
    pseudo = [[T("▁a", "b", "</s>"), T("▁b", "</s>")], [T("▁a", "</s>")], [], [T("▁ab", "</s>"), T("▁a", "▁b", "</s>"), T("c", "</s>")]]
    out = dec.rerank(hypos, pseudo=hyp_lists(pseudo))
    want = [R.expected_chrf(D, ts, ps, "sentencepiece", word_order=2) for ts, ps in zip(LISTS, pseudo)]
    check_order(out, want, hypos)
    assert calls[-1][5] is False and [float(h["mbr_score"]) for h in out[2]] == [0.0], "against an empty list the score is 0"
    w = [3.0, 0.0, 1.0]
    check_order(dec.rerank(hypos, pseudo=hyp_lists(pseudo), weights=w), [R.expected_chrf(D, ts, ps, "sentencepiece", w, word_order=2)
                                                                         for ts, ps in zip(LISTS, pseudo)], hypos)
    by_score = [[float(np.exp(-0.5 * k)) for k in range(len(ps))] for ps in pseudo]
    want = [R.expected_chrf(D, ts, ps, "sentencepiece", ws, word_order=2) for ts, ps, ws in zip(LISTS, pseudo, by_score)]
    check_order(MB.MBRDecoder(None, PAD, EOS, UNK, weights="score", utility=sc).rerank(hypos, pseudo=hyp_lists(pseudo)), want, hypos)
    assert MB.MBRDecoder(None, PAD, EOS, UNK, utility=sc).rerank([[], []]) == [[], []]
    assert MB.MBRDecoder.for_dictionary(None, D, utility=sc).utility is sc and MB.MBRDecoder.for_dictionary(None, D).utility is None


def test_the_cut_by_sentences_counts_this_kernels_bytes():
    assert MB._CHRF_PAIR_BYTES == 4 * 24 + 4 + 8 + 8
    nc = nr = [3000] * 4
    assert MB.MBRDecoder.chunk_sentences(nc, nr) == [(0, 2), (2, 4)] and MB.MBRDecoder.chunk_sentences(nc, nr, 44) == [(0, 2), (2, 4)]
    assert MB.MBRDecoder.chunk_sentences(nc, nr, MB._CHRF_PAIR_BYTES) == [(0, 1), (1, 2), (2, 3), (3, 4)]


def test_utility_none_still_calls_bleu_pairs(calls, monkeypatch):
    seen = []

    def bleu_pairs(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, max_list=None):
        seen.append((tuple(cand.shape), max_list))
        return torch.zeros((cand.shape[0], max_list, 10), dtype=torch.int32), torch.zeros((cand.shape[0], max_list), dtype=torch.int32)
    monkeypatch.setattr(MB.K, "bleu_pairs", bleu_pairs)
    out = MB.MBRDecoder(None, PAD, EOS, UNK).rerank(hyp_lists(LISTS))
    assert seen == [((8, 4), 4)] and calls == [] and [len(hs) for hs in out] == [4, 0, 1, 3]
