"""The unit entry point and its Python layers without a GPU: s2t_text_units is exported, bound and refuses bad arguments before
anything is launched; the constants are the same in the header, in kernels and in the class; kernels.text_units and TextErrorRate
refuse what they should; `unit_width` bounds the units of every row; and the host logic of TextErrorRate and of
MBRDecoder(utility=TextErrorRate) with kernels.text_units and kernels.edit_align replaced by stand-ins kept in this file, which read
the piece table the way the kernel does and count with the Python references (tests/text_error_ref.py, tests/edit_ref.py; the
kernels have their own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edit_ref as E
import text_error_ref as R
from fbk_fairseq_st_amd import chrf_scorer as CS
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd import mbr as MB
from fbk_fairseq_st_amd import text_error_rate as TE

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
ARGS = (("hyp", FAKE), ("hyp_len", FAKE), ("hyp_elem", 4), ("ref", FAKE), ("ref_len", FAKE), ("ref_elem", 8), ("hyp_row", None),
        ("ref_row", None), ("P", 2), ("Hmax", 7), ("Rmax", 5), ("Hrows", 2), ("Rrows", 2), ("pieces", FAKE), ("piece_off", FAKE),
        ("n_pieces", 40), ("V", 9), ("unk", 3), ("mode", 0), ("Uh", 15), ("Ur", 11), ("hyp_units", FAKE), ("ref_units", FAKE),
        ("hyp_n", FAKE), ("ref_n", FAKE), ("status", FAKE), ("stream", None))
D = R.make_dictionary()
PAD, EOS, UNK = D.pad(), D.eos(), D.unk()
T = lambda *s: [D.indices[x] for x in s]
TABLE = CS.piece_table(D, "sentencepiece")


def test_export_binding_and_constants():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert "s2t_text_units" in L.SIGNATURES and hasattr(raw, "s2t_text_units") and hasattr(lib, "s2t_text_units")
    assert len(L.SIGNATURES["s2t_text_units"]) == 27 == len(ARGS) and "s2t_text_units" not in L._SIZE_T_RESULT
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    assert "#define S2T_TEXT_MAX_UNITS %d\n" % K.TEXT_MAX_UNITS in text
    assert K.TEXT_MAX_UNITS == 4095 == K.EDIT_MAX_B == K.CHRF_MAX_CHARS, "whatever the unit kernel writes, the alignment takes"
    assert K.TEXT_MODES == {"word": 0, "char": 1, "char_nospace": 2} and TE.UNITS == ("word", "char", "char_nospace")
    assert (TE.MAX_LEN, TE.MAX_UNITS) == (K.CHRF_MAX_LEN, K.TEXT_MAX_UNITS) and TE.OPS is not None
    assert TE.TextErrorRate.utility_key == "sentence_accuracy"


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("hyp", "hyp_len", "ref", "ref_len", "pieces", "piece_off", "hyp_units", "ref_units", "hyp_n", "ref_n", "status"):
        assert f(**{name: None}) == -22, name                             # required pointers
    assert f(Hmax=-1) == -22 and f(Rmax=-1) == -22 and f(V=-1, unk=-1) == -22 and f(n_pieces=-1) == -22
    for name in ("hyp_elem", "ref_elem"):
        assert f(**{name: 2}) == -22 and f(**{name: 0}) == -22 and f(**{name: 16}) == -22, name
    assert f(Hrows=3) == -22 and f(Rrows=1) == -22, "a side without a map has one row per pair"
    assert f(Hrows=-1, hyp_row=FAKE) == -22 and f(Rrows=-1, ref_row=FAKE) == -22
    assert f(unk=9) == -22 and f(unk=100) == -22
    assert f(mode=-1) == -22 and f(mode=3) == -22
    for name in ("Uh", "Ur"):
        assert f(**{name: -1}) == -22 and f(**{name: 4096}) == -22, name
    assert f(Hmax=1025) == -95 and f(Rmax=1025) == -95 and f(Rmax=1025, Rrows=9, ref_row=FAKE) == -95
    assert f(P=0) == 0 and f(P=-3) == 0 and f(P=0, hyp=None, mode=9, Hmax=10 ** 6, Uh=-5) == 0     # an empty problem: nothing is looked at


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_text_units)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_text_units.argtypes = L.SIGNATURES["s2t_text_units"]
    check_refusals(fast.s2t_text_units)
    check_refusals(raw.s2t_text_units)


def test_kernels_text_units_checks_its_operands():
    pc, off = torch.from_numpy(TABLE["pieces"].view(np.int32).copy()), torch.from_numpy(TABLE["piece_off"].copy())
    h, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([5, 5], dtype=torch.int32)
    r, m = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    rows = torch.zeros(2, dtype=torch.int32)
    base = dict(pieces=pc, piece_off=off, unk=UNK, mode=0, hyp_width=8, ref_width=8)
    call = lambda *a, **kw: K.text_units(*a, **dict(base, **kw))
    for bad in (lambda: call(h[0], n, r, m), lambda: call(h.float(), n, r, m), lambda: call(h, n.long(), r, m),
                lambda: call(h, n, r, m.int()), lambda: call(h, n[:1], r, m), lambda: call(h, n, r, m[:1]),
                lambda: call(h, n, r[:1], m[:1]), lambda: call(h, n, r, m, ref_row=rows.long()), lambda: call(h, n, r, m, hyp_row=rows.long()),
                lambda: call(h, n, r, m, hyp_row=rows, ref_row=rows[:1]), lambda: call(h, n, r, m, ref_row=torch.zeros(3, dtype=torch.int32)),
                lambda: call(h, n, r, m, hyp_row=rows[None]),
                lambda: call(h, n, r, m, mode=3), lambda: call(h, n, r, m, mode=-1),
                lambda: call(h, n, r, m, hyp_width=-1), lambda: call(h, n, r, m, hyp_width=4096), lambda: call(h, n, r, m, ref_width=4096),
                lambda: call(h, n, r, m, unk=len(D)),
                lambda: call(h, n, r, m, pieces=pc.float()), lambda: call(h, n, r, m, piece_off=off.long()), lambda: call(h, n, r, m, piece_off=off[:1]),
                lambda: call(h, n, r, m, pieces=pc[None]),
                lambda: call(torch.zeros(2, 1025, dtype=torch.int32), n, r, m),
                lambda: call(h, n, torch.zeros(2, 1025, dtype=torch.int64), m)):
        with pytest.raises(ValueError, match="text_units"):
            bad()
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        call(torch.zeros(2, 1025, dtype=torch.int32), n, r, m)
    with pytest.raises(ValueError, match="S2T_TEXT_MAX_UNITS"):
        call(h, n, r, m, ref_width=4096)
    hu, hn, ru, rn, status = call(h[:0], n[:0], r[:0], m[:0])                    # no pairs: nothing is launched
    assert tuple(hu.shape) == (0, 8) and tuple(ru.shape) == (0, 8) and tuple(hn.shape) == tuple(rn.shape) == tuple(status.shape) == (0,)
    assert hu.dtype == ru.dtype == hn.dtype == rn.dtype == status.dtype == torch.int32
    hu, _, _, _, _ = call(h, n, r, m, hyp_row=rows[:0], ref_row=rows[:0])
    assert tuple(hu.shape) == (0, 8)


# ------------------------------------------------------------------ unit widths
def n_units(text, unit):
    return len(R.unit_rows(text, "", unit)[0])


def test_unit_width_bounds_every_row():
    t = CS.DeviceTable(TABLE, "test")
    assert (t.max_chars, t.max_breaks, t.max_spaced) == (8, 2, 8), "abcdefgh; a piece with two breaks; <<unk>> has 7"
    rng = np.random.default_rng(2)
    for unit in TE.UNITS:
        te = TE.TextErrorRate(TABLE, unit)
        assert te.unit_width(0) == (1 if unit == "word" else 0) and te.unit_width(10, "ref") == te.unit_width(10, "hyp")
        assert te.unit_width(10) == {"word": 21, "char": 80, "char_nospace": 80}[unit]
        assert te.unit_width(1024) == 4095 if unit != "word" else te.unit_width(1024) == 2049, "clipped to S2T_TEXT_MAX_UNITS"
        assert TE.TextErrorRate(TABLE, unit, max_units=7).unit_width(10) == 7 and TE.TextErrorRate(TABLE, unit, max_units=0).unit_width(3) == 0
        for _ in range(300):
            row = rng.integers(0, len(D), size=int(rng.integers(0, 12))).tolist()
            for side in (False, True):
                assert n_units(R.C.text_of(D, row, R.BPE, side), unit) <= te.unit_width(len(row), "ref" if side else "hyp"), (unit, row)
        worst = {"word": T("a▁b▁c") * 5, "char": T("abcdefgh") * 5, "char_nospace": T("abcdefgh") * 5}[unit]
        assert n_units(R.C.text_of(D, worst, R.BPE), unit) >= te.unit_width(5) - 1, "the bound is reached"
    with pytest.raises(ValueError, match="side"):
        TE.TextErrorRate(TABLE).unit_width(3, "both")
    te = TE.TextErrorRate(TABLE, "char")
    assert te.pair_bytes(10, 5) == 4 * (80 + 40) + 64 and TE.TextErrorRate(TABLE, "word").pair_bytes(10, 5) == 4 * (21 + 11) + 64


# ------------------------------------------------------------------ host logic on stand-ins for the two kernel calls
@pytest.fixture
def calls(monkeypatch):
    c = []

    def text_units(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk, mode, hyp_width, ref_width, hyp_row=None, ref_row=None):
        assert hyp.dtype == hyp_len.dtype and ref.dtype == ref_len.dtype and hyp.dtype in (torch.int32, torch.int64)
        assert pieces.dtype == torch.int32 and piece_off.dtype == torch.int32
        for m in (hyp_row, ref_row):
            assert m is None or (m.dtype == torch.int32 and m.dim() == 1)
        table = {"pieces": pieces.numpy().view(np.uint32), "piece_off": piece_off.numpy(), "V": piece_off.shape[0] - 2, "unk": unk}
        P = hyp_row.shape[0] if hyp_row is not None else ref_row.shape[0] if ref_row is not None else hyp.shape[0]
        c.append(("units", tuple(hyp.shape), tuple(ref.shape), (unk, mode, hyp_width, ref_width), None if hyp_row is None else hyp_row.tolist(),
                  None if ref_row is None else ref_row.tolist(), ref is hyp))
        hu, ru = np.full((P, hyp_width), -9, np.int32), np.full((P, ref_width), -9, np.int32)       # behind the lengths: not written
        hn, rn, status = np.zeros((P,), np.int32), np.zeros((P,), np.int32), np.zeros((P,), np.int32)
        for p in range(P):
            hr, rr = (p if hyp_row is None else int(hyp_row[p])), (p if ref_row is None else int(ref_row[p]))
            ok = 0 <= hr < hyp.shape[0] and 0 <= rr < ref.shape[0] and 0 <= int(hyp_len[hr]) <= hyp.shape[1] and 0 <= int(ref_len[rr]) <= ref.shape[1]
            ht = R.table_text(table, hyp[hr, :int(hyp_len[hr])].tolist()) if ok else None
            rt = R.table_text(table, ref[rr, :int(ref_len[rr])].tolist(), True) if ok else None
            if ht is None or rt is None or len(ht.replace(" ", "")) > 4095 or len(rt.replace(" ", "")) > 4095:
                status[p] = 2
                continue
            a, b = R.unit_rows(ht, rt, TE.UNITS[mode])
            if len(a) > hyp_width or len(b) > ref_width:
                status[p] = 2
                continue
            hu[p, :len(a)], ru[p, :len(b)], hn[p], rn[p] = a, b, len(a), len(b)
        return tuple(torch.from_numpy(x) for x in (hu, hn, ru, rn, status))

    def edit_align(a, a_len, b, b_len, costs=(1, 1, 1), collapse_blank=None, want_ops=False):
        assert a.dtype == a_len.dtype == b.dtype == b_len.dtype == torch.int32 and tuple(costs) == (1, 1, 1) and collapse_blank is None
        c.append(("align", tuple(a.shape), tuple(b.shape), want_ops))
        out = E.edit_align_batch(a.numpy(), a_len.numpy(), b.numpy(), b_len.numpy(), costs, None, want_ops)
        return tuple(None if x is None else torch.from_numpy(x) for x in out)
    monkeypatch.setattr(TE.K, "text_units", text_units)
    monkeypatch.setattr(TE.K, "edit_align", edit_align)
    return c


HYP = [T("▁a", "b", "▁a", "."), T("▁b", "</s>", "<pad>"), [PAD] * 3, T("a▁b", "c", "▁c,", "</s>"), T("▁a", "▁b", "▁c")]
REF = [T("▁ab", "▁a", "▁."), T("▁b", "b", "</s>"), T("▁a", "</s>"), T("▁a", "▁b", "c", "▁c,"), T("▁a", "▁x", "▁c", "d", "▁b")]
INTS = ["substitutions", "insertions", "deletions", "matches", "errors", "hyp_units_n", "ref_units_n"]
KEYS = sorted(INTS + ["status", "sentence_rate", "sentence_accuracy"])


def mat(rows, dtype=torch.int64):
    width = max(len(r) for r in rows)
    return torch.tensor([list(r) + [PAD] * (width - len(r)) for r in rows], dtype=dtype), torch.tensor([len(r) for r in rows], dtype=dtype)


def want_pairs(unit, hyp=HYP, ref=REF):
    return [R.pair(D, h, r, unit) for h, r in zip(hyp, ref)]


def check_pairs(out, want, where=None):
    for s, w in enumerate(want):
        at = s if where is None else where[s]
        assert [int(out[k][at]) for k in INTS] == [w[k] for k in INTS], (s, w)
        assert float(out["sentence_rate"][at]) == pytest.approx(w["rate"], rel=1e-12, abs=0)
        assert float(out["sentence_accuracy"][at]) == pytest.approx(w["accuracy"], rel=1e-12, abs=0)


def sums_of(te):
    return {k: te.result()[k] for k in TE._SUMS}


EMPTY = dict(errors=0, substitutions=0, insertions=0, deletions=0, ref_units=0, hyp_units=0, pairs=0, rate=0.0, accuracy=100.0)


@pytest.mark.parametrize("unit", TE.UNITS)
def test_score_fields_sums_and_result(calls, unit):
    te = TE.TextErrorRate.for_dictionary(D, unit=unit)
    name = "WER" if unit == "word" else "CER"
    assert te.result() == EMPTY and te.result_string() == "%s = 0.00 (S 0, D 0, I 0, N 0)" % name, "an empty accumulator: nothing divided"
    (h, hl), (r, rl) = mat(HYP), mat(REF, torch.int32)
    out = te.score(h, hl, r, rl)
    assert sorted(out) == KEYS
    Uh, Ur = te.unit_width(4), te.unit_width(5)
    assert calls == [("units", (5, 4), (5, 5), (UNK, K.TEXT_MODES[unit], Uh, Ur), None, None, False), ("align", (5, Uh), (5, Ur), False)], "two calls"
    want = want_pairs(unit)
    check_pairs(out, want)
    assert out["status"].tolist() == [0] * 5 and out["sentence_rate"].dtype == out["sentence_accuracy"].dtype == torch.float64
    assert all(out[k].dtype == torch.int32 for k in INTS)
    res = te.result()
    assert res == R.corpus(want) and all(isinstance(res[k], int) for k in TE._SUMS)
    assert te.result_string() == "%s = %.2f (S %d, D %d, I %d, N %d)" % (name, res["rate"], res["substitutions"], res["deletions"],
                                                                         res["insertions"], res["ref_units"])
    te.score(h[:2], hl[:2], r[:2], rl[:2])
    assert te.result() == R.corpus(want + want[:2]), "calls add up"
    te.reset()
    assert te.result() == EMPTY


def test_the_hand_cases_through_the_class(calls):
    te = TE.TextErrorRate.for_dictionary(D)
    hyp = [T("▁a", "▁b", "▁c"), T("▁ab", "c"), [], T("▁a", "▁b")]
    ref = [T("▁a", "▁x", "▁c", "▁", "b▁"), T("▁ab", "c"), T("▁a", "▁b"), []]
    (h, hl), (r, rl) = mat(hyp), mat(ref)
    out = te.score(h, hl, r, rl)
    assert out["substitutions"].tolist() == [1, 0, 0, 0] and out["deletions"].tolist() == [1, 0, 2, 0] and out["insertions"].tolist() == [0, 0, 0, 2]
    assert out["ref_units_n"].tolist() == [4, 1, 2, 0] and out["sentence_rate"].tolist() == [50.0, 0.0, 100.0, 200.0]
    assert out["sentence_accuracy"].tolist() == [50.0, 100.0, 0.0, 0.0]
    assert te.result_string() == "WER = 85.71 (S 1, D 3, I 2, N 7)"
    assert TE.TextErrorRate.for_dictionary(D, unit="char").result_string().startswith("CER = ")


def test_refused_pairs_add_nothing(calls):
    te = TE.TextErrorRate.for_dictionary(D)
    h, _ = mat(HYP, torch.int32)
    r, _ = mat(REF)
    h[1, 0] = len(D)                                                         # a token outside the dictionary
    out = te.score(h, torch.tensor([4, 3, 4, -1, 3]), r, torch.tensor([3, 3, 9, 4, 5]))
    assert out["status"].tolist() == [0, 2, 2, 2, 0]
    for k in INTS + ["sentence_rate", "sentence_accuracy"]:
        assert out[k][1:4].eq(0).all(), k
    assert te.result() == R.corpus([want_pairs("word")[0], want_pairs("word")[4]])
    # a side with more units than max_units allows is the unit call's refusal
    small = TE.TextErrorRate.for_dictionary(D, max_units=2)
    (h, hl), (r, rl) = mat(HYP), mat(REF)
    out = small.score(h, hl, r, rl)
    assert out["status"].tolist() == [2, 0, 0, 2, 2] and calls[-2][3][2:] == (2, 2) and small.result()["pairs"] == 2


def test_unk_on_either_side(calls):
    te = TE.TextErrorRate.for_dictionary(D)
    out = te.score(*mat([T("▁a", "▁", "<unk>"), T("▁a", "<unk>", "▁b")]), *mat([T("▁a", "▁", "<unk>"), T("▁a", "▁b", "▁b")]))
    assert out["substitutions"].tolist() == [1, 1] and out["matches"].tolist() == [1, 1] and out["deletions"].tolist() == [0, 1]
    c = TE.TextErrorRate.for_dictionary(D, unit="char_nospace").score(*mat([T("<unk>")]), *mat([T("<unk>")]))
    assert (int(c["hyp_units_n"][0]), int(c["ref_units_n"][0]), int(c["deletions"][0]), int(c["matches"][0])) == (5, 7, 2, 5), "<unk> against <<unk>>"


def test_score_hypotheses_takes_the_best(calls):
    t = lambda *s: torch.tensor(T(*s))
    hypos = [[{"tokens": t("▁a", "b", "</s>")}, {"tokens": t("▁ab", "▁a", "▁.", "</s>")}], [{"tokens": t("▁b", "</s>")}], [], [{"tokens": t("</s>")}],
             [{"tokens": t("▁a", "▁x")}]]
    te = TE.TextErrorRate.for_dictionary(D)
    r, rl = mat(REF)
    out = te.score_hypotheses(hypos, r, rl)
    assert calls[0][1:3] == ((5, 3), (5, 5)) and sorted(out) == KEYS
    want = want_pairs("word", [T("▁a", "b"), T("▁b"), [], [], T("▁a", "▁x")])
    check_pairs(out, want)
    assert te.result() == R.corpus(want)
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 5 references"):
        te.score_hypotheses(hypos[:3], r, rl)


def test_score_nbest_ragged_lists_both_accumulate_modes_and_the_lowest_rate(calls):
    t = lambda *s: torch.tensor(T(*s))
    hypos = [[{"tokens": t("▁a", "b", "</s>")}, {"tokens": t("▁ab", "▁a", "▁.", "</s>")}, {"tokens": t("c", "</s>")}],   # the second is the reference
             [{"tokens": t("▁b", "</s>")}],
             [],
             [{"tokens": t("▁a", "▁b", "</s>")}, {"tokens": t("▁a", "▁b", "</s>")}],                                     # a tie: the first wins
             [{"tokens": torch.tensor([len(D)])}, {"tokens": t("▁a", "▁c")}, {"tokens": t("▁a", "▁x", "▁c", "d")}]]      # a refused one is no oracle
    r, rl = mat(REF)
    te = TE.TextErrorRate.for_dictionary(D)
    out = te.score_nbest(hypos, r, rl)
    assert calls[0][1:3] == ((9, 4), (5, 5)) and calls[0][4:] == (None, [0, 0, 0, 1, 3, 3, 4, 4, 4], False) and len(calls) == 2
    assert sorted(out) == sorted(KEYS + ["n_hyp", "oracle"]) and te.result() == EMPTY, "accumulate=None adds nothing"
    assert out["n_hyp"].tolist() == [3, 1, 0, 2, 3] and out["oracle"].tolist() == [1, 0, 0, 0, 2] and out["oracle"].dtype == torch.int64
    assert tuple(out["errors"].shape) == (5, 3) and tuple(out["sentence_rate"].shape) == (5, 3) and out["status"][4].tolist() == [2, 0, 0]
    real = []
    for b, hs in enumerate(hypos):
        for k in range(3):
            if k < len(hs) and (b, k) != (4, 0):
                w = R.pair(D, hs[k]["tokens"].tolist(), REF[b], "word")
                check_pairs(out, [w], [(b, k)])
                real.append((b, k, w))
            else:
                assert all(int(out[key][b, k]) == 0 for key in INTS) and out["sentence_accuracy"][b, k] == 0.0
                assert out["sentence_rate"][b, k] == (0.0 if (b, k) == (4, 0) else -1.0)
    assert float(out["sentence_rate"][0, 1]) == 0.0 and float(out["sentence_rate"][4, 2]) < float(out["sentence_rate"][4, 1])
    pick = lambda idx: R.corpus([w for b, k, w in real if k == idx[b]])
    best = TE.TextErrorRate.for_dictionary(D)
    best.score_nbest(hypos, r, rl, accumulate="best")
    assert best.result() == pick([0, 0, 0, 0, 0]) and best.result()["pairs"] == 3
    orc = TE.TextErrorRate.for_dictionary(D)
    orc.score_nbest(hypos, r, rl, accumulate="oracle")
    assert orc.result() == pick([1, 0, 0, 0, 2]) and orc.result()["rate"] < best.result()["rate"] and orc.result()["pairs"] == 4
    orc.score_nbest(hypos, r, rl, accumulate="oracle")
    assert orc.result()["errors"] == 2 * pick([1, 0, 0, 0, 2])["errors"], "calls add up"
    with pytest.raises(ValueError, match="accumulate"):
        te.score_nbest(hypos, r, rl, accumulate="all")
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 5 references"):
        te.score_nbest(hypos[:3], r, rl)
    nothing = te.score_nbest([[], []], r[:2], rl[:2], accumulate="best")
    assert tuple(nothing["errors"].shape) == (2, 1) and nothing["n_hyp"].tolist() == [0, 0] and nothing["sentence_rate"].tolist() == [[-1.0], [-1.0]]
    assert nothing["oracle"].tolist() == [0, 0] and te.result() == EMPTY


def test_nbest_tables_default_is_the_highest_score():
    from fbk_fairseq_st_amd.token_rows import nbest_tables
    hypos = [[{"tokens": torch.tensor([k])} for k in range(3)], []]
    run = lambda hyp, hyp_len, rows: {"stats": hyp.int(), "status": torch.tensor([0, 2, 0], dtype=torch.int32),
                                      "s": torch.tensor([1.0, 0.0, 3.0], dtype=torch.float64)}
    assert nbest_tables(hypos, 2, torch.device("cpu"), run, 1, "s")[4].tolist() == [2, 0]
    assert nbest_tables(hypos, 2, torch.device("cpu"), run, 1, "s", lowest=True)[4].tolist() == [0, 0], "the refused 0.0 is no result"


def test_score_pairs_maps_and_one_matrix(calls):
    te = TE.TextErrorRate.for_dictionary(D)
    h, hl = mat(HYP)
    r, rl = mat(REF)
    hr, rr = [3, 0, 0, 1], [0, 0, 3, 9]
    out = te.score_pairs(h, hl, torch.tensor(hr), r, rl, torch.tensor(rr))
    assert calls[0][4:] == (hr, rr, False) and out["status"].tolist() == [0, 0, 0, 2] and sorted(out) == KEYS
    check_pairs(out, [R.pair(D, HYP[i], REF[j], "word") for i, j in zip(hr[:3], rr[:3])])
    own = te.score_pairs(h, hl, torch.tensor([0, 1]), h, hl, torch.tensor([0, 0]))
    assert calls[-2][6] is True and own["sentence_rate"][0] == 0.0 and own["sentence_accuracy"][0] == 100.0, "one matrix as both sides stays one"
    only_ref = te.score_pairs(h, hl, None, r, rl, torch.tensor([0, 0, 0, 0, 0]))
    assert calls[-2][4] is None
    check_pairs(only_ref, [R.pair(D, x, REF[0], "word") for x in HYP])


def test_ops_and_the_cut_of_their_workspace(calls, monkeypatch):
    te = TE.TextErrorRate.for_dictionary(D)
    (h, hl), (r, rl) = mat(HYP), mat(REF)
    h[1, 0] = len(D)
    out = te.score(h, hl, r, rl, ops=True)
    assert sorted(out) == sorted(KEYS + ["ops", "n_ops", "hyp_units", "ref_units"]) and calls[-1] == ("align", (5, 9), (5, 11), True)
    assert out["ops"].dtype == torch.uint8 and tuple(out["ops"].shape) == (5, 20) and out["status"].tolist() == [0, 2, 0, 0, 0]
    for s, w in enumerate(want_pairs("word")):
        if s == 1:
            assert int(out["n_ops"][s]) == 0
            continue
        n, nh, nr = int(out["n_ops"][s]), int(out["hyp_units_n"][s]), int(out["ref_units_n"][s])
        assert out["ops"][s, :n].tolist() == w["ops"] and out["hyp_units"][s, :nh].tolist() == w["hyp_units"] and out["ref_units"][s, :nr].tolist() == w["ref_units"]
        assert E.replay(out["hyp_units"][s, :nh].tolist(), out["ref_units"][s, :nr].tolist(), out["ops"][s, :n].tolist())
    whole = {k: v.clone() for k, v in out.items()}
    # two pairs per alignment call: the same numbers
    from fbk_fairseq_st_amd import error_rate as ER
    monkeypatch.setattr(ER, "WORKSPACE_LIMIT", 2 * (4 * 10 * 1 + 8 * 9 + 512))
    assert ER.ErrorRate.chunk_sentences(9, 11) == 2
    del calls[:]
    cut = TE.TextErrorRate.for_dictionary(D).score(h, hl, r, rl, ops=True)
    assert [c[:2] for c in calls] == [("units", (5, 4)), ("align", (2, 9)), ("align", (2, 9)), ("align", (1, 9))]
    for k in INTS + ["status", "n_ops", "sentence_rate"]:
        assert torch.equal(cut[k], whole[k]), k
    for s in (0, 2, 3, 4):
        assert cut["ops"][s, :int(cut["n_ops"][s])].tolist() == whole["ops"][s, :int(whole["n_ops"][s])].tolist()
    plain = TE.TextErrorRate.for_dictionary(D).score(h, hl, r, rl)
    assert [c[1] for c in calls[-1:]] == [(5, 9)] and calls[-1][3] is False, "without ops: one alignment call"
    assert torch.equal(plain["errors"], whole["errors"])


def test_value_errors_of_the_class(calls):
    for kw in (dict(unit="words"), dict(unit=0), dict(max_units=-1), dict(max_units=4096)):
        with pytest.raises(ValueError, match="TextErrorRate"):
            TE.TextErrorRate(TABLE, **kw)
    for bad in (dict(TABLE, pieces=TABLE["pieces"].astype(np.int64)), dict(TABLE, piece_off=TABLE["piece_off"][:-1]), dict(TABLE, unk=len(D)),
                dict(TABLE, piece_off=TABLE["piece_off"][::-1].copy()), dict(TABLE, pieces=TABLE["pieces"][:-1])):
        with pytest.raises(ValueError, match="TextErrorRate"):
            TE.TextErrorRate(bad)
        with pytest.raises(ValueError, match="ChrfScorer"):
            CS.ChrfScorer(bad)                                              # the one check, under the owner's name
    te = TE.TextErrorRate(TABLE)
    ok, n1 = torch.zeros(1, 3).long(), torch.tensor([3])
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        te.score(torch.zeros(1, 1025).long(), n1, ok, n1)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        te.score_pairs(ok, n1, None, torch.zeros(1, 1025).long(), n1, None)
    with pytest.raises(ValueError, match="S2T_CHRF_MAX_LEN"):
        te.score_hypotheses([[{"tokens": torch.zeros(1025).long()}]], ok, n1)
    with pytest.raises(ValueError, match="one B"):
        te.score(ok, n1, torch.zeros(2, 3).long(), torch.tensor([3, 3]))
    with pytest.raises(ValueError, match="matrices"):
        te.score_pairs(ok[0], n1, None, ok, n1, None)
    assert calls == [] and te.result() == EMPTY, "nothing was scored"
    one = TE.TextErrorRate(TABLE)
    assert one.table_on("cpu") is one.table_on("cpu"), "copied to a device once"


# ------------------------------------------------------------------ MBRDecoder(utility=TextErrorRate)
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


@pytest.mark.parametrize("unit", ("word", "char"))
def test_mbr_with_a_text_error_utility(calls, monkeypatch, unit):
    monkeypatch.setattr(MB.K, "bleu_pairs", lambda *a, **kw: pytest.fail("the BLEU route was taken"))
    te = TE.TextErrorRate.for_dictionary(D, unit=unit)
    dec = MB.MBRDecoder(None, PAD, EOS, UNK, utility=te)
    hypos = hyp_lists(LISTS)
    out = dec.rerank(hypos)
    want = [R.expected_accuracy(D, ts, ts, unit) for ts in LISTS]
    check_order(out, want, hypos)
    assert [h["mbr_index"] for h in out[0]][:2] == [0, 2], "the two equal hypotheses tie and keep their order"
    assert len(calls) == 2 and calls[0][6] is True, "one unit call and one alignment call, one matrix as both sides"
    assert calls[0][4] == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] + [5] * 3 + [6] * 3 + [7] * 3
    assert calls[0][5] == [0, 1, 2, 3] * 4 + [4] + [5, 6, 7] * 3, "candidate row and pseudo-reference row of every pair of a sentence"
    assert te.result()["pairs"] == 26, "the pairs went through score_pairs"
    # separate pseudo-references, and the three forms of weights
    pseudo = [[T("▁a", "b", "</s>"), T("▁b", "</s>")], [T("▁a", "</s>")], [], [T("▁ab", "</s>"), T("▁a", "▁b", "</s>"), T("c", "</s>")]]
    out = dec.rerank(hypos, pseudo=hyp_lists(pseudo))
    check_order(out, [R.expected_accuracy(D, ts, ps, unit) for ts, ps in zip(LISTS, pseudo)], hypos)
    assert calls[-2][6] is False and [float(h["mbr_score"]) for h in out[2]] == [0.0], "against an empty list the score is 0"
    w = [3.0, 0.0, 1.0]
    check_order(dec.rerank(hypos, pseudo=hyp_lists(pseudo), weights=w),
                [R.expected_accuracy(D, ts, ps, unit, weights=w) for ts, ps in zip(LISTS, pseudo)], hypos)
    per = [[1.0, 2.0], [1.0], [], [0.5, 0.0, 4.0]]
    check_order(dec.rerank(hypos, pseudo=hyp_lists(pseudo), weights=per),
                [R.expected_accuracy(D, ts, ps, unit, weights=ws) for ts, ps, ws in zip(LISTS, pseudo, per)], hypos)
    by_score = [[float(np.exp(-0.5 * k)) for k in range(len(ps))] for ps in pseudo]
    want = [R.expected_accuracy(D, ts, ps, unit, weights=ws) for ts, ps, ws in zip(LISTS, pseudo, by_score)]
    check_order(MB.MBRDecoder(None, PAD, EOS, UNK, weights="score", utility=te).rerank(hypos, pseudo=hyp_lists(pseudo)), want, hypos)
    assert MB.MBRDecoder(None, PAD, EOS, UNK, utility=te).rerank([[], []]) == [[], []]
    assert MB.MBRDecoder.for_dictionary(None, D, utility=te).utility is te


def test_a_refused_candidate_pair_counts_for_nothing(calls):
    te = TE.TextErrorRate.for_dictionary(D)
    lists = [[T("▁a", "▁b"), [len(D)], T("▁a")]]
    out = MB.MBRDecoder(None, PAD, EOS, UNK, utility=te).rerank(hyp_lists(lists))
    gains = {h["mbr_index"]: float(h["mbr_score"]) for h in out[0]}
    assert gains == {0: 50.0, 1: 0.0, 2: 75.0}, "the refused row is no pseudo-reference and has no utility"


def test_the_cut_by_sentences_counts_this_utilitys_bytes(calls, monkeypatch):
    te = TE.TextErrorRate.for_dictionary(D)
    dec = MB.MBRDecoder(None, PAD, EOS, UNK, utility=te)
    hypos = hyp_lists(LISTS)
    assert dec._pair_bytes(hypos, hypos) == te.pair_bytes(4, 4) == 4 * (9 + 9) + 64
    assert dec._pair_bytes(hypos, hyp_lists([[T("▁a") * 7]])) == te.pair_bytes(4, 7)
    assert MB.MBRDecoder(None, PAD, EOS, UNK)._pair_bytes(hypos, hypos) == 44
    assert MB.MBRDecoder(None, PAD, EOS, UNK, utility=CS.ChrfScorer.for_dictionary(D))._pair_bytes(hypos, hypos) == MB._CHRF_PAIR_BYTES == 116
    # a limit that two sentences' pairs pass: the batch is cut, the order is the uncut one
    want = [[h["mbr_index"] for h in hs] for hs in dec.rerank(hypos)]
    n = len(calls)
    monkeypatch.setattr(MB, "OUTPUT_LIMIT", 4 * 4 * te.pair_bytes(4, 4))
    assert MB.MBRDecoder.chunk_sentences([4, 0, 1, 3], [4, 0, 1, 3], te.pair_bytes(4, 4)) == [(0, 2), (2, 4)]
    assert [[h["mbr_index"] for h in hs] for hs in dec.rerank(hypos)] == want and len(calls) == n + 4, "two cuts, two calls each"


def test_utility_none_and_a_chrf_scorer_still_take_their_routes(calls, monkeypatch):
    seen = []

    def bleu_pairs(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, max_list=None):
        seen.append((tuple(cand.shape), max_list))
        return torch.zeros((cand.shape[0], max_list, 10), dtype=torch.int32), torch.zeros((cand.shape[0], max_list), dtype=torch.int32)

    def chrf_stats(hyp, hyp_len, ref, ref_len, pieces, piece_off, unk=-1, char_order=6, word_order=0, hyp_row=None, ref_row=None):
        seen.append(("chrf", hyp_row.shape[0]))
        return torch.zeros((hyp_row.shape[0], 24), dtype=torch.int32), torch.zeros((hyp_row.shape[0],), dtype=torch.int32)
    monkeypatch.setattr(MB.K, "bleu_pairs", bleu_pairs)
    monkeypatch.setattr(CS.K, "chrf_stats", chrf_stats)
    out = MB.MBRDecoder(None, PAD, EOS, UNK).rerank(hyp_lists(LISTS))
    assert seen == [((8, 4), 4)] and [len(hs) for hs in out] == [4, 0, 1, 3]
    sc = CS.ChrfScorer.for_dictionary(D)
    assert not hasattr(sc, "utility_key") and not hasattr(sc, "pair_bytes")
    out = MB.MBRDecoder(None, PAD, EOS, UNK, utility=sc).rerank(hyp_lists(LISTS))
    assert seen[1:] == [("chrf", 26)] and calls == [] and [h["mbr_index"] for h in out[0]] == [0, 1, 2, 3]
