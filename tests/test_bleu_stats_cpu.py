"""The BLEU statistics entry point without a GPU: it is exported, bound and refuses bad arguments before anything is launched, the
limit is the same in the header, in kernels and in the class, and the host logic of BleuScorer -- result keys and dtypes, the sums
and the arithmetic of result() and result_string(), reset(), refused sentences, the best hypothesis of every sentence, n-best lists
with ragged N and both accumulate modes -- with kernels.bleu_stats replaced by the Python reference (tests/bleu_ref.py; the kernel has
its own tests)."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import bleu_ref as R
from fbk_fairseq_st_amd import bleu_scorer as BS
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd.data import Dictionary

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
MAX_LEN = 4095
PAD, EOS, UNK = 1, 2, 3
ARGS = (("hyp", FAKE), ("hyp_len", FAKE), ("hyp_elem", 4), ("ref", FAKE), ("ref_len", FAKE), ("ref_elem", 8), ("ref_row", None), ("B", 2),
        ("Hmax", 7), ("Rmax", 5), ("Rrows", 2), ("pad", PAD), ("eos", EOS), ("unk", UNK), ("stats", FAKE), ("status", FAKE), ("stream", None))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleu_stats.npz")


def test_export_binding_and_limit():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert "s2t_bleu_stats" in L.SIGNATURES and hasattr(raw, "s2t_bleu_stats") and hasattr(lib, "s2t_bleu_stats")
    assert len(L.SIGNATURES["s2t_bleu_stats"]) == 17 == len(ARGS) and "s2t_bleu_stats" not in L._SIZE_T_RESULT
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    assert "#define S2T_BLEU_MAX_LEN %d" % MAX_LEN in text and "#define S2T_BLEU_WAVE_LEN %d" % K.BLEU_WAVE_LEN in text
    assert "#define S2T_BLEU_GROUP_LEN %d" % K.BLEU_GROUP_LEN in text
    assert K.BLEU_MAX_LEN == MAX_LEN == BS.MAX_LEN


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("hyp", "hyp_len", "ref", "ref_len", "stats", "status"):
        assert f(**{name: None}) == -22, name                             # required pointers
    assert f(Hmax=-1) == -22 and f(Rmax=-1) == -22
    for name in ("hyp_elem", "ref_elem"):
        assert f(**{name: 2}) == -22 and f(**{name: 0}) == -22 and f(**{name: 16}) == -22, name
    assert f(Rrows=3) == -22 and f(Rrows=1) == -22, "without a map there is one reference per hypothesis"
    assert f(Rrows=-1, ref_row=FAKE) == -22
    assert f(pad=EOS) == -22 and f(unk=PAD) == -22 and f(unk=EOS) == -22
    assert f(pad=-1, eos=-1, unk=-1) == -22, "pad == eos is refused whatever unk is"
    assert f(Hmax=MAX_LEN + 1) == -95 and f(Rmax=MAX_LEN + 1) == -95 and f(Rmax=MAX_LEN + 1, Rrows=9, ref_row=FAKE) == -95
    assert f(B=0) == 0 and f(B=-3) == 0 and f(B=0, hyp=None, pad=EOS, Hmax=10 ** 6) == 0     # an empty problem: nothing is looked at


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_bleu_stats)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_bleu_stats.argtypes = L.SIGNATURES["s2t_bleu_stats"]
    check_refusals(fast.s2t_bleu_stats)
    check_refusals(raw.s2t_bleu_stats)


def test_kernels_bleu_stats_checks_its_operands():
    h, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([5, 5], dtype=torch.int32)
    r, m = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    rows = torch.zeros(2, dtype=torch.int32)
    call = lambda *a, **kw: K.bleu_stats(*a, **dict(dict(pad=PAD, eos=EOS), **kw))
    for bad in (lambda: call(h[0], n, r, m), lambda: call(h.float(), n, r, m), lambda: call(h, n.long(), r, m),
                lambda: call(h, n, r, m.int()), lambda: call(h, n[:1], r, m), lambda: call(h, n, r, m[:1]),
                lambda: call(h, n, r[:1], m[:1]), lambda: call(h, n, r, m, ref_row=rows.long()), lambda: call(h, n, r, m, ref_row=rows[:1]),
                lambda: call(h, n, r, m, pad=EOS), lambda: call(h, n, r, m, unk=PAD), lambda: call(h, n, r, m, unk=EOS),
                lambda: call(torch.zeros(2, MAX_LEN + 1, dtype=torch.int32), n, r, m),
                lambda: call(h, n, torch.zeros(2, MAX_LEN + 1, dtype=torch.int64), m)):
        with pytest.raises(ValueError, match="bleu_stats"):
            bad()
    stats, status = call(h[:0], n[:0], r[:0], m[:0])                           # no sentences: nothing is launched
    assert tuple(stats.shape) == (0, 10) and tuple(status.shape) == (0,) and stats.dtype == status.dtype == torch.int32
    stats, _ = call(h[:0], n[:0], r, m, ref_row=rows[:0])
    assert tuple(stats.shape) == (0, 10)


# ------------------------------------------------------------------ host logic on the Python reference
@pytest.fixture
def calls(monkeypatch):
    c = []

    def bleu_stats(hyp, hyp_len, ref, ref_len, pad, eos, unk=-1, ref_row=None):
        assert hyp.dtype == hyp_len.dtype and ref.dtype == ref_len.dtype and hyp.dtype in (torch.int32, torch.int64)
        assert ref_row is None or (ref_row.dtype == torch.int32 and tuple(ref_row.shape) == (hyp.shape[0],))
        c.append((tuple(hyp.shape), tuple(ref.shape), (pad, eos, unk), None if ref_row is None else ref_row.tolist()))
        out = R.bleu_stats_batch(hyp.numpy(), hyp_len.numpy(), ref.numpy(), ref_len.numpy(), pad, eos, unk,
                                 None if ref_row is None else ref_row.numpy())
        return tuple(torch.from_numpy(x) for x in out)
    monkeypatch.setattr(BS.K, "bleu_stats", bleu_stats)
    return c


HYP = [[4, 5, 6, 7, EOS, PAD], [4, 4, EOS, PAD, PAD, PAD], [PAD] * 6, [9, 8, 7, 6, 5, EOS]]
HYP_LEN = [5, 3, 0, 6]
REF = [[4, 5, 6, 8, 7, EOS], [4, 4, 4, EOS, PAD, PAD], [5, 5, EOS, PAD, PAD, PAD], [9, 8, 7, 5, EOS, PAD]]
REF_LEN = [6, 4, 3, 5]
KEYS = ["count", "match", "ref_len", "sentence_bleu", "stats", "status", "sys_len"]
EMPTY = dict(ref_len=0, sys_len=0, match1=0, count1=0, match2=0, count2=0, match3=0, count3=0, match4=0, count4=0,
             bleu=0.0, precisions=[0.0] * 4, brevity=0.0, ratio=0.0)


def want_rows(hyp=HYP, hyp_len=HYP_LEN, ref=REF, ref_len=REF_LEN, unk=UNK):
    return [R.stats_counter(h[:n], r[:m], PAD, EOS, unk) for h, n, r, m in zip(hyp, hyp_len, ref, ref_len)]


def test_score_fields_sums_and_result(calls):
    bs = BS.BleuScorer(PAD, EOS, UNK)
    assert bs.result() == EMPTY, "an empty accumulator: zeros, nothing divided"
    assert bs.result_string() == "BLEU4 = 0.00, 0.0/0.0/0.0/0.0 (BP=0.000, ratio=0.000, syslen=0, reflen=0)"
    out = bs.score(torch.tensor(HYP), torch.tensor(HYP_LEN), torch.tensor(REF), torch.tensor(REF_LEN))
    assert sorted(out) == KEYS and calls == [((4, 6), (4, 6), (PAD, EOS, UNK), None)]
    want = want_rows()
    assert want[0] == [5, 4, 4, 4, 2, 3, 1, 2, 0, 1] and want[2] == [2] + [0] * 9
    assert out["stats"].tolist() == want and out["stats"].dtype == torch.int32 and tuple(out["stats"].shape) == (4, 10)
    assert out["match"].tolist() == [w[2::2] for w in want] and out["count"].tolist() == [w[3::2] for w in want]
    assert out["sys_len"].tolist() == [4, 2, 0, 5] and out["ref_len"].tolist() == [5, 3, 2, 4] and out["status"].tolist() == [0] * 4
    assert out["sentence_bleu"].dtype == torch.float64 and out["sentence_bleu"][2] == 0.0
    for s, w in enumerate(want):
        assert float(out["sentence_bleu"][s]) == pytest.approx(R.sentence_bleu(w), rel=1e-12, abs=0), s
    sums = np.array(want).sum(0).tolist()
    res = bs.result()
    assert [res[k] for k in BS._SUMS] == sums and all(isinstance(res[k], int) for k in BS._SUMS)
    assert res["bleu"] == R.score(sums) and res["precisions"] == R.precisions(sums) and res["brevity"] == R.brevity(sums)
    assert res["ratio"] == sums[1] / sums[0] and bs.result_string() == R.result_string(sums)
    assert bs.result_string(order=2) == R.result_string(sums, order=2)
    bs.score(torch.tensor(HYP)[:2], torch.tensor(HYP_LEN)[:2], torch.tensor(REF)[:2], torch.tensor(REF_LEN)[:2])
    twice = (np.array(sums) + np.array(want[:2]).sum(0)).tolist()
    assert [bs.result()[k] for k in BS._SUMS] == twice and bs.result_string() == R.result_string(twice), "calls add up"
    bs.reset()
    assert bs.result() == EMPTY
    # nothing matches at order 4: bleu is 0.0, the rest stands
    bs.score(torch.tensor([[4, 5, 6]]), torch.tensor([3]), torch.tensor([[4, 5, 6]]), torch.tensor([3]))
    res = bs.result()
    assert res["bleu"] == 0.0 and res["precisions"] == [1.0, 1.0, 1.0, 0] and res["brevity"] == 1 and res["ratio"] == 1.0
    assert bs.result_string() == "BLEU4 = 0.00, 100.0/100.0/100.0/0.0 (BP=1.000, ratio=1.000, syslen=3, reflen=3)"
    with pytest.raises(ValueError, match="order > 4"):
        bs.result_string(order=5)


def test_refused_sentences_add_nothing(calls):
    bs = BS.BleuScorer(PAD, EOS)
    out = bs.score(torch.tensor(HYP, dtype=torch.int32), torch.tensor([5, 7, 0, -1]), torch.tensor(REF), torch.tensor([6, 4, 7, 5]))
    assert out["status"].tolist() == [0, 2, 2, 2] and out["stats"][1:].eq(0).all() and out["sentence_bleu"][1:].eq(0).all()
    assert [bs.result()[k] for k in BS._SUMS] == want_rows(unk=-1)[0] and calls[0][2] == (PAD, EOS, -1)
    assert calls[0][0] == (4, 6) and out["stats"].dtype == torch.int32


def test_for_dictionary_and_the_three_ids(calls):
    d = Dictionary.synthetic(9)
    bs = BS.BleuScorer.for_dictionary(d)
    assert (bs.pad, bs.eos, bs.unk) == (d.pad(), d.eos(), d.unk()) == (PAD, EOS, UNK)
    one = bs.score(torch.tensor([[UNK, 4]]), torch.tensor([2]), torch.tensor([[UNK, 4]]), torch.tensor([2]))
    assert one["match"].tolist() == [[1, 0, 0, 0]] and one["count"].tolist() == [[2, 1, 0, 0]], "a reference unk matches nothing"
    off = BS.BleuScorer(PAD, EOS).score(torch.tensor([[UNK, 4]]), torch.tensor([2]), torch.tensor([[UNK, 4]]), torch.tensor([2]))
    assert off["match"].tolist() == [[2, 1, 0, 0]]
    for bad in ((1, 1, 3), (1, 2, 1), (1, 2, 2)):
        with pytest.raises(ValueError, match="three different ids"):
            BS.BleuScorer(*bad)


def test_score_hypotheses_takes_the_best(calls):
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    hypos = [[{"tokens": t(4, 5, 6, EOS)}, {"tokens": t(4, 5, 6, 8, 7, EOS)}], [{"tokens": t(4, EOS)}], [], [{"tokens": t(EOS)}]]
    bs = BS.BleuScorer(PAD, EOS, UNK)
    out = bs.score_hypotheses(hypos, torch.tensor(REF), torch.tensor(REF_LEN))
    assert calls == [((4, 4), (4, 6), (PAD, EOS, UNK), None)] and sorted(out) == KEYS
    want = want_rows([[4, 5, 6, EOS], [4, EOS], [], [EOS]], [4, 2, 0, 1])
    assert out["stats"].tolist() == want and out["sys_len"].tolist() == [3, 1, 0, 1] and out["match"][:, 0].tolist() == [3, 1, 0, 0]
    assert [bs.result()[k] for k in BS._SUMS] == np.array(want).sum(0).tolist()
    i32 = BS.BleuScorer(PAD, EOS).score_hypotheses([[{"tokens": h[0]["tokens"].int()}] for h in hypos[:2]], torch.tensor(REF)[:2],
                                                   torch.tensor(REF_LEN)[:2])
    assert i32["stats"].tolist() == want[:2]
    none = BS.BleuScorer(PAD, EOS).score_hypotheses([[], []], torch.tensor(REF)[:2], torch.tensor(REF_LEN)[:2])
    assert none["ref_len"].tolist() == [5, 3] and none["sys_len"].tolist() == [0, 0] and calls[-1][0] == (2, 0)
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 4 references"):
        bs.score_hypotheses(hypos[:3], torch.tensor(REF), torch.tensor(REF_LEN))


def test_score_nbest_ragged_lists_and_both_accumulate_modes(calls):
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    hypos = [[{"tokens": t(4, 5, 6, EOS)}, {"tokens": t(4, 5, 6, 8, 7, EOS)}, {"tokens": t(7, EOS)}],     # the second is the reference
             [{"tokens": t(4, 4, EOS)}],
             [],
             [{"tokens": t(9, 8, EOS)}, {"tokens": t(9, 8, EOS)}]]                                        # a tie: the first wins
    ref, ref_len = torch.tensor(REF), torch.tensor(REF_LEN)
    bs = BS.BleuScorer(PAD, EOS, UNK)
    out = bs.score_nbest(hypos, ref, ref_len)
    assert calls == [((6, 6), (4, 6), (PAD, EOS, UNK), [0, 0, 0, 1, 3, 3])]
    assert sorted(out) == sorted(KEYS + ["n_hyp", "oracle"]) and bs.result() == EMPTY, "accumulate=None adds nothing"
    assert out["n_hyp"].tolist() == [3, 1, 0, 2] and out["oracle"].tolist() == [1, 0, 0, 0] and out["oracle"].dtype == torch.int64
    assert tuple(out["stats"].shape) == (4, 3, 10) and tuple(out["match"].shape) == (4, 3, 4) and tuple(out["sentence_bleu"].shape) == (4, 3)
    for b, hs in enumerate(hypos):
        for k in range(3):
            if k < len(hs):
                w = R.stats_counter(hs[k]["tokens"].tolist(), REF[b][:REF_LEN[b]], PAD, EOS, UNK)
                assert out["stats"][b, k].tolist() == w and out["ref_len"][b, k] == w[0] and out["sys_len"][b, k] == w[1]
                assert float(out["sentence_bleu"][b, k]) == pytest.approx(R.sentence_bleu(w), rel=1e-12, abs=0)
            else:
                assert out["stats"][b, k].eq(0).all() and out["sentence_bleu"][b, k] == -1.0 and out["status"][b, k] == 0
    assert float(out["sentence_bleu"][0, 1]) == pytest.approx(100.0, rel=1e-12)
    pick = lambda idx: np.array([out["stats"][b, k].tolist() for b, k in enumerate(idx) if len(hypos[b])]).sum(0).tolist()
    best = BS.BleuScorer(PAD, EOS, UNK)
    best.score_nbest(hypos, ref, ref_len, accumulate="best")
    assert [best.result()[k] for k in BS._SUMS] == pick([0, 0, 0, 0])
    orc = BS.BleuScorer(PAD, EOS, UNK)
    orc.score_nbest(hypos, ref, ref_len, accumulate="oracle")
    assert [orc.result()[k] for k in BS._SUMS] == pick([1, 0, 0, 0]) and orc.result()["bleu"] > best.result()["bleu"]
    orc.score_nbest(hypos, ref, ref_len, accumulate="oracle")
    assert orc.result()["match1"] == 2 * pick([1, 0, 0, 0])[2], "calls add up"
    with pytest.raises(ValueError, match="accumulate"):
        bs.score_nbest(hypos, ref, ref_len, accumulate="all")
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 4 references"):
        bs.score_nbest(hypos[:3], ref, ref_len)
    nothing = bs.score_nbest([[], []], ref[:2], ref_len[:2], accumulate="best")
    assert tuple(nothing["stats"].shape) == (2, 1, 10) and nothing["n_hyp"].tolist() == [0, 0] and nothing["sentence_bleu"].tolist() == [[-1.0], [-1.0]]
    assert bs.result() == EMPTY


def test_result_string_equals_the_reference_scorer(calls):
    """the fixture's strings are the reference's Scorer.result_string() over the same pairs"""
    g = dict(np.load(GOLDEN))
    t = lambda k: torch.from_numpy(g[k])
    for name in ("all", "first", "small_alphabets", "quirks"):
        idx = torch.from_numpy(g["subset_" + name]).long()
        bs = BS.BleuScorer(int(g["pad"]), int(g["eos"]), int(g["unk"]))
        half = len(idx) // 2
        for part in (idx[:half], idx[half:]):
            out = bs.score(t("hyp")[part], t("hyp_len")[part], t("ref")[part], t("ref_len")[part])
            assert out["stats"].tolist() == g["stats"][part.numpy()].tolist()
        assert bs.result_string() == str(g["string_" + name]), name
        assert bs.result_string(order=2) == str(g["string2_" + name]), name
        assert bs.result()["bleu"] == float(g["score_" + name])
        assert bs.result()["ref_len"] == int(g["stats"][idx.numpy(), 0].sum())


def test_value_errors(calls):
    bs = BS.BleuScorer(PAD, EOS, UNK)
    ok, n1 = torch.zeros(1, 3).long(), torch.tensor([3])
    with pytest.raises(ValueError, match="S2T_BLEU_MAX_LEN"):
        bs.score(torch.zeros(1, MAX_LEN + 1).long(), n1, ok, n1)
    with pytest.raises(ValueError, match="S2T_BLEU_MAX_LEN"):
        bs.score(ok, n1, torch.zeros(1, MAX_LEN + 1).long(), n1)
    with pytest.raises(ValueError, match="S2T_BLEU_MAX_LEN"):
        bs.score_hypotheses([[{"tokens": torch.zeros(MAX_LEN + 1).long()}]], ok, n1)
    with pytest.raises(ValueError, match="one B"):
        bs.score(ok, n1, torch.zeros(2, 3).long(), torch.tensor([3, 3]))
    assert calls == [] and bs.result() == EMPTY, "nothing was scored"
    assert math.isinf(BS._corpus([0, 3, 0, 3, 0, 2, 0, 1, 0, 0], 4)["ratio"])


# ------------------------------------------------------------------ token_rows: what the four scorers share
def test_token_rows_dtypes_and_empty_lists():
    from fbk_fairseq_st_amd import token_rows as TR
    for dt, want in ((torch.int32, torch.int32), (torch.int64, torch.int64), (torch.int16, torch.int64), (torch.uint8, torch.int64),
                     (torch.float32, torch.int64)):
        tok, ln = TR.as_ints(torch.tensor([[4, 5], [6, 7]]).to(dt), torch.tensor([2, 1], dtype=torch.int16), "cpu")
        assert tok.dtype == want and ln.dtype == want and tok.tolist() == [[4, 5], [6, 7]] and ln.tolist() == [2, 1], dt
    t = lambda dt, *v: torch.tensor(v, dtype=dt)
    mat, ln = TR.pad_rows([t(torch.int32, 4, 5, 6), t(torch.int32), t(torch.int32, 7)], "cpu")
    assert mat.dtype == ln.dtype == torch.int32 and mat.tolist() == [[4, 5, 6], [0, 0, 0], [7, 0, 0]] and ln.tolist() == [3, 0, 1]
    mat, ln = TR.pad_rows([t(torch.int32, 4, 5), t(torch.int64, 7)], "cpu")                # one row that is not int32: int64
    assert mat.dtype == ln.dtype == torch.int64 and mat.tolist() == [[4, 5], [7, 0]] and ln.tolist() == [2, 1]
    mat, ln = TR.pad_rows([], "cpu")
    assert tuple(mat.shape) == (0, 0) and tuple(ln.shape) == (0,) and mat.dtype == ln.dtype == torch.int64
    mat, ln = TR.pad_rows([t(torch.int32), t(torch.int32)], "cpu")                         # rows without tokens: width 0
    assert tuple(mat.shape) == (2, 0) and ln.tolist() == [0, 0] and mat.dtype == torch.int32
    best = TR.best_rows([[{"tokens": t(torch.int32, 4, 5)}, {"tokens": t(torch.int32, 9)}], [], [{"tokens": t(torch.int64, 6).reshape(1, 1)}]], "cpu")
    assert [b.tolist() for b in best] == [[4, 5], [], [6]] and [b.dtype for b in best] == [torch.int32, torch.int64, torch.int64]


def test_nbest_tables_with_a_stub_run():
    """the helper of both score_nbest methods on a run() that needs no kernel: the flat list it hands over, the scatter, the first
    maximum, the picked sums; and a batch without sentences, which the scorers' tests do not reach"""
    from fbk_fairseq_st_amd import token_rows as TR
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    hypos = [[{"tokens": t(4, 5)}, {"tokens": t(9, 9, 9)}, {"tokens": t(9, 9, 9)}], [], [{"tokens": t(7)}]]
    seen = []

    def run(hyp, hyp_len, rows):                                   # stats: (first token, length, row), the score is the length
        seen.append((hyp.tolist(), hyp_len.tolist(), rows.tolist(), rows.dtype))
        stats = torch.stack([hyp[:, :1].sum(1).int(), hyp_len.int(), rows], 1)
        return {"stats": stats, "status": torch.full((hyp.shape[0],), 2, dtype=torch.int32), "points": hyp_len.double()}
    stats, status, score, n_hyp, oracle, pick = TR.nbest_tables(hypos, 3, "cpu", run, 3, "points")
    assert seen == [([[4, 5, 0], [9, 9, 9], [9, 9, 9], [7, 0, 0]], [2, 3, 3, 1], [0, 0, 0, 2], torch.int32)]
    assert stats.dtype == status.dtype == torch.int32 and score.dtype == torch.float64 and n_hyp.dtype == oracle.dtype == torch.int64
    assert stats.tolist() == [[[4, 2, 0], [9, 3, 0], [9, 3, 0]], [[0, 0, 0]] * 3, [[7, 1, 2], [0, 0, 0], [0, 0, 0]]]
    assert status.tolist() == [[2, 2, 2], [0, 0, 0], [2, 0, 0]] and score.tolist() == [[2, 3, 3], [-1, -1, -1], [1, -1, -1]]
    assert n_hyp.tolist() == [3, 0, 1] and oracle.tolist() == [1, 0, 0], "the first of two equal maxima; 0 for an empty list"
    assert pick("best").tolist() == [11, 3, 2] and pick("oracle").tolist() == [16, 4, 2] and pick("best").dtype == torch.int64
    stats, status, score, n_hyp, oracle, pick = TR.nbest_tables([], 0, "cpu", run, 3, "points")
    assert tuple(stats.shape) == (0, 1, 3) and tuple(score.shape) == (0, 1) and tuple(oracle.shape) == (0,) and oracle.dtype == torch.int64
    assert seen[-1][0] == [] and n_hyp.tolist() == []
