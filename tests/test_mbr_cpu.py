"""The pairwise BLEU entry point and MBRDecoder without a GPU: s2t_bleu_pairs is exported, bound and refuses bad arguments before
anything is launched, the limits and switches are the same in the header and in kernels, kernels.bleu_pairs checks its operands, and
the host logic of MBRDecoder -- reordering and its stability, mbr_index, ragged and empty lists, separate pseudo-references, the
weight forms, the batch cut, both construction paths -- with kernels.bleu_pairs replaced by the Python reference (tests/mbr_ref.py;
the kernel has its own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bleu_ref as R
import mbr_ref as MR
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd import mbr as MB
from fbk_fairseq_st_amd.data import Dictionary

FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
PAD, EOS, UNK = 1, 2, 3
ARGS = (("cand", FAKE), ("cand_len", FAKE), ("cand_elem", 4), ("ref", FAKE), ("ref_len", FAKE), ("ref_elem", 8), ("cand_sent", FAKE),
        ("ref_off", FAKE), ("Rc", 3), ("B", 2), ("Hmax", 7), ("Pmax", 5), ("Rr", 4), ("M", 2), ("pad", PAD), ("eos", EOS), ("unk", UNK),
        ("stats", FAKE), ("status", FAKE), ("stream", None))


def test_export_binding_limits_and_switches():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    assert "s2t_bleu_pairs" in L.SIGNATURES and hasattr(raw, "s2t_bleu_pairs") and hasattr(lib, "s2t_bleu_pairs")
    assert len(L.SIGNATURES["s2t_bleu_pairs"]) == 20 == len(ARGS) and "s2t_bleu_pairs" not in L._SIZE_T_RESULT
    assert lib.s2t_abi_version() == 9
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    for name, value in (("MAX_LEN", K.MBR_MAX_LEN), ("MAX_LIST", K.MBR_MAX_LIST), ("WAVE_LEN", K.MBR_WAVE_LEN), ("GROUP_LEN", K.MBR_GROUP_LEN),
                        ("CHUNK_BYTES", K.MBR_CHUNK_BYTES), ("SLICE", K.MBR_SLICE)):
        assert "#define S2T_MBR_%s %d\n" % (name, value) in text, name
    assert (K.MBR_MAX_LEN, K.MBR_MAX_LIST) == (1024, 256) == (MB.MAX_LEN, MB.MAX_LIST)
    assert "the rule of a pair is s2t_bleu_stats's" in text.lower().replace("\n * ", " ") or "The rule of a pair is s2t_bleu_stats's" in text
    # the chunk: as many padded rows as the bytes hold, at most the slice, never less than one within the limits
    assert K.bleu_pairs_chunk(60, True) == 8 == K.bleu_pairs_chunk(1020, False) == K.MBR_SLICE and K.bleu_pairs_chunk(1021, False) == 7
    assert K.bleu_pairs_chunk(1024, True) == 3 and K.bleu_pairs_chunk(1020, True) == 4 and K.bleu_pairs_chunk(0, False) == 8


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("cand", "cand_len", "ref", "ref_len", "cand_sent", "ref_off", "stats", "status"):
        assert f(**{name: None}) == -22, name                             # required pointers
    for name in ("Hmax", "Pmax", "B", "Rr", "M"):
        assert f(**{name: -1}) == -22, name
    for name in ("cand_elem", "ref_elem"):
        assert f(**{name: 2}) == -22 and f(**{name: 0}) == -22 and f(**{name: 16}) == -22, name
    assert f(pad=EOS) == -22 and f(unk=PAD) == -22 and f(unk=EOS) == -22
    assert f(pad=-1, eos=-1, unk=-1) == -22, "pad == eos is refused whatever unk is"
    assert f(Hmax=1025) == -95 and f(Pmax=1025) == -95 and f(M=257) == -95
    assert f(Hmax=4095) == -95, "the widths of s2t_bleu_stats are not these"
    assert f(Rc=0) == 0 and f(Rc=-3) == 0 and f(M=0) == 0 and f(Rc=0, cand=None, pad=EOS, Hmax=10 ** 6) == 0   # nothing is looked at


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_bleu_pairs)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    raw.s2t_bleu_pairs.argtypes = L.SIGNATURES["s2t_bleu_pairs"]
    check_refusals(fast.s2t_bleu_pairs)
    check_refusals(raw.s2t_bleu_pairs)
    with pytest.raises(TypeError, match="20 arguments"):
        fast.s2t_bleu_pairs(*[d for _, d in ARGS][:-1])


def test_kernels_bleu_pairs_checks_its_operands():
    c, n = torch.zeros(3, 5, dtype=torch.int32), torch.tensor([5, 5, 5], dtype=torch.int32)
    r, m = torch.zeros(2, 4, dtype=torch.int64), torch.tensor([3, 3])
    sent, off = torch.zeros(3, dtype=torch.int32), torch.tensor([0, 2], dtype=torch.int32)
    call = lambda *a, **kw: K.bleu_pairs(*a, **dict(dict(pad=PAD, eos=EOS, max_list=2), **kw))
    for bad in (lambda: call(c[0], n, sent, r, m, off), lambda: call(c.float(), n, sent, r, m, off), lambda: call(c, n.long(), sent, r, m, off),
                lambda: call(c, n, sent, r, m.int(), off), lambda: call(c, n[:1], sent, r, m, off), lambda: call(c, n, sent, r, m[:1], off),
                lambda: call(c, n, sent.long(), r, m, off), lambda: call(c, n, sent[:2], r, m, off), lambda: call(c, n, sent, r, m, off.long()),
                lambda: call(c, n, sent, r, m, off[:0]), lambda: call(c, n, sent, r, m, off.view(1, 2)),
                lambda: call(c, n, sent, r, m, off, pad=EOS), lambda: call(c, n, sent, r, m, off, unk=PAD), lambda: call(c, n, sent, r, m, off, unk=EOS),
                lambda: call(c, n, sent, r, m, off, max_list=257), lambda: call(c, n, sent, r, m, off, max_list=-1),
                lambda: call(torch.zeros(3, 1025, dtype=torch.int32), n, sent, r, m, off),
                lambda: call(c, n, sent, torch.zeros(2, 1025, dtype=torch.int64), m, off)):
        with pytest.raises(ValueError, match="bleu_pairs"):
            bad()
    stats, status = call(c[:0], n[:0], sent[:0], r, m, off)                         # no candidates: nothing is launched
    assert tuple(stats.shape) == (0, 2, 10) and tuple(status.shape) == (0, 2) and stats.dtype == status.dtype == torch.int32
    stats, status = call(c, n, sent, r[:0], m[:0], torch.zeros(2, dtype=torch.int32), max_list=None)     # an empty list: M is 0
    assert tuple(stats.shape) == (3, 0, 10) and tuple(status.shape) == (3, 0)


# ------------------------------------------------------------------ host logic on the Python reference
@pytest.fixture
def calls(monkeypatch):
    c = []

    def bleu_pairs(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, max_list=None):
        assert cand.dtype == cand_len.dtype and ref.dtype == ref_len.dtype and cand.dtype in (torch.int32, torch.int64)
        assert cand_sent.dtype == ref_off.dtype == torch.int32 and tuple(cand_sent.shape) == (cand.shape[0],)
        c.append(dict(cand=tuple(cand.shape), ref=tuple(ref.shape), ids=(pad, eos, unk), same=ref is cand, M=max_list,
                      sent=cand_sent.tolist(), off=ref_off.tolist()))
        out = MR.pair_stats(cand.numpy(), cand_len.numpy(), cand_sent.numpy(), ref.numpy(), ref_len.numpy(), ref_off.numpy(), pad, eos, unk, max_list)
        return tuple(torch.from_numpy(x) for x in out)
    monkeypatch.setattr(MB.K, "bleu_pairs", bleu_pairs)
    return c


def hyp(*v, score=None):
    h = {"tokens": torch.tensor(v + (EOS,), dtype=torch.int64)}
    if score is not None:
        h["score"] = torch.tensor(score)
    return h


def tokens(lists):
    return [[h["tokens"].tolist() for h in hs] for hs in lists]


LISTS = [[hyp(4, 5, 6, 7, score=-0.1), hyp(4, 5, 6, 8, score=-0.5), hyp(9, 9, score=-3.0), hyp(4, 5, 6, 7, score=-4.0)],      # 0 and 3 tie
         [],
         [hyp(5, score=-1.0)],
         [hyp(4, 4, 5, score=-0.2), hyp(UNK, 4, score=-0.3), hyp(4, 4, 5, 6, score=-2.5)]]


def fresh():
    return [[dict(h) for h in hs] for hs in LISTS]


def check_lists(out, lists, want, places=12):
    """out: what rerank returned for `lists`; want: mbr_ref.rank_lists on the same tokens"""
    assert len(out) == len(lists)
    for b, (hs, (gains, order)) in enumerate(zip(out, want)):
        assert [h["mbr_index"] for h in hs] == order, (b, "the order, ties as they came")
        for h in hs:
            assert h is lists[b][h["mbr_index"]], "the same dicts"
            assert h["mbr_score"].dtype == torch.float64 and h["mbr_score"].dim() == 0
            assert float(h["mbr_score"]) == pytest.approx(gains[h["mbr_index"]], rel=10.0 ** -places, abs=0), (b, h["mbr_index"])


def test_rerank_orders_by_expected_utility_and_keeps_ties(calls):
    dec = MB.MBRDecoder(None, PAD, EOS, UNK)
    lists = fresh()
    out = dec.rerank(lists)
    want = MR.rank_lists(tokens(LISTS), PAD, EOS, UNK)
    check_lists(out, lists, want)
    assert [h["mbr_index"] for h in out[0]] == [0, 3, 1, 2], "an exact tie keeps the generator's order; the odd one goes last"
    assert out[1] == [] and [h["mbr_index"] for h in out[2]] == [0]
    assert float(out[2][0]["mbr_score"]) == pytest.approx(R.sentence_bleu(R.stats_counter([5, EOS], [5, EOS], PAD, EOS, UNK)), rel=1e-12)
    unk_self = R.sentence_bleu(R.stats_counter([UNK, 4, EOS], [UNK, 4, EOS], PAD, EOS, UNK))
    assert unk_self < 100.0 == pytest.approx(R.sentence_bleu(R.stats_counter([4, 4, 5, 6], [4, 4, 5, 6], PAD, EOS, UNK)), rel=1e-12), \
        "a hypothesis with an unk scores below 100 against itself"
    assert len(calls) == 1 and calls[0]["same"] and calls[0]["M"] == 4 and calls[0]["ids"] == (PAD, EOS, UNK)
    assert calls[0]["cand"] == (8, 5) and calls[0]["sent"] == [0, 0, 0, 0, 2, 3, 3, 3] and calls[0]["off"] == [0, 4, 4, 5, 8]
    assert all("mbr_score" in h for hs in lists for h in hs), "the dicts that came in gained the fields"


def test_generate_wraps_the_generator_and_both_construction_paths(calls):
    class Gen:
        def __init__(self):
            self.seen = []

        def generate(self, models, sample, prefix_tokens=None):
            self.seen.append((models, sample, prefix_tokens))
            return fresh()

    d = Dictionary.synthetic(12)
    gen = Gen()
    dec = MB.MBRDecoder.for_dictionary(gen, d)
    assert (dec.pad, dec.eos, dec.unk) == (d.pad(), d.eos(), d.unk()) == (PAD, EOS, UNK) and dec.generator is gen and dec.weights == "uniform"
    out = dec.generate(["m"], {"id": 1}, prefix_tokens="p")
    assert gen.seen == [(["m"], {"id": 1}, "p")]
    want = MR.rank_lists(tokens(LISTS), PAD, EOS, UNK)
    assert [[h["mbr_index"] for h in hs] for hs in out] == [o for _, o in want]
    plain = MB.MBRDecoder(gen, PAD, EOS)
    assert plain.unk == -1 and MB.MBRDecoder.for_dictionary(gen, d, weights="score").weights == "score"
    plain.generate(None, None)
    assert calls[-1]["ids"] == (PAD, EOS, -1)
    for bad in ((1, 1, 3), (1, 2, 1), (1, 2, 2)):
        with pytest.raises(ValueError, match="three different ids"):
            MB.MBRDecoder(gen, *bad)
    with pytest.raises(ValueError, match="weights"):
        MB.MBRDecoder(gen, PAD, EOS, weights="rank")
    with pytest.raises(ValueError, match="without a generator"):
        MB.MBRDecoder(None, PAD, EOS).generate(None, None)


def test_separate_pseudo_references(calls):
    dec = MB.MBRDecoder(None, PAD, EOS, UNK)
    lists = fresh()
    pseudo = [[hyp(4, 5, 6, 8), hyp(4, 5)], [hyp(7)], [], [hyp(4, 4, 5, 6, 7, 8, 9), hyp(4, 4), hyp(4), hyp(UNK, 4), hyp(5, 5)]]
    out = dec.rerank(lists, pseudo=pseudo)
    want = MR.rank_lists(tokens(LISTS), PAD, EOS, UNK, pseudo=tokens(pseudo))
    check_lists(out, lists, want)
    assert not calls[0]["same"] and calls[0]["ref"] == (8, 8) and calls[0]["M"] == 5 and calls[0]["off"] == [0, 2, 3, 3, 8]
    assert [h["mbr_index"] for h in out[0]][0] == 1 and float(out[2][0]["mbr_score"]) == 0.0, "no pseudo-references: gain 0"
    assert "mbr_score" not in pseudo[0][0]
    with pytest.raises(ValueError, match="4 sentences of hypotheses, 3 of pseudo-references"):
        dec.rerank(lists, pseudo=pseudo[:3])
    with pytest.raises(ValueError, match="S2T_MBR_MAX_LIST"):
        dec.rerank([[hyp(4)]], pseudo=[[hyp(4)] * 257])


def test_the_weight_forms(calls):
    lists = fresh()
    toks = tokens(LISTS)
    scores = [[float(h["score"]) for h in hs] for hs in LISTS]
    by_score = [[float(np.exp(np.float64(s) - max(ss))) for s in ss] for ss in scores]
    out = MB.MBRDecoder(None, PAD, EOS, UNK, weights="score").rerank(lists)
    check_lists(out, lists, MR.rank_lists(toks, PAD, EOS, UNK, weights=by_score), places=6)       # the fixture's scores are float32
    dec = MB.MBRDecoder(None, PAD, EOS, UNK)
    per = [[0.0, 2.0, 1.0, 0.5], [], [3.0], [1.0, 0.0, 0.0]]
    for form in (per, [torch.tensor(w) for w in per]):
        lists = fresh()
        check_lists(dec.rerank(lists, weights=form), lists, MR.rank_lists(toks, PAD, EOS, UNK, weights=per))
    flat = [1.0, 0.25, 0.0, 4.0]
    for form in (flat, torch.tensor(flat), torch.tensor([flat] * 4)):
        lists = fresh()
        check_lists(dec.rerank(lists, weights=form), lists, MR.rank_lists(toks, PAD, EOS, UNK, weights=[flat[:len(hs)] for hs in LISTS]))
    lists = fresh()
    zero = dec.rerank(lists, weights=[0.0] * 4)
    assert all(float(h["mbr_score"]) == 0.0 for hs in zero for h in hs) and [h["mbr_index"] for h in zero[0]] == [0, 1, 2, 3]
    assert MR.rank_lists(toks, PAD, EOS, UNK, weights=per)[0][1] != MR.rank_lists(toks, PAD, EOS, UNK)[0][1], "the weights decide an order here"
    for bad, msg in ((per[:3], "3 sequences of weights for 4 sentences"), ([[1.0] * 3, [], [1.0], [1.0] * 3], "3 weights for the 4"),
                     ([1.0, 1.0], "2 weights for the 4"), ([1.0, -1.0, 1.0, 1.0], "non-negative"), ("rank", "weights is")):
        with pytest.raises(ValueError, match=msg):
            dec.rerank(fresh(), weights=bad)


def test_the_batch_is_cut_by_sentences(calls, monkeypatch):
    dec = MB.MBRDecoder(None, PAD, EOS, UNK, weights="score")
    whole = dec.rerank(fresh())
    assert len(calls) == 1
    monkeypatch.setattr(MB, "OUTPUT_LIMIT", 44 * 16)                      # 4 candidates x 4 pseudo-references
    assert MB.MBRDecoder.chunk_sentences([4, 0, 1, 3], [4, 0, 1, 3]) == [(0, 2), (2, 4)]
    monkeypatch.setattr(MB, "OUTPUT_LIMIT", 44 * 10)                      # sentence 0 passes it alone: a range of its own
    assert MB.MBRDecoder.chunk_sentences([4, 0, 1, 3], [4, 0, 1, 3]) == [(0, 1), (1, 3), (3, 4)]
    assert MB.MBRDecoder.chunk_sentences([], []) == [] and MB.MBRDecoder.chunk_sentences([9], [9]) == [(0, 1)]
    lists = fresh()
    cut = dec.rerank(lists)
    assert [c["cand"][0] for c in calls[1:]] == [4, 1, 3] and [c["M"] for c in calls[1:]] == [4, 1, 3]
    assert [c["sent"] for c in calls[1:]] == [[0, 0, 0, 0], [1], [0, 0, 0]] and calls[2]["off"] == [0, 0, 1]
    for a, b in zip(whole, cut):
        assert [h["mbr_index"] for h in a] == [h["mbr_index"] for h in b]
        assert [float(h["mbr_score"]) for h in a] == [float(h["mbr_score"]) for h in b], "sentences are independent: the cut changes nothing"
    per = [[0.0, 2.0, 1.0, 0.5], [], [3.0], [1.0, 0.0, 0.0]]
    lists = fresh()
    check_lists(dec.rerank(lists, weights=per), lists, MR.rank_lists(tokens(LISTS), PAD, EOS, UNK, weights=per))


def test_expected_bleu_fields_refusals_and_first_best(calls):
    dec = MB.MBRDecoder(None, PAD, EOS, UNK)
    lists = [[[4, 5, 4], [5, 5], [4, 5, 4]], [], [[4], [4, 4, 5, EOS], [5], [4]]]
    cand, cand_len, sent, off = MR.matrices(lists, width=5)
    cand_len[4], sent[1] = 6, 9                                           # a refused length (candidate and pseudo-reference), a sentence outside
    w = [1.0, 0.5, 2.0, 2.0, 1.0, 0.25, 2.0]
    t = torch.from_numpy
    tc, tn = t(cand), t(cand_len)
    out = dec.expected_bleu(tc, tn, t(sent), tc, tn, t(off), weights=w, max_list=4)
    want = MR.expected_bleu(cand, cand_len, sent, cand, cand_len, off, PAD, EOS, UNK, w, M=4)
    assert sorted(out) == ["best", "gain", "stats", "status", "utility"] and calls[-1]["same"] and calls[-1]["M"] == 4
    assert out["stats"].tolist() == want["stats"].tolist() and out["status"].tolist() == want["status"].tolist()
    assert out["utility"].dtype == out["gain"].dtype == torch.float64 and out["best"].dtype == torch.int64
    assert tuple(out["utility"].shape) == (7, 4) and tuple(out["gain"].shape) == (7,) and tuple(out["best"].shape) == (3,)
    for c in range(7):
        assert out["gain"][c].item() == pytest.approx(want["gain"][c], rel=1e-12, abs=0), c
        for k in range(4):
            assert out["utility"][c, k].item() == pytest.approx(want["utility"][c][k], rel=1e-12, abs=0), (c, k)
    assert out["gain"][1].item() == -1.0 == out["gain"][4].item() and out["status"][1].tolist() == [2] * 4 and out["status"][4].tolist() == [2] * 4
    assert out["status"][3].tolist() == [0, 2, 0, 0] and out["status"][0].tolist() == [0] * 4
    assert out["best"].tolist() == want["best"] == [0, -1, 3], "rows 0 and 2 tie: the first; rows 3 and 6 tie: the first"
    uniform = dec.expected_bleu(tc, tn, t(sent), tc, tn, t(off))
    assert calls[-1]["M"] is None and uniform["gain"].tolist() == pytest.approx(MR.expected_bleu(cand, cand_len, sent, cand, cand_len, off, PAD, EOS, UNK)["gain"], rel=1e-12)
    bad_off = np.array([0, 3, 2, 7], np.int32)                            # sentence 1 descends: its candidates have no list
    sent2 = np.array([0, 1, 0, 2, 2, 2, 2], np.int32)
    got = dec.expected_bleu(tc, tn, t(sent2), tc, tn, t(bad_off), max_list=5)
    ref = MR.expected_bleu(cand, cand_len, sent2, cand, cand_len, bad_off, PAD, EOS, UNK, M=5)
    assert got["status"].tolist() == ref["status"].tolist() and got["gain"][1].item() == -1.0 and got["best"].tolist() == ref["best"]
    assert got["gain"].tolist() == pytest.approx(ref["gain"], rel=1e-12)
    none = dec.expected_bleu(t(cand[:0]), t(cand_len[:0]), t(sent[:0]), t(cand), t(cand_len), t(off), max_list=4)
    assert none["best"].tolist() == [-1, -1, -1] and tuple(none["gain"].shape) == (0,)
    with pytest.raises(ValueError, match="S2T_MBR_MAX_LEN"):
        dec.expected_bleu(torch.zeros(1, 1025).long(), torch.tensor([3]), torch.tensor([0]), t(cand), t(cand_len), t(off))
    with pytest.raises(ValueError, match="one weight per pseudo-reference row"):
        dec.expected_bleu(tc, tn, t(sent), tc, tn, t(off), weights=w[:3])
