"""The edit-distance aligner without a GPU: the new entry points are exported, bound and refuse bad arguments before anything is
launched, the workspace formula, and the host logic of ErrorRate -- result keys and dtypes, the sums and the arithmetic of result(),
reset(), refused sentences, EOS stripping, the best hypothesis of every sentence, chunking of calls with ops, the refusals -- with
kernels.edit_align replaced by the Python reference (tests/edit_ref.py; the kernels have their own tests)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import edit_ref as R
from fbk_fairseq_st_amd import error_rate as ER
from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd.data import Dictionary

NEW = ("s2t_edit_align_workspace", "s2t_edit_align")
FAKE = 1 << 20            # a non-null pointer: a refused call reads and writes nothing
MAX_A, MAX_B = 32767, 4095
ARGS = (("a", FAKE), ("a_len", FAKE), ("a_elem", 4), ("b", FAKE), ("b_len", FAKE), ("b_elem", 8), ("B", 2), ("Amax", 7), ("Bmax", 5),
        ("cs", 4), ("ca", 3), ("cb", 3), ("collapse", 0), ("blank", 0), ("ws", FAKE), ("counts", FAKE), ("cost", FAKE), ("status", FAKE),
        ("a_n", FAKE), ("a_out", FAKE), ("ops", FAKE), ("n_ops", FAKE), ("stream", None))


def ws_bytes(B, Amax, Bmax, want_ops):
    r = lambda x: (x + 255) // 256 * 256
    return r(8 * B * Amax) + (r(4 * B * (Amax + 1) * ((Bmax + 1 + 15) // 16)) if want_ops else 0)


def test_exports_bindings_and_workspace_size():
    lib = L.load()
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(raw, name) and hasattr(lib, name)
    assert "s2t_edit_align_workspace" in L._SIZE_T_RESULT
    assert len(L.SIGNATURES["s2t_edit_align"]) == 23 and len(L.SIGNATURES["s2t_edit_align_workspace"]) == 4
    assert lib.s2t_abi_version() == 9
    for B, Amax, Bmax in ((64, 375, 60), (16, 1500, 1024), (1, 0, 0), (1, MAX_A, MAX_B), (3, 7, 15), (3, 7, 16), (5, 1, 4095)):
        for want in (0, 1):
            assert lib.s2t_edit_align_workspace(B, Amax, Bmax, want) == ws_bytes(B, Amax, Bmax, want), (B, Amax, Bmax, want)
    # without ops nothing grows with n * m; with ops 2 bits per cell
    assert lib.s2t_edit_align_workspace(4, 1000, 4000, 0) == lib.s2t_edit_align_workspace(4, 1000, 0, 0) <= 8 * 4 * 1000 + 256
    assert lib.s2t_edit_align_workspace(4, 1000, 4000, 1) >= 4 * 1001 * 4001 // 4
    assert lib.s2t_edit_align_workspace(0, 5, 5, 1) == 0 and lib.s2t_edit_align_workspace(-1, 5, 5, 1) == 0
    assert lib.s2t_edit_align_workspace(5, -1, 5, 1) == 0 and lib.s2t_edit_align_workspace(5, 5, -1, 0) == 0
    assert lib.s2t_edit_align_workspace(5, MAX_A + 1, 5, 0) == 0 and lib.s2t_edit_align_workspace(5, 5, MAX_B + 1, 0) == 0
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "s2t_hip.h")) as f:
        text = f.read()
    assert "#define S2T_EDIT_MAX_A %d" % MAX_A in text and "#define S2T_EDIT_MAX_B %d" % MAX_B in text
    assert (K.EDIT_MAX_A, K.EDIT_MAX_B) == (MAX_A, MAX_B) == (ER.MAX_HYP, ER.MAX_REF)


def check_refusals(fn):
    f = lambda **kw: fn(*[kw.get(k, d) for k, d in ARGS])
    for name in ("a", "a_len", "b", "b_len", "counts", "cost", "status"):
        assert f(**{name: None}) == -22, name                             # required pointers
    assert f(n_ops=None) == -22 and f(ws=None) == -22, "ops asks for n_ops and the workspace"
    assert f(collapse=1, a_n=None) == -22
    assert f(collapse=1, a_out=None, ops=None, ws=None) == -22, "the collapsed tokens need a place"
    for name in ("cs", "ca", "cb"):
        assert f(**{name: 0}) == -22 and f(**{name: 256}) == -22 and f(**{name: -1}) == -22, name
    assert f(Amax=-1) == -22 and f(Bmax=-1) == -22
    for name in ("a_elem", "b_elem"):
        assert f(**{name: 2}) == -22 and f(**{name: 0}) == -22 and f(**{name: 16}) == -22, name
    assert f(Amax=MAX_A + 1) == -95 and f(Bmax=MAX_B + 1) == -95
    assert f(B=0) == 0 and f(B=-3) == 0 and f(B=0, a=None, cs=0) == 0      # an empty problem: nothing to do, nothing looked at


def test_refusals_before_any_launch():
    check_refusals(L.load().s2t_edit_align)


def test_generated_binding_answers_like_ctypes():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        getattr(raw, name).argtypes = L.SIGNATURES[name]
    raw.s2t_edit_align_workspace.restype = ctypes.c_size_t
    check_refusals(fast.s2t_edit_align)
    check_refusals(raw.s2t_edit_align)
    for args in ((64, 375, 60, 1), (4096, MAX_A, MAX_B, 1), (0, 1, 1, 1), (7, 9, 33, 0)):
        assert fast.s2t_edit_align_workspace(*args) == raw.s2t_edit_align_workspace(*args) == (ws_bytes(*args) if args[0] else 0)
    assert fast.s2t_edit_align_workspace(4096, MAX_A, MAX_B, 1) > 1 << 32, "a size_t result, not an int"


def test_kernels_edit_align_checks_its_operands():
    a, n = torch.zeros(2, 5, dtype=torch.int32), torch.tensor([5, 5], dtype=torch.int32)
    b, m = torch.zeros(2, 3, dtype=torch.int64), torch.tensor([3, 3])
    for bad in (lambda: K.edit_align(a[0], n, b, m), lambda: K.edit_align(a, n, b[:1], m[:1]), lambda: K.edit_align(a.float(), n, b, m),
                lambda: K.edit_align(a, n.long(), b, m), lambda: K.edit_align(a, n, b, m.int()), lambda: K.edit_align(a, n[:1], b, m),
                lambda: K.edit_align(a, n, b, m, costs=(0, 1, 1)), lambda: K.edit_align(a, n, b, m, costs=(1, 256, 1)),
                lambda: K.edit_align(torch.zeros(2, MAX_A + 1, dtype=torch.int32), n, b, m),
                lambda: K.edit_align(a, n, torch.zeros(2, MAX_B + 1, dtype=torch.int64), m)):
        with pytest.raises(ValueError, match="edit_align"):
            bad()
    out = K.edit_align(a[:0], n[:0], b[:0], m[:0], want_ops=True)              # no sentences: nothing is launched
    assert tuple(out[0].shape) == (0, 4) and tuple(out[5].shape) == (0, 8) and out[4] is None


# ------------------------------------------------------------------ host logic on the Python reference
@pytest.fixture
def calls(monkeypatch):
    c = []

    def edit_align(a, a_len, b, b_len, costs=(1, 1, 1), collapse_blank=None, want_ops=False):
        assert a.dtype == a_len.dtype and b.dtype == b_len.dtype and a.dtype in (torch.int32, torch.int64)
        c.append((tuple(a.shape), tuple(b.shape), tuple(costs), collapse_blank, want_ops))
        out = R.edit_align_batch(a.numpy(), a_len.numpy(), b.numpy(), b_len.numpy(), costs, collapse_blank, want_ops)
        return tuple(None if x is None else torch.from_numpy(x) for x in out)
    monkeypatch.setattr(ER.K, "edit_align", edit_align)
    return c


HYP = [[4, 5, 6, 7, 0], [4, 4, 0, 0, 0], [0, 0, 0, 0, 0], [9, 8, 7, 6, 5]]
HYP_LEN = [4, 2, 0, 5]
REF = [[4, 6, 7, 1], [5, 4, 4, 1], [3, 3, 1, 1], [9, 7, 5, 1]]
REF_LEN = [3, 3, 2, 3]
KEYS = ["cost", "deletions", "errors", "insertions", "matches", "ref_len", "status", "substitutions"]


def test_score_fields_sums_and_result(calls):
    er = ER.ErrorRate()
    assert er.result() == dict(errors=0, substitutions=0, insertions=0, deletions=0, ref_tokens=0, sentences=0, error_rate=0.0,
                               accuracy=100.0)
    out = er.score(torch.tensor(HYP), torch.tensor(HYP_LEN), torch.tensor(REF), torch.tensor(REF_LEN))
    assert sorted(out) == KEYS and calls == [((4, 5), (4, 4), (1, 1, 1), None, False)]
    want = [R.align(h[:n], r[:m]) for h, n, r, m in zip(HYP, HYP_LEN, REF, REF_LEN)]
    assert out["matches"].tolist() == [w[1][0] for w in want] and out["substitutions"].tolist() == [w[1][1] for w in want]
    assert out["deletions"].tolist() == [w[1][2] for w in want] == [0, 1, 2, 0], "reference tokens left alone"
    assert out["insertions"].tolist() == [w[1][3] for w in want] == [1, 0, 0, 2], "hypothesis tokens left alone"
    assert out["errors"].tolist() == [1, 1, 2, 2] and out["cost"].tolist() == [1, 1, 2, 2] and out["status"].tolist() == [0] * 4
    assert out["ref_len"].tolist() == REF_LEN and out["ref_len"].dtype == torch.int64 and out["errors"].dtype == torch.int32
    res = er.result()
    assert res == dict(errors=6, substitutions=0, insertions=3, deletions=3, ref_tokens=11, sentences=4,
                       error_rate=100.0 * 6 / 11, accuracy=100.0 - 100.0 * 6 / 11)
    er.score(torch.tensor(HYP)[:2], torch.tensor(HYP_LEN)[:2], torch.tensor(REF)[:2], torch.tensor(REF_LEN)[:2])
    assert er.result()["errors"] == 8 and er.result()["ref_tokens"] == 17 and er.result()["sentences"] == 6, "calls add up"
    er.reset()
    assert er.result()["sentences"] == 0 and er.result()["error_rate"] == 0.0
    # more errors than reference tokens: the rate is not capped, the accuracy is
    er.score(torch.tensor([[1, 2, 3, 4, 5]]), torch.tensor([5]), torch.tensor([[9]]), torch.tensor([1]))
    assert er.result()["error_rate"] == 500.0 and er.result()["accuracy"] == 0.0


def test_refused_sentences_add_nothing(calls):
    er = ER.ErrorRate(costs=(4, 3, 3))
    out = er.score(torch.tensor(HYP, dtype=torch.int32), torch.tensor([4, 6, 0, -1]), torch.tensor(REF), torch.tensor(REF_LEN))
    assert out["status"].tolist() == [0, 2, 0, 2] and out["errors"].tolist() == [1, 0, 2, 0] and out["ref_len"].tolist() == [3, 0, 2, 0]
    assert er.result()["sentences"] == 2 and er.result()["ref_tokens"] == 5 and er.result()["errors"] == 3
    assert calls[0][2] == (4, 3, 3)


def test_ops_are_chunked_under_the_workspace_limit(calls, monkeypatch):
    rng = np.random.default_rng(0)
    hyp, ref = torch.from_numpy(rng.integers(0, 3, (7, 9))), torch.from_numpy(rng.integers(0, 3, (7, 6)))
    hl, rl = torch.from_numpy(rng.integers(0, 10, 7)), torch.from_numpy(rng.integers(0, 7, 7))
    whole = ER.ErrorRate((3, 2, 1)).score(hyp, hl, ref, rl, ops=True)
    assert len(calls) == 1 and sorted(whole) == sorted(KEYS + ["ops", "n_ops"]) and tuple(whole["ops"].shape) == (7, 15)
    per = 4 * 10 * 1 + 8 * 9 + 512
    assert ER.ErrorRate.chunk_sentences(9, 6) == (1 << 30) // per
    monkeypatch.setattr(ER, "WORKSPACE_LIMIT", 3 * per + 5)
    del calls[:]
    er = ER.ErrorRate((3, 2, 1))
    cut = er.score(hyp, hl, ref, rl, ops=True)
    assert [c[0][0] for c in calls] == [3, 3, 1] and all(c[4] for c in calls)
    for k in whole:
        assert torch.equal(whole[k], cut[k]), k
    assert er.result()["sentences"] == 7
    del calls[:]
    er.score(hyp, hl, ref, rl)
    assert len(calls) == 1, "without ops nothing grows with the matrix: one call"
    # the size a chunk asks for stays under the limit at the widest shapes
    monkeypatch.setattr(ER, "WORKSPACE_LIMIT", 1 << 30)
    n = ER.ErrorRate.chunk_sentences(MAX_A, MAX_B)
    assert n > 1 and ws_bytes(n, MAX_A, MAX_B, 1) < 1 << 30 <= ws_bytes(n + 2, MAX_A, MAX_B, 1)
    n = ER.ErrorRate.chunk_sentences(1500, 1024)
    assert ws_bytes(n, 1500, 1024, 1) < 1 << 30


def test_score_frames_and_reference_uer(calls):
    d = Dictionary.synthetic(4)
    d.add_symbol("<ctc_blank>")
    er = ER.ErrorRate.reference_uer(d)
    assert er.costs == (4, 3, 3) and er.blank == len(d) - 1
    with pytest.raises(ValueError, match="ctc_blank"):
        ER.ErrorRate.reference_uer(Dictionary.synthetic(4))
    blank = er.blank
    pred = torch.tensor([[5, 5, blank, 5, 6, 6, blank, blank], [blank] * 8, [4, 4, 4, 4, 5, 5, 5, 5]], dtype=torch.int32)
    out = er.score_frames(pred, torch.tensor([8, 8, 6]), torch.tensor([[5, 5, 6], [4, 1, 1], [4, 6, 1]]), torch.tensor([3, 1, 2]))
    assert calls == [((3, 8), (3, 3), (4, 3, 3), blank, False)]
    assert out["hyp_len"].tolist() == [3, 0, 2] and out["hyp"][0, :3].tolist() == [5, 5, 6] and out["hyp"][2, :2].tolist() == [4, 5]
    assert out["errors"].tolist() == [0, 1, 1] and out["cost"].tolist() == [0, 3, 4]
    assert er.result()["accuracy"] == 100.0 - 100.0 * 2 / 6
    with pytest.raises(ValueError, match="needs the blank"):
        ER.ErrorRate().score_frames(pred, torch.tensor([8, 8, 6]), torch.tensor([[5]] * 3), torch.tensor([1] * 3))


def test_score_hypotheses_takes_the_best_and_strips_eos(calls):
    EOS = 2
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    hypos = [[{"tokens": t(4, 5, 6, EOS)}, {"tokens": t(9, 9)}], [{"tokens": t(7, EOS)}], [], [{"tokens": t(EOS)}]]
    ref, ref_len = torch.tensor([[4, 5, 6, EOS], [7, 8, EOS, 1], [EOS, 1, 1, 1], [5, 1, 1, 1]]), torch.tensor([4, 3, 1, 1])
    er = ER.ErrorRate()
    out = er.score_hypotheses(hypos, ref, ref_len, strip_eos=EOS, ops=True)
    assert calls == [((4, 4), (4, 4), (1, 1, 1), None, True)]
    assert out["ref_len"].tolist() == [3, 2, 0, 1] and out["errors"].tolist() == [0, 1, 0, 1] and out["matches"].tolist() == [3, 1, 0, 0]
    assert out["n_ops"].tolist() == [3, 2, 0, 1] and out["ops"][1, :2].tolist() == [0, 2]
    kept = ER.ErrorRate().score_hypotheses(hypos, ref, ref_len)
    assert kept["ref_len"].tolist() == [4, 3, 1, 1] and kept["matches"].tolist() == [4, 2, 0, 0] and kept["errors"].tolist() == [0, 1, 1, 1]
    i32 = ER.ErrorRate().score_hypotheses([[{"tokens": h[0]["tokens"].int()}] if h else [] for h in hypos[:2]], ref[:2], ref_len[:2])
    assert i32["matches"].tolist() == [4, 2]
    none = ER.ErrorRate().score_hypotheses([[], []], ref[:2], ref_len[:2])
    assert none["deletions"].tolist() == [4, 3] and calls[-1][0] == (2, 0)
    with pytest.raises(ValueError, match="3 sentences of hypotheses, 4 references"):
        er.score_hypotheses(hypos[:3], ref, ref_len)


def test_value_errors(calls):
    er = ER.ErrorRate()
    ok, n1 = torch.zeros(1, 3).long(), torch.tensor([3])
    with pytest.raises(ValueError, match="S2T_EDIT_MAX_A"):
        er.score(torch.zeros(1, MAX_A + 1).long(), n1, ok, n1)
    with pytest.raises(ValueError, match="S2T_EDIT_MAX_B"):
        er.score(ok, n1, torch.zeros(1, MAX_B + 1).long(), n1)
    with pytest.raises(ValueError, match="one B"):
        er.score(ok, n1, torch.zeros(2, 3).long(), torch.tensor([3, 3]))
    for bad in ((0, 1, 1), (1, 1), (1, 1, 256)):
        with pytest.raises(ValueError, match="costs"):
            ER.ErrorRate(costs=bad)
    assert calls == [] and er.result()["sentences"] == 0, "nothing was aligned"
