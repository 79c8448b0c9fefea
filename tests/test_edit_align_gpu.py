"""The edit-distance kernels (csrc/edit_align.hip) and ErrorRate on the GPU against the rule in plain Python (tests/edit_ref.py).
Everything is an integer: every comparison is exact -- cost, the four counts, the path's length and, with `ops`, every step of the
path.  Small alphabets put ties everywhere; the tie order shows in the paths and under the asymmetric costs (3, 2, 1)
(tests/test_edit_ref_cpu.py counts how often), so every sweep compares paths and runs (1, 1, 1), (4, 3, 3) and (3, 2, 1).
Raw calls fill the outputs with sentinels first: what the rule calls "not written" must still hold them.  Rows are padded with junk
behind their lengths."""
import functools
import os

import numpy as np
import pytest
import torch

import edit_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
COSTS = ((1, 1, 1), (4, 3, 3), (3, 2, 1))
JUNK = (10 ** 12, -5, 2 ** 31)        # what pads the rows beyond their lengths (int32 rows: reduced to 32 bits)
S_INT, S_OP = -7, 0xEE                # sentinels of the int32 outputs and of ops
NP = {4: np.int32, 8: np.int64}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---------------------------------------------------------------------------------------------- calling the kernel
def padded(rows, width, elem, salt=0):
    out = np.empty((len(rows), width), np.int64)
    for s, r in enumerate(rows):
        out[s] = [JUNK[(s + i + salt) % 3] for i in range(width)]
        out[s, :len(r)] = r
    if elem == 4:
        out = ((out + 2 ** 31) % 2 ** 32 - 2 ** 31)
    return out.astype(NP[elem])


def call_raw(a, a_len, b, b_len, costs, collapse_blank=None, want_ops=False, a_out_in_ws=False):
    """s2t_edit_align on numpy operands and sentinel-filled outputs -> dict of numpy arrays"""
    from fbk_fairseq_st_amd import lib as L
    lib = L.load()
    B, Amax, Bmax = a.shape[0], a.shape[1], b.shape[1]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ta, tb = dev(a), dev(b)
    tal, tbl = dev(np.asarray(a_len, a.dtype)), dev(np.asarray(b_len, b.dtype))
    full = lambda shape, v, dt=torch.int32: torch.full(shape, v, dtype=dt, device=DEV)
    counts, cost, status, a_n, n_ops = full((B, 4), S_INT), full((B,), S_INT), full((B,), S_INT), full((B,), S_INT), full((B,), S_INT)
    collapse = collapse_blank is not None
    a_out = full((B, max(Amax, 1)), S_INT, ta.dtype) if collapse and not a_out_in_ws else None
    ops = full((B, max(Amax + Bmax, 1)), S_OP, torch.uint8) if want_ops else None
    ws = torch.empty((max(int(lib.s2t_edit_align_workspace(B, Amax, Bmax, int(want_ops))), 256),), dtype=torch.uint8, device=DEV)
    pad = torch.zeros((2,), dtype=torch.int64, device=DEV)
    p = lambda t: L.ptr(t if t.numel() else pad)
    L.check(lib.s2t_edit_align(p(ta), L.ptr(tal), a.dtype.itemsize, p(tb), L.ptr(tbl), b.dtype.itemsize, B, Amax, Bmax, costs[0], costs[1],
                               costs[2], int(collapse), int(collapse_blank) if collapse else 0, L.ptr(ws), L.ptr(counts), L.ptr(cost),
                               L.ptr(status), L.ptr(a_n), L.ptr(a_out), L.ptr(ops), L.ptr(n_ops) if want_ops else 0, L.stream()),
            "s2t_edit_align")
    torch.cuda.synchronize()
    out = dict(counts=counts, cost=cost, status=status, a_n=a_n, n_ops=n_ops, a_out=a_out, ops=ops)
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def _reference(key):
    a, b, costs = _REGISTRY[key]
    return R.align_np(a, b, costs)


_REGISTRY = {}


def ref_of(a, b, costs):
    """the rule for a pair, computed once per process"""
    key = (tuple(int(x) for x in a), tuple(int(x) for x in b), tuple(costs))
    _REGISTRY[key] = (key[0], key[1], key[2])
    return _reference(key)


def differs(got, want):
    """THE comparison of this file: (cost, counts, ops) against the rule's, None when equal"""
    if int(got[0]) != want[0]:
        return "cost %d, the rule gives %d" % (got[0], want[0])
    if tuple(int(x) for x in got[1]) != tuple(want[1]):
        return "counts %s, the rule gives %s" % (tuple(got[1]), want[1])
    if got[2] is not None and [int(x) for x in got[2]] != list(want[2]):
        return "the path differs from the rule's"
    return None


def check_batch(pairs, costs, Amax, Bmax, elems=(4, 8), what=""):
    """aligns the pairs in one call with ops and one without; every sentence against the rule, every unwritten entry a sentinel"""
    a = padded([p[0] for p in pairs], Amax, elems[0])
    b = padded([p[1] for p in pairs], Bmax, elems[1], salt=1)
    a_len, b_len = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    with_ops = call_raw(a, a_len, b, b_len, costs, want_ops=True)
    plain = call_raw(a, a_len, b, b_len, costs)
    assert plain["ops"] is None and (plain["n_ops"] == S_INT).all()
    for s, (x, y) in enumerate(pairs):
        want = ref_of(x, y, costs)
        for name, out in (("ops", with_ops), ("plain", plain)):
            assert out["status"][s] == 0 and out["a_n"][s] == len(x), (what, name, s)
            path = None
            if name == "ops":
                assert out["n_ops"][s] == len(want[2]), (what, s, len(x), len(y), out["n_ops"][s], len(want[2]))
                path = out["ops"][s, :len(want[2])]
                assert (out["ops"][s, len(want[2]):] == S_OP).all(), (what, s, "entries behind the path were written")
            bad = differs((out["cost"][s], out["counts"][s], path), want)
            assert bad is None, (what, name, costs, "sentence %d: n = %d, m = %d" % (s, len(x), len(y)), bad)


def draw(rng, n, m, k, identical=False):
    x = rng.integers(0, k, n).tolist()
    return (x, list(x[:m]) + rng.integers(0, k, max(m - n, 0)).tolist()) if identical else (x, rng.integers(0, k, m).tolist())


# the rows around the 64-row blocks of the backward walk (16 and 32 rows at the two widest widths), both n > m and n < m
N_SMALL = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
# around every columns-per-lane switch of the register form, and its last width
REGISTER_WIDTHS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129, 254, 255, 256, 257, 510, 511, 512, 513, 1022, 1023)
WORKGROUP_WIDTHS = (1024, 1025, 2047, 4095)


def sweep_cases(Bmax, seed):
    """pairs for one padded width: full-width, one-short and short references against every row count"""
    rng = np.random.default_rng(seed)
    pairs = []
    for q, n in enumerate(N_SMALL):
        m = (Bmax, max(Bmax - 1, 0), int(rng.integers(0, Bmax + 1)), min(Bmax, 3))[q % 4]
        pairs.append(draw(rng, n, m, (2, 3, 6)[q % 3]))
    pairs.append(draw(rng, min(Bmax, 150), Bmax, 3, identical=True))
    pairs.append(draw(rng, 90, min(Bmax, 90), 2, identical=True))
    return pairs


@pytest.mark.parametrize("costs", COSTS, ids=lambda c: "%d-%d-%d" % c)
def test_register_form_sweep(costs):
    for w, Bmax in enumerate(REGISTER_WIDTHS):
        check_batch(sweep_cases(Bmax, 100 + w), costs, Amax=max(N_SMALL), Bmax=Bmax, elems=((4, 8), (8, 4))[w % 2], what="Bmax %d" % Bmax)


@pytest.mark.parametrize("costs", COSTS, ids=lambda c: "%d-%d-%d" % c)
def test_workgroup_form_sweep(costs):
    for w, Bmax in enumerate(WORKGROUP_WIDTHS):
        rng = np.random.default_rng(200 + w)
        pairs = [draw(rng, n, m, k) for n, m, k in ((0, Bmax, 2), (1, Bmax, 3), (16, Bmax - 1, 2), (17, Bmax, 6), (33, min(Bmax, 1025), 3),
                                                    (65, Bmax, 2), (130, Bmax, 3), (64, 0, 2), (129, 5, 3))]
        pairs.append(draw(rng, 130, Bmax, 6, identical=True))
        check_batch(pairs, costs, Amax=130, Bmax=Bmax, what="Bmax %d" % Bmax)


@pytest.mark.parametrize("Bmax", (1000, 1024))
def test_long_hypotheses(Bmax):
    """1,500 rows in both forms, n > m"""
    rng = np.random.default_rng(7)
    pairs = [draw(rng, 1500, Bmax, 3), draw(rng, 1499, Bmax - 7, 2), draw(rng, 1500, 40, 6), draw(rng, 1500, 1000, 3, identical=True)]
    check_batch(pairs, (4, 3, 3), Amax=1500, Bmax=Bmax, what="Bmax %d" % Bmax)


def test_widest_operands():
    """the limits of both widths in one call: 32,767 rows, 4,095 columns"""
    rng = np.random.default_rng(8)
    pairs = [draw(rng, 300, 4095, 3), draw(rng, 32767, 20, 3)]
    check_batch(pairs, (3, 2, 1), Amax=32767, Bmax=4095, what="limits")


# ---------------------------------------------------------------------------------------------- planted alignments
def planted(rng, m, edits):
    """a reference of m distinct tokens and a hypothesis made from it by `edits` isolated operations (at least two kept tokens
    between any two of them: with one, a deletion and an insertion tie with two substitutions): under (1, 1, 1) the one cheapest
    alignment makes exactly these operations"""
    ref = (1000 + rng.permutation(m)).tolist()
    where = sorted(rng.choice(np.arange(1, m - 1, 3), edits, replace=False).tolist())
    kinds = rng.integers(0, 3, edits).tolist()
    hyp, new = [], 10 ** 6
    plan = dict(zip(where, kinds))
    for j, tok in enumerate(ref):
        kind = plan.get(j)
        if kind == 0:                       # substitution
            hyp.append(new)
        elif kind == 1:                     # deletion: the reference token has no partner
            pass
        elif kind == 2:                     # insertion in front of a kept token
            hyp += [new, tok]
        else:
            hyp.append(tok)
        new += 1
    return hyp, ref, (kinds.count(0), kinds.count(2), kinds.count(1))


def test_planted_alignments():
    from fbk_fairseq_st_amd import error_rate as ER
    rng = np.random.default_rng(11)
    cases = [planted(rng, m, e) for m, e in ((40, 5), (64, 9), (129, 20), (300, 60), (700, 3), (1023, 100), (1500, 200), (12, 0))]
    Hmax, Rmax = max(len(c[0]) for c in cases), max(len(c[1]) for c in cases)
    hyp, ref = padded([c[0] for c in cases], Hmax, 8), padded([c[1] for c in cases], Rmax, 8, salt=2)
    er = ER.ErrorRate()
    out = er.score(torch.from_numpy(hyp).to(DEV), torch.tensor([len(c[0]) for c in cases], device=DEV), torch.from_numpy(ref).to(DEV),
                   torch.tensor([len(c[1]) for c in cases], device=DEV), ops=True)
    host = {k: v.cpu().numpy() for k, v in out.items()}
    for s, (h, r, (subs, ins, dele)) in enumerate(cases):
        assert host["errors"][s] == subs + ins + dele == host["cost"][s], (s, host["errors"][s], subs + ins + dele)
        assert (host["substitutions"][s], host["insertions"][s], host["deletions"][s]) == (subs, ins, dele), s
        assert host["matches"][s] == len(r) - subs - dele and host["status"][s] == 0
        path = host["ops"][s, :host["n_ops"][s]].tolist()
        assert R.replay(h, r, path) and len(path) == host["matches"][s] + subs + ins + dele, (s, "ops do not replay a into b")
    assert er.result()["errors"] == sum(sum(c[2]) for c in cases) and er.result()["ref_tokens"] == sum(len(c[1]) for c in cases)


# ---------------------------------------------------------------------------------------------- padding, dtypes, refusals
@pytest.mark.parametrize("elems", ((4, 4), (4, 8), (8, 4), (8, 8)), ids=lambda e: "a%d-b%d" % e)
def test_ragged_batches_sentinels_and_refusals(elems):
    rng = np.random.default_rng(13)
    Amax, Bmax = 70, 37
    pairs = [draw(rng, n, m, 3) for n, m in ((70, 37), (0, 0), (1, 37), (70, 1), (33, 16), (5, 17), (64, 32), (0, 9), (9, 0))]
    a, b = padded([p[0] for p in pairs], Amax, elems[0]), padded([p[1] for p in pairs], Bmax, elems[1], salt=1)
    a_len, b_len = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    refused = {1: (-1, 0), 4: (Amax + 1, 3), 6: (3, Bmax + 1), 7: (2, -4)}           # beside ordinary sentences
    for s, (n, m) in refused.items():
        a_len[s], b_len[s] = n, m
    for costs in COSTS:
        out = call_raw(a, a_len, b, b_len, costs, want_ops=True)
        for s, (x, y) in enumerate(pairs):
            if s in refused:
                assert out["status"][s] == 2, s
                for k in ("counts", "cost", "a_n", "n_ops"):
                    assert (out[k][s] == S_INT).all(), (s, k, "a refused sentence gets its status and nothing else")
                assert (out["ops"][s] == S_OP).all()
                continue
            want = ref_of(x, y, costs)
            path = out["ops"][s, :len(want[2])]
            assert out["status"][s] == 0 and out["n_ops"][s] == len(want[2]) and out["a_n"][s] == len(x)
            assert differs((out["cost"][s], out["counts"][s], path), want) is None, (s, costs)
            assert (out["ops"][s, len(want[2]):] == S_OP).all()


# ---------------------------------------------------------------------------------------------- collapse mode
def frames_case(seed, B, T, V, blank):
    """frame labels with long runs and many blanks; in_len of 0 and of T among them"""
    rng = np.random.default_rng(seed)
    pred = np.empty((B, T), np.int32)
    for s in range(B):
        t = 0
        while t < T:
            run = int(rng.integers(1, 9))
            pred[s, t:t + run] = blank if rng.random() < 0.4 else rng.integers(0, V)
            t += run
    in_len = rng.integers(0, T + 1, B)
    in_len[0], in_len[1] = 0, T
    tgt_len = rng.integers(0, 25, B)
    tgt = rng.integers(0, V, (B, 24))
    return pred, in_len.astype(np.int64), tgt.astype(np.int64), tgt_len.astype(np.int64)


@pytest.mark.parametrize("T", (50, 64, 200))
def test_collapse_mode_equals_the_host_pass(T):
    from fbk_fairseq_st_amd import kernels as K
    blank = 4
    pred, in_len, tgt, tgt_len = frames_case(17 + T, 12, T, 6, blank)
    e_host, n_host = K.host_ctc_uer(torch.from_numpy(pred), torch.from_numpy(in_len), torch.from_numpy(tgt), torch.from_numpy(tgt_len), blank)
    for in_ws in (False, True):
        out = call_raw(pred, in_len, tgt, tgt_len, (4, 3, 3), collapse_blank=blank, a_out_in_ws=in_ws)
        assert (out["status"] == 0).all()
        assert float(out["counts"][:, 1:].sum()) == e_host and float(tgt_len.sum()) == n_host
        for s in range(pred.shape[0]):
            hyp = R.collapse(pred[s, :in_len[s]], blank)
            assert out["a_n"][s] == len(hyp), s
            if not in_ws:
                assert out["a_out"][s, :len(hyp)].tolist() == hyp and (out["a_out"][s, len(hyp):] == S_INT).all(), s
            assert differs((out["cost"][s], out["counts"][s], None), ref_of(hyp, tgt[s, :tgt_len[s]], (4, 3, 3))) is None, s
    # int64 frames, other costs, the path as well
    out = call_raw(pred.astype(np.int64), in_len, tgt.astype(np.int32), tgt_len, (3, 2, 1), collapse_blank=blank, want_ops=True)
    for s in range(pred.shape[0]):
        want = ref_of(R.collapse(pred[s, :in_len[s]], blank), tgt[s, :tgt_len[s]], (3, 2, 1))
        assert differs((out["cost"][s], out["counts"][s], out["ops"][s, :out["n_ops"][s]]), want) is None, s


def test_collapse_mode_reproduces_the_reference_uer_counts():
    """tests/golden/ctc_uer.npz: `errors` and `total` of the reference's compute_ctc_uer on these log-probabilities"""
    from fbk_fairseq_st_amd import error_rate as ER
    g = dict(np.load(os.path.join(GOLDEN, "ctc_uer.npz")))
    pred = torch.from_numpy(g["lp"].argmax(-1).astype(np.int32)).to(DEV)
    er = ER.ErrorRate(costs=(4, 3, 3), blank=int(g["blank"]))
    er.score_frames(pred, torch.from_numpy(g["in_len"]).to(DEV), torch.from_numpy(g["tgt"]).to(DEV), torch.from_numpy(g["tgt_len"]).to(DEV))
    res = er.result()
    assert (float(res["errors"]), float(res["ref_tokens"])) == (float(g["errors"]), float(g["total"]))
    assert res["accuracy"] == 100.0 - min(100.0 * float(g["errors"]) / float(g["total"]), 100.0)


# ---------------------------------------------------------------------------------------------- batch independence
@pytest.mark.parametrize("Bmax", (60, 300, 1100))
def test_a_sentence_alone_and_inside_a_batch(Bmax):
    rng = np.random.default_rng(19)
    Amax = 140
    pairs = [draw(rng, int(rng.integers(0, Amax + 1)), int(rng.integers(0, Bmax + 1)), 3) for _ in range(64)]
    pairs[5], pairs[63] = draw(rng, Amax, Bmax, 2), draw(rng, 129, Bmax - 1, 3)
    a, b = padded([p[0] for p in pairs], Amax, 4), padded([p[1] for p in pairs], Bmax, 8, salt=1)
    a_len, b_len = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    for want_ops in (False, True):
        batch = call_raw(a, a_len, b, b_len, (4, 3, 3), want_ops=want_ops)
        for s in (0, 5, 31, 63):
            alone = call_raw(a[s:s + 1], a_len[s:s + 1], b[s:s + 1], b_len[s:s + 1], (4, 3, 3), want_ops=want_ops)
            for k in ("counts", "cost", "status", "a_n", "n_ops") + (("ops",) if want_ops else ()):
                assert np.array_equal(alone[k][0], batch[k][s]), (Bmax, want_ops, s, k)
            assert differs((alone["cost"][0], alone["counts"][0], None), ref_of(pairs[s][0], pairs[s][1], (4, 3, 3))) is None


# ---------------------------------------------------------------------------------------------- end to end
def test_error_rate_end_to_end(monkeypatch):
    from fbk_fairseq_st_amd import ctc_decoder as CD
    from fbk_fairseq_st_amd import error_rate as ER
    from fbk_fairseq_st_amd import kernels as K
    from fbk_fairseq_st_amd.data import Dictionary
    d = Dictionary.synthetic(7)
    d.add_symbol("<ctc_blank>")
    V, T, B = len(d), 90, 9
    g = torch.Generator().manual_seed(3)
    logits = (torch.randn(T, B, V, generator=g) * 2).to(DEV)
    logits[..., V - 1] += 1.5                                                        # blanks between the tokens
    in_len = torch.tensor([T, 0, 1, 64, 65, 33, T, 17, 80], dtype=torch.int32, device=DEV)
    ref = torch.randint(4, V - 1, (B, 30), generator=g).to(DEV)
    ref_len = torch.tensor([30, 0, 3, 12, 29, 1, 30, 7, 22], device=DEV)
    hypos = CD.CTCDecoder(d, strategy="greedy").decode_logits(logits, in_len)
    pred, _ = K.ctc_argmax(logits)
    by_hyp, by_frames = ER.ErrorRate.reference_uer(d), ER.ErrorRate.reference_uer(d)
    one = by_hyp.score_hypotheses(hypos, ref, ref_len, ops=True)
    two = by_frames.score_frames(pred, in_len, ref, ref_len)
    for k in ("matches", "substitutions", "insertions", "deletions", "errors", "cost", "ref_len", "status"):
        assert torch.equal(one[k], two[k]), k
    assert two["hyp_len"].tolist() == [len(h[0]["tokens"]) for h in hypos]
    e_host, n_host = K.host_ctc_uer(pred.cpu(), in_len.long().cpu(), ref.cpu(), ref_len.cpu(), by_hyp.blank)
    res = by_frames.result()
    assert (float(res["errors"]), float(res["ref_tokens"]), res["sentences"]) == (e_host, n_host, B)
    assert res["errors"] == res["substitutions"] + res["insertions"] + res["deletions"] and res == by_hyp.result()
    assert res["error_rate"] == 100.0 * e_host / n_host and res["accuracy"] == 100.0 - min(res["error_rate"], 100.0)
    by_frames.score_frames(pred, in_len, ref, ref_len)                               # a second call adds up
    twice = by_frames.result()
    assert twice["errors"] == 2 * res["errors"] and twice["sentences"] == 2 * B and twice["error_rate"] == res["error_rate"]
    by_frames.reset()
    assert by_frames.result()["sentences"] == 0 and by_frames.result()["errors"] == 0
    # the chunked call with ops equals the unchunked one
    monkeypatch.setattr(ER, "WORKSPACE_LIMIT", 4 * (4 * (T + 1) * 2 + 8 * T + 512))
    cut = ER.ErrorRate.reference_uer(d)
    assert ER.ErrorRate.chunk_sentences(one["ops"].shape[1] - 30, 30) < B
    parts = cut.score_hypotheses(hypos, ref, ref_len, ops=True)
    n_ops = one["n_ops"].tolist()
    for k in one:
        if k != "ops":
            assert torch.equal(one[k], parts[k]), k
    for s in range(B):
        assert torch.equal(one["ops"][s, :n_ops[s]], parts["ops"][s, :n_ops[s]]), s
        hyp = hypos[s][0]["tokens"].tolist()
        assert R.replay(hyp, ref[s, :int(ref_len[s])].tolist(), one["ops"][s, :n_ops[s]].tolist()), s
    assert cut.result() == res


# ---------------------------------------------------------------------------------------------- sensitivity
def test_every_wrong_twin_fails_this_files_comparison():
    """the comparison the sweeps make, on the sweeps' own cases, fed each twin's answer in place of the kernel's"""
    cases = [p for w in (62, 64, 129) for p in sweep_cases(w, 100 + REGISTER_WIDTHS.index(w))]
    caught = {name: [] for name in R.TWINS}
    for name, twin in R.TWINS.items():
        for costs in COSTS:
            for x, y in cases:
                cost, counts, ops = twin(x, y, costs)
                full = differs((cost, counts, ops), ref_of(x, y, costs))
                plain = differs((cost, counts, None), ref_of(x, y, costs))
                if full is not None:
                    caught[name].append((costs, plain is not None))
    for name, hits in caught.items():
        assert hits, "no case of the sweep tells the rule from its twin: " + name
    # the tie order: seen in the paths under every cost set, and in the counts alone under the asymmetric one
    assert {c for c, _ in caught["up before left"]} == set(COSTS)
    assert any(plain for c, plain in caught["up before left"] if c == (3, 2, 1))
    assert any(plain for _, plain in caught["non-strict comparisons"]) and any(plain for _, plain in caught["ca and cb swapped"])
    assert any(plain for c, plain in caught["counts of a Levenshtein path"] if c == (4, 3, 3))
