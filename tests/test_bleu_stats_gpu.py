"""The BLEU statistics kernel (csrc/bleu_stats.hip) and BleuScorer on the GPU against the rule in plain Python (tests/bleu_ref.py).
The statistics are integers: every comparison of them is exact.  Small alphabets make n-grams repeat on both sides, so the clipping
decides most rows.  Raw calls fill the outputs with sentinels first, and rows are padded behind their lengths with junk that is the
same on both sides: a kernel that read past a length would find matches there.  Hypothesis widths sit on both sides of the
wave / workgroup switch (64), of the switch between 256 and 1,024 threads (256) and of every further 1,024 positions a thread
takes; both staging widths (32-bit when both sides are int32, 64-bit otherwise) run everywhere, and both limits in one call."""
import os

import numpy as np
import pytest
import torch

import bleu_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, EOS, UNK = 1, 2, 3
S_INT = -7                            # sentinel of the int32 outputs
NP = {4: np.int32, 8: np.int64}
ELEMS = ((4, 4), (4, 8), (8, 4), (8, 8))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleu_stats.npz")
_WANT = {}


# ---------------------------------------------------------------------------------------------- calling the kernel
def padded(rows, width, elem):
    """rows behind their lengths: ordinary symbols, the same on both sides"""
    out = np.empty((len(rows), width), NP[elem])
    for s, r in enumerate(rows):
        out[s] = [(4, 5, 4, 4, 5, 6)[(s + i) % 6] for i in range(width)]
        out[s, :len(r)] = r
    return out


def call_raw(hyp, hyp_len, ref, ref_len, pad=PAD, eos=EOS, unk=UNK, ref_row=None):
    """s2t_bleu_stats on numpy operands and sentinel-filled outputs -> (stats, status) as numpy"""
    from fbk_fairseq_st_amd import lib as L
    lib = L.load()
    B, Hmax, Rrows, Rmax = hyp.shape[0], hyp.shape[1], ref.shape[0], ref.shape[1]
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    th, tr = dev(hyp), dev(ref)
    thl, trl = dev(np.asarray(hyp_len, hyp.dtype)), dev(np.asarray(ref_len, ref.dtype))
    rows = None if ref_row is None else dev(np.asarray(ref_row, np.int32))
    stats = torch.full((B, 10), S_INT, dtype=torch.int32, device=DEV)
    status = torch.full((B,), S_INT, dtype=torch.int32, device=DEV)
    fill = torch.zeros((2,), dtype=torch.int64, device=DEV)
    p = lambda t: L.ptr(t if t.numel() else fill)
    L.check(lib.s2t_bleu_stats(p(th), L.ptr(thl), hyp.dtype.itemsize, p(tr), L.ptr(trl), ref.dtype.itemsize, L.ptr(rows), B, Hmax, Rmax, Rrows,
                               pad, eos, unk, L.ptr(stats), L.ptr(status), L.stream()), "s2t_bleu_stats")
    torch.cuda.synchronize()
    return stats.cpu().numpy(), status.cpu().numpy()


def ref_of(h, r, unk=UNK):
    """the rule for a pair (the Counter form), computed once per process"""
    key = (tuple(int(x) for x in h), tuple(int(x) for x in r), unk)
    if key not in _WANT:
        _WANT[key] = R.stats_counter(key[0], key[1], PAD, EOS, unk)
    return _WANT[key]


def differs(got, want):
    """THE comparison of this file: ten integers against the rule's, None when equal"""
    got = [int(x) for x in got]
    if got[:2] != list(want[:2]):
        return "lengths (ref, hyp) %s, the rule gives %s" % (got[:2], list(want[:2]))
    if got[3::2] != list(want[3::2]):
        return "counts %s, the rule gives %s" % (got[3::2], list(want[3::2]))
    if got[2::2] != list(want[2::2]):
        return "matches %s, the rule gives %s" % (got[2::2], list(want[2::2]))
    return None


def check_batch(pairs, Hmax=None, Rmax=None, elems=ELEMS, unk=UNK, what=""):
    """scores the pairs in one call per dtype combination; every sentence against the rule"""
    Hmax = max(len(p[0]) for p in pairs) if Hmax is None else Hmax
    Rmax = max(len(p[1]) for p in pairs) if Rmax is None else Rmax
    for he, re in elems:
        stats, status = call_raw(padded([p[0] for p in pairs], Hmax, he), [len(p[0]) for p in pairs],
                                 padded([p[1] for p in pairs], Rmax, re), [len(p[1]) for p in pairs], unk=unk)
        for s, (h, r) in enumerate(pairs):
            assert status[s] == 0, (what, he, re, s)
            bad = differs(stats[s], ref_of(h, r, unk))
            assert bad is None, (what, "hyp int%d, ref int%d" % (8 * he, 8 * re), "sentence %d: %d and %d tokens" % (s, len(h), len(r)), bad)


def draw(rng, n, m, k, lo=4):
    return (lo + rng.integers(0, k, n)).tolist(), (lo + rng.integers(0, k, m)).tolist()


# ---------------------------------------------------------------------------------------------- the reference's numbers
@pytest.mark.parametrize("elems", ELEMS, ids=lambda e: "h%d-r%d" % e)
def test_fixture_rows(elems):
    g = dict(np.load(GOLDEN))
    for Hmax in (g["hyp"].shape[1], 70):                                 # the wave form and the workgroup form
        hyp = np.full((len(g["hyp"]), Hmax), 4, NP[elems[0]])
        hyp[:, :g["hyp"].shape[1]] = g["hyp"]
        stats, status = call_raw(hyp, g["hyp_len"], g["ref"].astype(NP[elems[1]]), g["ref_len"], int(g["pad"]), int(g["eos"]), int(g["unk"]))
        assert (status == 0).all()
        wrong = [s for s in range(len(stats)) if stats[s].tolist() != g["stats"][s].tolist()]
        assert not wrong, (Hmax, wrong[:5], stats[wrong[0]].tolist(), g["stats"][wrong[0]].tolist())


# ---------------------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("Hmax", (6, 65))
def test_every_length_up_to_six(Hmax):
    """0 to 6 tokens on both sides in every combination: the borders of the four orders, and the reference's end in the last windows"""
    rng = np.random.default_rng(1)
    pairs = [draw(rng, n, m, 2) for n in range(7) for m in range(7)]
    pairs += [([4] * n, [4] * m) for n in range(7) for m in range(7)]
    check_batch(pairs, Hmax=Hmax, Rmax=6, what="Hmax %d" % Hmax)
    # with pad and eos among the symbols: the trim decides the lengths
    pairs = [draw(rng, n, m, 4, lo=1) for n in range(7) for m in range(7) for _ in range(2)]
    check_batch(pairs, Hmax=Hmax, Rmax=6, unk=-1, what="trimmed, Hmax %d" % Hmax)
    check_batch(pairs, Hmax=Hmax, Rmax=6, unk=UNK, elems=((4, 4), (8, 8)), what="trimmed with unk, Hmax %d" % Hmax)


# the wave / workgroup switch (64), the 256 / 1,024 thread switch (256), one pass of the 1,024 threads, and the second and third
LENGTHS = (61, 63, 64, 65, 67, 127, 129, 255, 256, 257, 259, 511, 513, 1023, 1024, 1025, 1027, 2047, 2048, 2049, 2051)


@pytest.mark.parametrize("k", (2, 3))
def test_lengths_around_every_switch(k):
    rng = np.random.default_rng(2 + k)
    pairs = []
    for q, n in enumerate(LENGTHS):
        m = (n, LENGTHS[(q + 5) % len(LENGTHS)], n - 1, 3, n + 2)[q % 5]
        pairs.append(draw(rng, n, m, k))
    for Hmax in (64, 65, 256, 257, 1024, 1025, 2051):
        some = [p for p in pairs if len(p[0]) <= Hmax][-6:]
        check_batch(some, Hmax=Hmax, elems=((4, 4), (8, 4)) if Hmax % 2 else ((8, 8), (4, 8)), what="k %d, Hmax %d" % (k, Hmax))


def test_trim_across_the_chunks_of_the_scan():
    """leading pads and trailing eos / pads that cross the 64-, 256- and 1,024-token chunks the ballots take"""
    rng = np.random.default_rng(4)
    pairs = []
    for lead, body, trail in ((0, 5, 300), (63, 3, 64), (64, 70, 1), (255, 2, 255), (256, 1, 0), (300, 130, 257), (511, 1, 3), (1, 0, 600),
                              (1023, 2, 1), (1100, 3, 1030), (3, 1024, 70)):
        for side in range(2):
            toks = [PAD] * lead + draw(rng, body, 0, 2)[0] + [(EOS, PAD)[int(rng.integers(0, 2))] for _ in range(trail)]
            other = draw(rng, 40, 0, 2)[0] + [EOS]
            pairs.append((toks, other) if side == 0 else (other, toks))
    pairs += [([PAD] * 400, [4, 5, EOS]), ([4, 5, EOS], [PAD] * 400), ([EOS] * 400, [EOS]), ([PAD] * 399 + [EOS], [EOS] * 2)]
    assert ref_of(*pairs[-1])[:4] == [1, 1, 1, 1] and ref_of(*pairs[-4])[:2] == [2, 0]
    check_batch(pairs, elems=((4, 4), (8, 8)), what="trim")
    check_batch([p for p in pairs if len(p[0]) <= 256], Hmax=256, elems=((4, 4), (8, 8)), what="trim, 256 threads")
    check_batch([p for p in pairs if len(p[0]) <= 64], Hmax=64, elems=((4, 4), (8, 8)), what="trim, wave form")


@pytest.mark.parametrize("elems", ((4, 4), (8, 8)), ids=lambda e: "h%d-r%d" % e)
def test_both_limits(elems):
    """4,095 x 4,095 and 4,095 x 1 (and 1 x 4,095) in one call; 64-bit tokens at both limits take more than 64 KiB of LDS"""
    rng = np.random.default_rng(5)
    h, r = draw(rng, 4095, 4095, 2)
    pairs = [(h, r), (draw(rng, 4095, 0, 3)[0], [5]), ([5], draw(rng, 4095, 0, 3)[0])]
    check_batch(pairs, Hmax=4095, Rmax=4095, elems=(elems,), what="limits")


# ---------------------------------------------------------------------------------------------- contents
def test_identical_disjoint_and_repeated():
    rng = np.random.default_rng(6)
    pairs = []
    for n in (1, 3, 4, 5, 64, 65, 300):
        x = draw(rng, n, 0, 3)[0]
        pairs += [(x, list(x)), (x, [t + 10 for t in x]), ([4] * n, x), (x, [4] * n), ([4] * n, [4] * max(n // 2, 1)), ([4] * max(n // 2, 1), [4] * n)]
    assert ref_of(*pairs[-6 + 0])[2::2] == [300, 299, 298, 297] and ref_of(*pairs[-6 + 1])[2::2] == [0, 0, 0, 0]
    assert ref_of(*pairs[-2])[2::2] == [150, 149, 148, 147], "a run against a shorter run: clipped by the reference"
    check_batch(pairs, what="contents")
    check_batch([p for p in pairs if len(p[0]) <= 64], Hmax=64, what="contents, wave form")


def test_unk_and_64_bit_tokens():
    rng = np.random.default_rng(7)
    pairs = []
    for n in (5, 30, 64, 90):
        h, r = draw(rng, n, n, 2)
        for s in (h, r):
            for at in rng.integers(0, n, max(n // 4, 1)):
                s[int(at)] = UNK
        pairs += [(h, r), (h, list(h)), ([UNK] * n, [UNK] * n)]
    for unk in (UNK, -1, 5):
        check_batch(pairs, unk=unk, what="unk %d" % unk)
    # tokens that agree in their low 32 bits are different tokens; negative ones are ordinary
    big = [(4 + (int(t) << 32) if i % 2 else 4) for i, t in enumerate(rng.integers(0, 2, 80))]
    low = [4] * 80
    neg = [-(int(t) + 1) for t in rng.integers(0, 2, 80)]
    pairs = [(big, low), (low, big), (big, list(big)), (neg, list(reversed(neg))), (neg[:40], [t + (1 << 32) for t in neg])]
    assert ref_of(*pairs[0])[2] < 80 == ref_of(*pairs[2])[2]
    check_batch(pairs, elems=((8, 8),), what="64-bit tokens")
    check_batch([(p[0][:64], p[1]) for p in pairs], Hmax=64, elems=((8, 8),), what="64-bit tokens, wave form")
    check_batch([(neg, low), (low, neg)], elems=((4, 8), (8, 4), (4, 4)), what="negative tokens of either width")


# ---------------------------------------------------------------------------------------------- padding, dtypes, refusals
@pytest.mark.parametrize("elems", ELEMS, ids=lambda e: "h%d-r%d" % e)
def test_ragged_batches_sentinels_and_refusals(elems):
    rng = np.random.default_rng(13)
    for Hmax, Rmax in ((40, 37), (70, 37), (300, 80)):
        pairs = [draw(rng, n, m, 2) for n, m in ((Hmax, Rmax), (0, 0), (1, Rmax), (Hmax, 1), (33, 16), (5, 17), (Hmax - 1, 32), (0, 9), (9, 0))]
        hyp, ref = padded([p[0] for p in pairs], Hmax, elems[0]), padded([p[1] for p in pairs], Rmax, elems[1])
        hyp_len, ref_len = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
        row = list(range(len(pairs)))
        refused = {1: (-1, 0), 4: (Hmax + 1, 3), 6: (3, Rmax + 1), 7: (2, -4)}           # beside ordinary sentences
        for s, (n, m) in refused.items():
            hyp_len[s], ref_len[s] = n, m
        for use_map in (False, True):
            if use_map:
                row[2], refused[2] = len(pairs), None                                   # a reference row that does not exist
                row[8], refused[8] = -1, None
            stats, status = call_raw(hyp, hyp_len, ref, ref_len, ref_row=row if use_map else None)
            for s, (h, r) in enumerate(pairs):
                if s in refused:
                    assert status[s] == 2 and (stats[s] == 0).all(), (Hmax, s, "a refused sentence gets status 2 and zeros")
                else:
                    assert status[s] == 0 and differs(stats[s], ref_of(h, r)) is None, (Hmax, s, differs(stats[s], ref_of(h, r)))
    assert S_INT not in stats and S_INT not in status, "every output is written"


@pytest.mark.parametrize("Hmax", (50, 140, 300))
def test_a_sentence_alone_and_inside_a_batch(Hmax):
    rng = np.random.default_rng(19)
    Rmax = 90
    pairs = [draw(rng, int(rng.integers(0, Hmax + 1)), int(rng.integers(0, Rmax + 1)), 3) for _ in range(64)]
    pairs[5], pairs[63] = draw(rng, Hmax, Rmax, 2), draw(rng, Hmax - 1, Rmax - 1, 3)
    hyp, ref = padded([p[0] for p in pairs], Hmax, 4), padded([p[1] for p in pairs], Rmax, 8)
    hyp_len, ref_len = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    stats, status = call_raw(hyp, hyp_len, ref, ref_len)
    for s in (0, 5, 31, 63):
        alone = call_raw(hyp[s:s + 1], hyp_len[s:s + 1], ref[s:s + 1], ref_len[s:s + 1])
        assert np.array_equal(alone[0][0], stats[s]) and alone[1][0] == status[s] == 0, (Hmax, s)
        assert differs(alone[0][0], ref_of(*pairs[s])) is None


def test_ref_row_maps():
    rng = np.random.default_rng(23)
    refs = [draw(rng, 0, m, 2)[1] for m in (30, 7, 0, 64, 12)]
    hyps = [draw(rng, n, 0, 2)[0] for n in (30, 8, 5, 70, 12, 1, 0, 33, 64, 65, 2)]
    ref, ref_len = padded(refs, 64, 8), [len(r) for r in refs]
    hyp, hyp_len = padded(hyps, 70, 4), [len(h) for h in hyps]
    for row in ([0, 0, 0, 1, 1, 1, 3, 3, 3, 4, 4], [4, 3, 2, 1, 0, 0, 1, 2, 3, 4, 2], [2] * 11):       # n-best lists, a shuffle, one row
        stats, status = call_raw(hyp, hyp_len, ref, ref_len, ref_row=row)
        for s, r in enumerate(row):
            assert status[s] == 0 and differs(stats[s], ref_of(hyps[s], refs[r])) is None, (row, s)
    perm = [3, 0, 4, 1, 2]
    stats, status = call_raw(hyp[:5], hyp_len[:5], ref, ref_len, ref_row=perm)
    direct = call_raw(hyp[:5], hyp_len[:5], ref[perm], [ref_len[r] for r in perm])
    assert np.array_equal(stats, direct[0]) and np.array_equal(status, direct[1]), "a permutation through the map equals permuted rows"


# ---------------------------------------------------------------------------------------------- the class
def nbest_case(seed, B, N, width, k):
    rng = np.random.default_rng(seed)
    refs = [draw(rng, 0, int(rng.integers(3, width)), k)[1] + [EOS] for _ in range(B)]
    hypos = []
    for b in range(B):
        hs = []
        for _ in range(int(rng.integers(0, N + 1)) if b else N):
            h = [t if rng.random() < 0.7 else int(4 + rng.integers(0, k)) for t in refs[b]][:int(rng.integers(1, len(refs[b]) + 1))]
            hs.append({"tokens": torch.tensor(h[:-1] + [EOS], dtype=torch.int64, device=DEV)})
        hypos.append(hs)
    ref = torch.from_numpy(padded(refs, width, 8)).to(DEV)
    return refs, hypos, ref, torch.tensor([len(r) for r in refs], device=DEV)


def test_sentence_bleu_and_result_against_python_float64():
    """the integers are exact; sentence_bleu goes through four logs and an exp in float64: 1e-9 relative is float64 rounding"""
    from fbk_fairseq_st_amd import bleu_scorer as BS
    refs, hypos, ref, ref_len = nbest_case(29, 24, 1, 30, 3)
    hypos[3] = []
    bs = BS.BleuScorer(PAD, EOS, UNK)
    out = bs.score_hypotheses(hypos, ref, ref_len)
    assert out["sentence_bleu"].dtype == torch.float64 and out["sentence_bleu"].is_cuda and out["stats"].is_cuda
    want = [ref_of(h[0]["tokens"].tolist() if h else [], r) for h, r in zip(hypos, refs)]
    assert out["stats"].tolist() == want
    got = out["sentence_bleu"].tolist()
    for s, w in enumerate(want):
        assert got[s] == pytest.approx(R.sentence_bleu(w), rel=1e-9, abs=0), (s, w)
    assert got[3] == 0.0 and any(v > 0 for v in got)
    sums = np.array(want).sum(0).tolist()
    res = bs.result()
    assert [res[k] for k in BS._SUMS] == sums and res["bleu"] == R.score(sums) and bs.result_string() == R.result_string(sums)


def test_nbest_and_oracle():
    from fbk_fairseq_st_amd import bleu_scorer as BS
    refs, hypos, ref, ref_len = nbest_case(31, 16, 5, 40, 3)
    bs = BS.BleuScorer(PAD, EOS, UNK)
    out = bs.score_nbest(hypos, ref, ref_len, accumulate="oracle")
    host = {k: v.cpu() for k, v in out.items()}
    assert host["n_hyp"].tolist() == [len(h) for h in hypos] and tuple(host["stats"].shape) == (16, 5, 10)
    sums = np.zeros(10, np.int64)
    for b, hs in enumerate(hypos):
        scores = []
        for k, h in enumerate(hs):
            w = ref_of(h["tokens"].tolist(), refs[b])
            assert host["stats"][b, k].tolist() == w and host["status"][b, k] == 0, (b, k)
            scores.append(R.sentence_bleu(w))
            assert float(host["sentence_bleu"][b, k]) == pytest.approx(scores[-1], rel=1e-9, abs=0)
        assert (host["sentence_bleu"][b, len(hs):] == -1).all() and (host["stats"][b, len(hs):] == 0).all()
        o = int(host["oracle"][b])
        if hs:
            assert o < len(hs) and abs(scores[o] - max(scores)) <= 1e-9 * max(scores), (b, o, scores)
            assert float(host["sentence_bleu"][b, o]) == float(host["sentence_bleu"][b].max())
            assert o == int((host["sentence_bleu"][b] == host["sentence_bleu"][b].max()).nonzero()[0]), "the first of the best"
            sums += np.array(host["stats"][b, o].tolist())
        else:
            assert o == 0
    assert [bs.result()[k] for k in BS._SUMS] == sums.tolist()
    best = BS.BleuScorer(PAD, EOS, UNK)
    best.score_nbest(hypos, ref, ref_len, accumulate="best")
    plain = BS.BleuScorer(PAD, EOS, UNK)
    plain.score_hypotheses([h for h in hypos if h], ref[[b for b, h in enumerate(hypos) if h]], ref_len[[b for b, h in enumerate(hypos) if h]])
    assert best.result() == plain.result() and best.result()["bleu"] <= bs.result()["bleu"]


def test_score_hypotheses_on_the_device_search():
    """generate fixture case `c` through the device-resident search; its hypotheses are scored where they lie"""
    import test_model_gpu as TM
    from fbk_fairseq_st_amd import bleu_scorer as BS
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    task, model, src, lens, opts, exp, _ = TM.build_gen("c")
    gen = SequenceGenerator([model], task.target_dictionary, **opts)
    hypos = gen.generate([model], dict(net_input=dict(src_tokens=src, src_lengths=lens)))
    assert "launches_per_step" in gen.last_stats, "the search did not take the device route"
    d = task.target_dictionary
    bs = BS.BleuScorer.for_dictionary(d)
    assert (bs.pad, bs.eos, bs.unk) == (PAD, EOS, UNK)
    # references: the last hypothesis of every sentence, behind two pads and in front of three
    refs = [[PAD, PAD] + hs[-1]["tokens"].tolist() + [PAD] * 3 for hs in hypos]
    ref = torch.from_numpy(padded(refs, max(len(r) for r in refs), 8)).to(DEV)
    ref_len = torch.tensor([len(r) for r in refs], device=DEV)
    out = bs.score_hypotheses(hypos, ref, ref_len)
    want = [ref_of(hs[0]["tokens"].tolist(), r) for hs, r in zip(hypos, refs)]
    assert out["stats"].tolist() == want and all(w[1] > 0 and w[0] == max(len(r) - 6, 1) for w, r in zip(want, refs)), "eos and the pads are trimmed"
    assert bs.result_string() == R.result_string(np.array(want).sum(0).tolist())
    nb = bs.score_nbest(hypos, ref, ref_len)
    assert nb["n_hyp"].tolist() == [len(hs) for hs in hypos]
    for b, hs in enumerate(hypos):
        assert nb["stats"][b, len(hs) - 1].tolist() == ref_of(hs[-1]["tokens"].tolist(), refs[b])
        assert float(nb["sentence_bleu"][b, len(hs) - 1]) == pytest.approx(100.0, rel=1e-9), "a hypothesis against itself"
        assert float(nb["sentence_bleu"][b, int(nb["oracle"][b])]) == float(nb["sentence_bleu"][b].max())


# ---------------------------------------------------------------------------------------------- sensitivity
def test_wrong_twins_fail_this_files_comparison():
    """the comparison the sweeps make, on the sweeps' own kind of cases, fed a twin's answer in place of the kernel's"""
    rng = np.random.default_rng(1)
    cases = [draw(rng, n, m, 2) for n in range(7) for m in range(7)] + [([4] * n, [4] * m) for n in range(7) for m in range(7)]
    cases += [draw(rng, n, m, 4, lo=1) for n in range(7) for m in range(7)]
    for name in ("unclipped matches", "clip by the hypothesis count only", "trim to length 0", "no trim", "unk allowed to match"):
        caught = [c for c in cases if differs(R.TWINS[name](c[0], c[1], PAD, EOS, UNK), ref_of(*c)) is not None]
        assert caught, "no case of the sweep tells the rule from its twin: " + name
