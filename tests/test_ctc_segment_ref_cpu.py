"""The float64 reference of the segmentation rule (tests/ctc_segment_ref.py) against enumeration of every path for tiny cases under all
four flag combinations, against ctc_align_ref.viterbi with both flags off, its utterance outputs on a case worked by hand, and each of
its wrong twins against it on a stated share of seeded planted recordings."""
import itertools

import numpy as np
import pytest

import ctc_align_ref as A
import ctc_segment_ref as R

FLAGS = list(itertools.product((False, True), repeat=2))


@pytest.mark.parametrize("free_start,free_end", FLAGS)
def test_recursion_equals_enumeration(free_start, free_end):
    rng = np.random.default_rng(11)
    seen = 0
    for n, L, V in itertools.product(range(1, 8), range(1, 4), (2, 3)):
        for rep in range(3):
            y = A.draw_transcript(rng, L, V, V - 1, p_repeat=0.4)
            lp = A.log_softmax64(rng.standard_normal((n, V)) * 2)
            r = R.viterbi(lp, y, V - 1, free_start, free_end)
            best, arg = R.brute_force(R.emissions(lp, y, V - 1, free_start, free_end), y)
            if arg is None:
                assert r["status"] == 1 and n < A.min_frames(y)
                continue
            seen += 1
            assert r["status"] == 0 and r["score"] == best and tuple(r["states"]) == arg, (n, y)
            assert R.is_valid_path(r["states"], y, n)
            for U in range(1, min(L, 2) + 1):                       # the utterance outputs, restated on the enumerated path
                ends = [L] if U == 1 else [1 + rep % (L - 1), L]
                em = R.emissions(lp, y, V - 1, free_start, free_end)
                fr, sc, mean, low = R.utterances(R.path_values(em, r["states"]), r["states"], ends, 2)
                for u in range(U):
                    own = [t for t, s in enumerate(arg) if s % 2 and (ends[u - 1] if u else 0) <= s // 2 < ends[u]]
                    f0, f1 = own[0], own[-1] + 1
                    vals = [em[t, arg[t]] for t in range(f0, f1)]
                    wins = [sum(vals[i:i + 2]) / 2 for i in range(len(vals) - 1)] or [sum(vals) / len(vals)]
                    assert fr[u].tolist() == [f0, f1] and sc[u] == pytest.approx(sum(vals), abs=1e-12)
                    assert mean[u] == pytest.approx(sum(vals) / len(vals), abs=1e-12) and low[u] == pytest.approx(min(wins), abs=1e-12)
    assert seen >= 80


def test_both_flags_off_is_the_aligner_rule():
    for seed in range(12):
        c = A.planted_case(seed, 40 + seed, 7, 5 + seed, "f32", bonus=1.0)
        lp = A.log_softmax64(c["x"])
        a, r = A.viterbi(lp, c["y"], c["blank"]), R.viterbi(lp, c["y"], c["blank"], False, False)
        assert r["status"] == a["status"] == 0 and r["score"] == a["score"] and r["states"].tolist() == a["states"].tolist()
        s, f, t = R.path_sums(r["em"], r["states"], len(c["y"]))
        s2, f2, t2 = A.path_sums(lp, a["states"], c["y"], c["blank"])
        assert s == s2 and f.tolist() == f2.tolist() and t.tolist() == t2.tolist()


def test_free_ends_absorb_what_surrounds_the_text():
    """two tokens a b in frames 3 and 4 of 8; everything else favours a symbol that is not in the transcript"""
    x = np.zeros((8, 4))
    x[:, 2] = 6.0
    x[3], x[4] = [6, 0, 0, 0], [0, 6, 0, 0]
    r = R.segment(x, 8, [[0], [1]], 3)
    assert r["states"].tolist() == [0, 0, 0, 1, 3, 4, 4, 4]
    assert r["utt_frames"].tolist() == [[3, 4], [4, 5]] and r["frames"].tolist() == [[3, 4], [4, 5]]
    lp = A.log_softmax64(x)
    assert r["score"] == pytest.approx(lp[3, 0] + lp[4, 1]) and r["utt_score"].tolist() == pytest.approx([lp[3, 0], lp[4, 1]])
    pinned = R.segment(x, 8, [[0], [1]], 3, free_start=False, free_end=False)
    assert pinned["score"] < r["score"] - 30                         # six frames of an unlikely blank


def test_utterance_outputs_by_hand():
    vals = np.array([0, -1, -2, -9, -1, -1, -3, -1, 0, 0], dtype=np.float64)
    states = np.array([0, 1, 1, 2, 3, 5, 6, 7, 8, 8])                # y = a b c d, utterances [a b] [c d]; frame 6: a blank between
    fr, sc, mean, low = R.utterances(vals, states, [2, 4], 2)
    assert fr.tolist() == [[1, 5], [5, 8]]
    assert sc.tolist() == [-13, -5] and mean.tolist() == [-13 / 4, -5 / 3] and low.tolist() == [-11 / 2, -4 / 2]
    fr, sc, mean, low = R.utterances(vals, states, [2, 4], 4)
    assert low.tolist() == [-13 / 4, -5 / 3]                         # a window as long as the span; a span shorter than the window
    fr, _, _, low = R.utterances(vals, states, [3, 4], 3)            # the blank of frame 6 lies between the utterances: in neither
    assert fr.tolist() == [[1, 6], [7, 8]] and low.tolist() == [-12 / 3, -1]
    fr, _, _, _ = R.utterances(vals, states, [3, 4], 3, span_from_blanks=True)
    assert fr.tolist() == [[0, 7], [6, 10]]
    _, _, _, low = R.utterances(vals, states, [2, 4], 2, window_leaves_span=True)
    assert low.tolist() == [-11 / 2, -4 / 2]
    _, _, _, low = R.utterances(vals, states, [1, 4], 2, window_leaves_span=True)
    assert low[0] == -11 / 2                                         # frames 2 and 3: the window left the span [1, 3)


CASES = [dict(seed=s, T=160 + 7 * s, V=5 + s % 3, L=12 + s, U=1 + s % 4, pre=10 + 3 * s, post=5 + 2 * s) for s in range(20)]


@pytest.mark.parametrize("twin,share", [("charge_free", 1.0), ("span_from_blanks", 0.9), ("window_leaves_span", 0.25)])
def test_every_twin_differs_on_its_share_of_the_seeded_cases(twin, share):
    differs = 0
    for c in CASES:
        p = R.planted_recording(c["seed"], c["T"], c["V"], c["L"], c["U"], "f32", c["pre"], c["post"])
        r = R.segment(p["x"], c["T"], p["utts"], p["blank"], window=8)
        assert r["status"] == 0 and r["states"].tolist() == p["path"].tolist(), "the planted path is the best one"
        q = R.segment(p["x"], c["T"], p["utts"], p["blank"], window=8, **{twin: True})
        same = all(np.array_equal(q[k], r[k]) for k in ("states", "utt_frames")) and \
            np.allclose(q["utt_conf_min"], r["utt_conf_min"], rtol=0, atol=1e-9)
        differs += not same
    assert differs >= share * len(CASES), (twin, differs)
