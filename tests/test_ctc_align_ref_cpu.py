"""The float64 alignment reference (tests/ctc_align_ref.py) against enumeration of every valid path, and its two wrong twins against the
cases that are there to contradict them.  No GPU, no library."""
import itertools

import numpy as np
import pytest

import ctc_align_ref as R

V, BLANK = R.TWIN_V, R.TWIN_BLANK


def transcripts(max_len):
    """every transcript of up to max_len non-blank tokens over V = 4, repeated tokens included"""
    for L in range(max_len + 1):
        yield from (list(y) for y in itertools.product(range(V - 1), repeat=L))


@pytest.mark.parametrize("T", range(1, 8))
def test_reference_against_every_path(T):
    rng = np.random.default_rng(T)
    lp = R.log_softmax64(rng.standard_normal((T, V)) * 2)
    for y in transcripts(3):
        r = R.viterbi(lp, y, BLANK)
        best, path = R.brute_force(lp, y, BLANK)
        if path is None:
            assert r["status"] == 1 and T < R.min_frames(y), (T, y)
            continue
        assert r["status"] == 0 and T >= R.min_frames(y)
        assert abs(r["score"] - best) <= 1e-12 * max(1, abs(best)) and list(r["states"]) == list(path), (T, y)
        assert R.is_valid_path(r["states"], y, T)
        score, frames, tok = R.path_sums(lp, r["states"], y, BLANK)
        assert abs(score - best) <= 1e-12 * max(1, abs(best)) and abs(score - tok.sum() - lp[r["states"] % 2 == 0, BLANK].sum()) < 1e-12
        assert all(list(r["states"][f0:f1]) == [2 * i + 1] * (f1 - f0) and f1 > f0 for i, (f0, f1) in enumerate(frames))


@pytest.mark.parametrize("T", range(1, 8))
def test_tie_rule_on_planted_exact_ties(T):
    """log-probabilities that are multiples of 1/4 (sums are exact in float64), few distinct values: many paths share the best value.
    The rule picks the path whose states, read from the last frame backwards, are highest."""
    rng = np.random.default_rng(100 + T)
    ties = 0
    for rep in range(3):
        lp = -0.25 * rng.integers(0, 3, size=(T, V)).astype(np.float64)
        for y in transcripts(3):
            best, path = R.brute_force(lp, y, BLANK)
            if path is None:
                continue
            z, _ = R.extended(y, BLANK)
            ties += sum(float(sum(lp[t, z[s]] for t, s in enumerate(p))) == best for p in R.all_paths(T, y)) > 1
            r = R.viterbi(lp, y, BLANK)
            assert r["score"] == best and list(r["states"]) == list(path), (T, rep, y)
    assert T <= 2 or ties > 10, "the inputs were to hold exact ties"


def test_all_ties_stay_over_advance_over_skip_and_end_in_the_last_state():
    lp = np.zeros((5, V))
    r = R.viterbi(lp, [0, 1], BLANK)
    assert list(r["states"]) == [1, 3, 4, 4, 4] and r["margin"] == 0.0
    r = R.viterbi(lp, [0, 0], BLANK)
    assert list(r["states"]) == [1, 2, 3, 4, 4]


def test_margin_is_the_closest_decision_on_the_path():
    lp = R.log_softmax64(np.array([[4.0, 0, 0, 0], [0, 0, 0, 4.0], [0, 0, 0, 4.0 + 1e-3]]))
    r = R.viterbi(lp, [0], BLANK)
    assert list(r["states"]) == [1, 2, 2] and r["margin"] > 0.1
    lp2 = lp.copy()
    lp2[1, 0] = lp2[1, 3] - 1e-6                                       # staying in the token at frame 1 is now nearly as good
    r2 = R.viterbi(lp2, [0], BLANK)
    assert list(r2["states"]) == [1, 2, 2] and 0 < r2["margin"] < 1e-5


# ------------------------------------------------------------------ the wrong twins
def test_twin_that_skips_between_equal_tokens_is_contradicted():
    x, y = R.twin_case_equal_tokens()
    right, wrong = R.align(x, 3, y, BLANK), R.align(x, 3, y, BLANK, skip_equal=True)
    assert list(right["states"]) == [1, 2, 3] and R.is_valid_path(right["states"], y, 3)
    assert list(wrong["states"]) == [1, 3, 3] and not R.is_valid_path(wrong["states"], y, 3)
    assert R.brute_force(right["lp"], y, BLANK)[1] == (1, 2, 3)


def test_twin_that_ends_in_the_last_state_only_is_contradicted():
    x, y = R.twin_case_ends_in_a_token()
    right, wrong = R.align(x, 4, y, BLANK), R.align(x, 4, y, BLANK, end_last_only=True)
    assert list(right["states"]) == [1, 1, 3, 3] and right["states"][-1] == 2 * len(y) - 1
    assert wrong["states"][-1] == 2 * len(y) and wrong["score"] < right["score"] - 1
    assert R.brute_force(right["lp"], y, BLANK)[1] == (1, 1, 3, 3)


# ------------------------------------------------------------------ the generators
def test_planted_paths_are_valid_and_have_skips_and_repeats():
    skips = repeats = 0
    for seed in range(8):
        c = R.planted_case(seed, 130, 300, 64, "bf16")
        assert R.is_valid_path(c["path"], c["y"], 130) and len(c["y"]) == 64 and c["blank"] not in c["y"]
        skips += int((np.diff(c["path"]) == 2).sum())
        repeats += sum(a == b for a, b in zip(c["y"], c["y"][1:]))
        r = R.align(c["x"], 130, c["y"], c["blank"])
        assert r["status"] == 0 and r["margin"] >= 1e-4
    assert skips > 50 and repeats > 20
    y = R.draw_transcript(np.random.default_rng(0), 6, 2, 0)
    assert y == [1] * 6 and R.min_frames(y) == 11
    path = R.draw_path(np.random.default_rng(0), y, 11)
    assert list(path) == list(range(1, 12)), "at L + repeats frames exactly one path exists"


def test_batch_form_statuses_and_untouched_entries():
    rng = np.random.default_rng(3)
    T, B, Lmax = 9, 5, 4
    x = rng.standard_normal((T, B, V)).astype(np.float32)
    targets = np.array([[0, 1, 2, 99], [0, 0, 0, 0], [0, BLANK, 1, 1], [1, 2, 0, 0], [2, 2, 2, 2]])
    states, frames, tok, score, status = R.align_batch(x, [9, 9, 9, 3, 9], targets, [3, 0, 3, 4, 5], BLANK)
    assert status.tolist() == [0, 0, 2, 1, 2]
    assert R.is_valid_path(states[0], [0, 1, 2], 9) and (frames[0, 3] == -7).all() and np.isnan(tok[0, 3])
    assert states[1].tolist() == [0] * 9 and (frames[1] == -7).all()
    assert (states[2] == -1).all() and (frames[2, :3] == -1).all() and (frames[2, 3] == -7).all() and score[2] == -np.inf
    assert (states[3] == -1).all() and (frames[3] == -1).all() and np.isneginf(tok[3]).all()
    assert (frames[4] == -7).all() and np.isnan(tok[4]).all() and score[4] == -np.inf
