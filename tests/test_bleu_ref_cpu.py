"""The BLEU statistics rule in plain Python (tests/bleu_ref.py) against the reference's own numbers (tests/golden/bleu_stats.npz, made
by tests/golden/make_bleu_fixture.py from the reference's compiled bleu_add and its Scorer): the Counter form and the position-wise
form agree with each other and with every row and every string of the fixture, and every wrong twin differs from it."""
import os

import numpy as np
import pytest

import bleu_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bleu_stats.npz")
SUBSETS = ("all", "first", "small_alphabets", "quirks")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


def rows(g, rule):
    pad, eos, unk = int(g["pad"]), int(g["eos"]), int(g["unk"])
    return [rule(g["hyp"][s, :g["hyp_len"][s]], g["ref"][s, :g["ref_len"][s]], pad, eos, unk) for s in range(len(g["hyp"]))]


def test_fixture_holds_what_it_says(g):
    pad, eos, unk = int(g["pad"]), int(g["eos"]), int(g["unk"])
    N = len(g["hyp"])
    assert 250 <= N <= 400 and g["hyp"].shape[1] <= 40 and os.path.getsize(GOLDEN) < 100 * 1024
    assert g["stats"].shape == (N, 10) and len({pad, eos, unk}) == 3
    hyps = [g["hyp"][s, :g["hyp_len"][s]].tolist() for s in range(N)]
    refs = [g["ref"][s, :g["ref_len"][s]].tolist() for s in range(N)]
    sizes = {len(set(h + r) - {pad, eos, unk}) for h, r in zip(hyps, refs)}
    assert {1, 2, 3} <= sizes and max(sizes) > 20, "alphabets of 2, 3 and 50 symbols"
    assert any(h[0] == pad for h in hyps) and any(r[0] == pad for r in refs) and any(h[-1] == pad for h in hyps), "pads at both ends"
    assert any(pad in R.trim(h, pad, eos)[1:-1] for h in hyps) and any(eos in R.trim(r, pad, eos)[1:-1] for r in refs), "interior pad / eos"
    assert any(R.trim(h, pad, eos) == [eos] for h in hyps) and any(R.trim(r, pad, eos) == [eos] for r in refs), "[eos] alone"
    assert any(len(set(h)) == 1 and len(set(r)) == 1 and h[0] == r[0] and len(h) > len(r) for h, r in zip(hyps, refs)), "a run against a shorter run"
    assert any(unk in h for h in hyps) and any(unk in r for r in refs)
    assert all(R.trim(h, pad, eos) and R.trim(r, pad, eos) for h, r in zip(hyps, refs)), "the reference reads out of bounds on an empty side"
    # the quirks are visible in the numbers: lengths after the trim, a reference unk that matched nothing
    s = [i for i in range(N) if hyps[i] == [eos, eos, eos]][0]
    assert g["stats"][s, 1] == 1 and g["stats"][s, 3] == 1
    s = [i for i in range(N) if hyps[i] == [unk] and refs[i] == [unk]][0]
    assert g["stats"][s].tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("form", ["counter", "positional"])
def test_both_forms_reproduce_every_row_of_the_fixture(g, form):
    got = rows(g, {"counter": R.stats_counter, "positional": R.stats_positional}[form])
    for s, row in enumerate(got):
        assert row == g["stats"][s].tolist(), (s, g["hyp"][s, :g["hyp_len"][s]].tolist(), g["ref"][s, :g["ref_len"][s]].tolist())


def test_strings_and_scores_of_the_fixture(g):
    for name in SUBSETS:
        sums = g["stats"][g["subset_" + name]].sum(0).tolist()
        assert R.result_string(sums) == str(g["string_" + name]), name
        assert R.result_string(sums, order=2) == str(g["string2_" + name]), name
        assert R.score(sums) == float(g["score_" + name]), name


def random_pair(rng):
    k = (2, 3, 6, 50)[int(rng.integers(0, 4))]
    alphabet = np.array([1, 2, 3] + list(range(4, 4 + k)))          # pad, eos and unk among the symbols
    p = np.array([0.05, 0.05, 0.05] + [0.85 / k] * k)
    draw = lambda: rng.choice(alphabet, int(rng.integers(0, 25)), p=p).tolist()
    return draw(), draw()


def test_the_two_forms_agree_on_random_pairs():
    rng = np.random.default_rng(5)
    seen = set()
    for q in range(2000):
        h, r = random_pair(rng)
        unk = (3, -1)[q % 2]
        a, b = R.stats_counter(h, r, 1, 2, unk), R.stats_positional(h, r, 1, 2, unk)
        assert a == b, (h, r, unk, a, b)
        assert a[3::2] == [max(a[1] - n + 1, 0) for n in R.ORDERS] and all(m <= c for m, c in zip(a[2::2], a[3::2]))
        assert all(a[2 + 2 * k] <= max(a[0] - k, 0) for k in range(4)), "no more matches than the reference has n-grams"
        seen.add((a[0] == 0, a[1] == 0))
    assert len(seen) == 4, "empty sides occur"


def test_trim_and_empty_sides():
    assert R.trim([1, 1, 4, 2, 1, 2], 1, 2) == [4] and R.trim([2, 2, 2], 1, 2) == [2] and R.trim([1, 2], 1, 2) == [2]
    assert R.trim([4, 1, 2, 5, 2], 1, 2) == [4, 1, 2, 5] and R.trim([1, 1], 1, 2) == [] and R.trim([], 1, 2) == []
    assert R.trim([2, 4], 1, 2) == [2, 4] and R.trim([2, 1, 1], 1, 2) == [2]
    for rule in (R.stats_counter, R.stats_positional):
        assert rule([1, 1], [4, 5], 1, 2) == [2] + [0] * 9 and rule([], [], 1, 2) == [0] * 10
        assert rule([4, 5], [1], 1, 2) == [0, 2, 0, 2, 0, 1, 0, 0, 0, 0]
        assert rule([3, 4], [3, 4], 1, 2, 3) == [2, 2, 1, 2, 0, 1, 0, 0, 0, 0] and rule([3, 4], [3, 4], 1, 2, -1)[2:6] == [2, 2, 1, 1]


def test_batch_form_refuses_what_the_kernel_refuses():
    hyp, ref = np.array([[4, 5, 6], [4, 4, 4], [7, 7, 7], [4, 5, 6]]), np.array([[4, 5], [4, 4]])
    stats, status = R.bleu_stats_batch(hyp, [3, 4, -1, 2], ref, [2, 3], 1, 2, ref_row=[0, 1, 1, 1])
    assert status.tolist() == [0, 2, 2, 2] and (stats[1:] == 0).all() and stats[0].tolist() == [2, 3, 2, 3, 1, 2, 0, 1, 0, 0]
    stats, status = R.bleu_stats_batch(hyp, [3, 3, 3, 3], ref, [2, 2], 1, 2, ref_row=[0, 2, -1, 1])
    assert status.tolist() == [0, 2, 2, 0] and stats[3].tolist() == [2, 3, 1, 3, 0, 2, 0, 1, 0, 0]


def test_sentence_bleu_is_the_one_init_scorer():
    import math
    assert R.sentence_bleu([3, 3, 3, 3, 2, 2, 1, 1, 0, 0]) == pytest.approx(100.0, rel=1e-15)
    assert R.sentence_bleu([5, 0] + [0] * 8) == 0.0 and R.sentence_bleu([4, 4, 0, 4, 0, 3, 0, 2, 0, 1]) == 0.0
    want = math.exp(1 - 6 / 4) * math.exp((math.log(3 / 4) + math.log(2 / 4) + math.log(1 / 3) + math.log(1 / 2)) / 4) * 100
    assert R.sentence_bleu([6, 4, 3, 4, 1, 3, 0, 2, 0, 1]) == want


def test_every_wrong_twin_differs_from_the_fixture(g):
    assert sorted(R.TWINS) == sorted(["unclipped matches", "unk allowed to match", "no trim", "trim to length 0",
                                      "clip by the hypothesis count only"])
    for name, twin in R.TWINS.items():
        got = rows(g, twin)
        wrong = [s for s, row in enumerate(got) if row != g["stats"][s].tolist()]
        assert wrong, "no row of the fixture tells the rule from its twin: " + name
