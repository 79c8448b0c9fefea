"""The plain-Python edit-distance reference (tests/edit_ref.py) checked on its own, without a GPU: against the oracle's restatement
of the reference's alignment, against the cheapest of ALL alignments by enumeration, against the reference's own compute_ctc_uer
numbers, the anti-diagonal form and the carried counts against the loop form, and every wrong twin against the rule."""
import os

import numpy as np

import edit_ref as R
from oracle import int_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COSTS = ((1, 1, 1), (4, 3, 3), (3, 2, 1))


def pairs(seed, count, max_len, alphabets=(3, 6)):
    rng = np.random.default_rng(seed)
    out = []
    for q in range(count):
        k = alphabets[q % len(alphabets)]
        out.append((rng.integers(0, k, rng.integers(0, max_len + 1)).tolist(), rng.integers(0, k, rng.integers(0, max_len + 1)).tolist()))
    return out


def test_error_counts_equal_the_oracles_alignment():
    """oracle.int_ref.align_errors_np restates wer_utils.EditDistance(False) + compute_ctc_uer's count: costs (4, 3, 3)"""
    for a, b in pairs(1, 400, 14, alphabets=(3,)):
        cost, counts, ops = R.align(a, b, (4, 3, 3))
        assert counts[1] + counts[2] + counts[3] == int_ref.align_errors_np(a, b), (a, b)
        assert R.carried(a, b, (4, 3, 3)) == (cost, counts), (a, b)


def all_alignment_costs(a, b, costs):
    cs, ca, cb = costs

    def go(i, j):
        if i == len(a) and j == len(b):
            yield 0
            return
        if i < len(a) and j < len(b):
            for c in go(i + 1, j + 1):
                yield c + (0 if a[i] == b[j] else cs)
        if i < len(a):
            for c in go(i + 1, j):
                yield c + ca
        if j < len(b):
            for c in go(i, j + 1):
                yield c + cb
    return go(0, 0)


def test_cost_is_the_cheapest_of_all_alignments():
    rng = np.random.default_rng(2)
    for costs in COSTS + ((1, 5, 2), (255, 1, 255)):
        for _ in range(40):
            a, b = rng.integers(0, 3, rng.integers(0, 6)).tolist(), rng.integers(0, 3, rng.integers(0, 6)).tolist()
            cost, counts, ops = R.align(a, b, costs)
            assert cost == min(all_alignment_costs(a, b, costs)), (a, b, costs)
            assert R.replay(a, b, ops) and cost == counts[1] * costs[0] + counts[3] * costs[1] + counts[2] * costs[2]
            assert counts[0] + counts[1] + counts[3] == len(a) and counts[0] + counts[1] + counts[2] == len(b)


def test_collapse_and_alignment_reproduce_the_reference_uer_counts():
    """tests/golden/ctc_uer.npz holds `errors` and `total` of the reference's compute_ctc_uer on these log-probabilities"""
    g = dict(np.load(os.path.join(GOLDEN, "ctc_uer.npz")))
    blank = int(g["blank"])
    pred = g["lp"].argmax(-1)
    errors = total = 0
    for s in range(pred.shape[0]):
        hyp = R.collapse(pred[s, :int(g["in_len"][s])], blank)
        tgt = g["tgt"][s, :int(g["tgt_len"][s])]
        _, counts, _ = R.align(hyp, tgt, (4, 3, 3))
        errors += counts[1] + counts[2] + counts[3]
        total += len(tgt)
    assert (float(errors), float(total)) == (float(g["errors"]), float(g["total"]))
    assert R.collapse([1, 1, 3, 1, 1, 2, 3, 3, 2], 3) == [1, 1, 2, 2] and R.collapse([], 3) == [] and R.collapse([3, 3], 3) == []
    counts, cost, status, a_n, a_out, _, _ = R.edit_align_batch(pred, g["in_len"], g["tgt"], g["tgt_len"], (4, 3, 3), collapse_blank=blank)
    assert float(counts[:, 1:].sum()) == float(g["errors"]) and not status.any()


def test_numpy_form_and_carried_counts_equal_the_loop_form():
    for costs in COSTS:
        for a, b in pairs(3, 120, 24):
            want = R.align(a, b, costs)
            assert R.align_np(a, b, costs) == want, (a, b, costs)
            assert R.carried(a, b, costs) == want[:2], (a, b, costs)
    assert R.align([], [], (4, 3, 3)) == (0, (0, 0, 0, 0), []) == R.align_np([], [], (4, 3, 3))
    assert R.align([5, 5], [], (4, 3, 2)) == (6, (0, 0, 0, 2), [R.A, R.A])
    assert R.align([], [5, 5, 5], (4, 3, 2)) == (6, (0, 0, 3, 0), [R.B] * 3)
    # the path that costs least is not always the path with the fewest errors: (4, 3, 3) prefers nothing here, (1, 1, 1) does
    assert R.align([1, 2], [2, 1], (1, 1, 1))[1] == (0, 2, 0, 0)
    a, b = [0, 0, 0, 2, 2], [2, 2, 1, 1, 0]
    assert sum(R.align(a, b, (4, 3, 3))[1][1:]) == 6 and sum(R.align(a, b, (1, 1, 1))[1][1:]) == 5


def test_every_twin_differs_from_the_rule():
    """The numbers of pairs on which a twin's path / counts differ from the rule's, over 300 random pairs (lengths 0-24): the tie
    order shows in the paths and under asymmetric costs, which is why the GPU tests compare paths and use (3, 2, 1)."""
    cases = pairs(4, 300, 24)

    def differing(twin, costs):
        path = counts = cost = 0
        for a, b in cases:
            want, got = R.align(a, b, costs), twin(a, b, costs)
            path += got[2] != want[2]
            counts += got[1] != want[1]
            cost += got[0] != want[0]
        return path, counts, cost
    path, counts, cost = differing(R.twin_up_first, (4, 3, 3))
    assert path >= 10 and counts >= 1 and cost == 0
    path, counts, cost = differing(R.twin_up_first, (3, 2, 1))
    assert path >= 40 and counts >= 30 and cost == 0
    for costs in COSTS:
        assert differing(R.twin_non_strict, costs)[0] >= 240, costs
    assert differing(R.twin_swapped, (3, 2, 1))[2] >= 200, "the swap shows in the cost whenever the lengths differ"
    assert differing(R.twin_swapped, (4, 3, 3)) == (0, 0, 0), "symmetric costs cannot show the swap"
    path, counts, cost = differing(R.twin_levenshtein_counts, (4, 3, 3))
    assert counts >= 50 and path >= counts and cost == 0
    assert differing(R.twin_levenshtein_counts, (1, 1, 1)) == (0, 0, 0)
