"""The float64 reference of the CTC decoders (tests/ctc_decode_ref.py) checked on its own, without a GPU: against the brute-force sum
over all alignments, against the reference's compute_ctc_uer numbers, and the random-case generator against the two conditions the
GPU test relies on (enough re-created prefixes, few near-ties)."""
import os

import numpy as np

import ctc_decode_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

def test_exact_marginals_against_all_alignments():
    """cand = V - 1 and a beam that holds every prefix: the totals are the strings' exact probabilities"""
    rng = np.random.default_rng(5)
    for T in (1, 2, 3, 5, 6):
        for blank in (0, 2):
            x = rng.standard_normal((T, 3)) * 2
            exact = R.brute_force_marginals(x, blank)
            got = R.prefix_beam(x, T, blank, beam=1000, cand=2, nbest=1000)
            assert set(got["totals"]) == set(exact), (T, blank)
            for s, v in exact.items():
                assert abs(got["totals"][s] - v) <= 1e-12, (T, blank, s, got["totals"][s], v)
            assert [h[0] for h in got["hyps"]] == sorted(exact, key=lambda s: -exact[s])
            assert abs(np.logaddexp.reduce(list(exact.values()))) <= 1e-12          # and they sum to one
    one = R.prefix_beam(np.zeros((1, 2)), 1, 1, beam=4, cand=1, nbest=4)
    assert [h[0] for h in one["hyps"]] in ([(), (0,)], [(0,), ()]) and len(one["hyps"]) == 2       # T = 1, V = 2: two prefixes
    none = R.prefix_beam(np.zeros((3, 4)), 0, 3, beam=4, cand=2, nbest=2)
    assert none["hyps"] == [((), 0.0)]


def test_greedy_reproduces_the_reference_uer_counts():
    """tests/golden/ctc_uer.npz holds `errors` and `total` of the reference's compute_ctc_uer on these log-probabilities"""
    g = dict(np.load(os.path.join(GOLDEN, "ctc_uer.npz")))
    blank = int(g["blank"])
    errors = total = 0
    for b in range(g["lp"].shape[0]):
        tokens, frames, tok_score, score = R.greedy(g["lp"][b], int(g["in_len"][b]), blank)
        tgt = [int(v) for v in g["tgt"][b, :int(g["tgt_len"][b])]]
        errors += R.levenshtein(tokens, tgt)
        total += len(tgt)
        assert len(tokens) == len(frames) == len(tok_score) and blank not in tokens
        assert all(a < e for a, e in frames) and all(frames[i][1] <= frames[i + 1][0] for i in range(len(frames) - 1))
        assert score <= sum(tok_score) + 1e-12                                         # blank frames belong to score only
    assert (float(errors), float(total)) == (float(g["errors"]), float(g["total"]))


def test_greedy_collapse_rule():
    x = np.full((5, 4), -5.0)
    for t, v in enumerate([1, 3, 1, 1, 2]):                            # a _ a a b with blank 3
        x[t, v] = 5.0
    tokens, frames, tok_score, score = R.greedy(x, 5, 3)
    assert tokens == [1, 1, 2] and frames == [(0, 1), (2, 4), (4, 5)]
    assert abs(tok_score[1] - 2 * tok_score[0]) <= 1e-12 and abs(score - 5 * tok_score[0]) <= 1e-12
    assert R.greedy(x, 3, 3)[0] == [1, 1] and R.greedy(x, 0, 3) == ([], [], [], 0.0)
    x[0, 0] = 5.0                                                       # an arg-max tie: the first index
    assert R.greedy(x, 1, 3)[0] == [0]


def test_generator_seeds_meet_the_gpu_tests_conditions():
    """of the f32 seeds the GPU test runs: every case within the generator's ranges, at least 5 contain a pruned prefix re-created
    under a live child and survive the margin, and at most 15 % have a keep / drop margin below MIN_GAP (the GPU test skips those by
    name).  Rounded to bf16 (ctc_decode_ref.GPU_SEEDS_BF16 says why it has more seeds): at least 51 cases stay, 5 of them with a
    re-created prefix."""
    for name, seeds in (("f32", R.GPU_SEEDS), ("bf16", R.GPU_SEEDS_BF16)):
        recreated = close = 0
        for seed in seeds:
            c, x, right, _ = R.case_reference(seed, name)
            assert 5 <= c["T"] <= 80 and c["V"] in (6, 12, 33, 100) and c["beam"] in (1, 2, 4, 8, 16)
            assert 1 <= c["cand"] <= min(8, c["V"] - 1) and c["x"].dtype == np.float32 and x.shape == (c["T"], c["V"])
            close += right["gap"] < R.MIN_GAP
            recreated += bool(right["recreated"]) and right["gap"] >= R.MIN_GAP
        print("%s: %d seeds, %d kept ones re-create a pruned prefix, %d below the margin" % (name, len(seeds), recreated, close))
        assert recreated >= 5, recreated
        if name == "f32":
            assert close <= R.MAX_SKIPPED * len(seeds), close
        else:
            assert len(seeds) - close >= R.MIN_KEPT_BF16, close


def test_the_wrong_twin_differs_on_a_kept_seed():
    """identity by parent entry splits a string's probability when a pruned prefix comes back: on at least one seed that the GPU test
    keeps, the twin's hypotheses differ from the reference's -- and never where no prefix was re-created"""
    for name, seeds in (("f32", R.GPU_SEEDS), ("bf16", R.GPU_SEEDS_BF16)):
        differ = []
        for seed in seeds:
            c, x, right, wrong = R.case_reference(seed, name)
            if not R.same_hyps(right["hyps"], wrong["hyps"]):
                assert right["recreated"], "seed %d: the twin differs without a re-created prefix" % seed
                if right["gap"] >= R.MIN_GAP:
                    differ.append(seed)
        print("%s: the twin differs on kept seeds" % name, differ)
        assert differ
