"""The plain-Python MBR reference (tests/mbr_ref.py) against a brute-force restatement: for lists of up to 4 hypotheses of up to 5
tokens over 2 symbols, every pair goes through bleu_ref.stats_positional (the other form of the rule) and the arithmetic of the
utility, the gain and the choice is spelled out here.  The wrong twins of the reference are run over the same cases: the file prints
how many each gets wrong, and each must be wrong on at least one."""
import math

import numpy as np

import bleu_ref as R
import mbr_ref as MR

PAD, EOS, UNK = 1, 2, 3


def brute(lists, weights):
    """-> per sentence (gains, first best or -1), the lists judged against themselves"""
    out = []
    for b, hs in enumerate(lists):
        gains = []
        for h in hs:
            num = den = 0.0
            for k, r in enumerate(hs):
                s = R.stats_positional(h, r, PAD, EOS, UNK)
                reflen, predlen = s[0], s[1]
                if predlen == 0 or s[2] == 0:
                    u = 0.0
                else:
                    logs = math.log(s[2] / s[3])
                    for n in (2, 3, 4):
                        logs += math.log((s[2 * n] + 1) / (s[2 * n + 1] + 1))
                    u = min(1, math.exp(1 - reflen / predlen)) * math.exp(logs / 4) * 100
                w = 1.0 if weights is None else float(weights[b][k])
                num += w * u
                den += w
            gains.append(num / den if den > 0 else 0.0)
        out.append((gains, gains.index(max(gains)) if gains else -1))
    return out


def cases():
    rng = np.random.default_rng(41)
    out = []
    for q in range(240):
        lists = []
        for _ in range(int(rng.integers(1, 4))):
            hs = [(4 + rng.integers(0, 2, int(rng.integers(0, 6)))).tolist() for _ in range(int(rng.integers(0, 5)))]
            if len(hs) >= 2 and q % 3 == 0:
                hs[-1] = list(hs[int(rng.integers(0, len(hs) - 1))])               # a planted duplicate: an exact tie
            if hs and q % 5 == 0:
                hs[0] = hs[0][:4] + [EOS]
            if hs and q % 7 == 0:
                hs[-1] = ([UNK] + hs[-1])[:5]
            lists.append(hs)
        weights = None if q % 2 else [[float(rng.choice([0.0, 0.5, 1.0, 2.0, 3.0])) for _ in hs] for hs in lists]
        out.append((lists, weights))
    return out


def answer(lists, weights, twin=None):
    cand, cand_len, cand_sent, off = MR.matrices(lists)
    w = None if weights is None else [x for ws in weights for x in ws]
    got = MR.expected_bleu(cand, cand_len, cand_sent, cand, cand_len, off, PAD, EOS, UNK, w, twin=twin)
    first = [int(o) for o in off]
    return [(got["gain"][first[b]:first[b + 1]], got["best"][b] - first[b] if got["best"][b] >= 0 else -1) for b in range(len(lists))]


def differs(got, want):
    """None when every gain is within 1e-12 relative and every choice is the same"""
    for b, ((g, best), (wg, wbest)) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g, wg)):
            if abs(x - y) > 1e-12 * max(abs(y), 1e-300):
                return "sentence %d, hypothesis %d: gain %r, brute force %r" % (b, k, x, y)
        if best != wbest:
            return "sentence %d: chose %d, brute force %d" % (b, best, wbest)
    return None


def test_reference_equals_brute_force():
    ties = 0
    for lists, weights in cases():
        want = brute(lists, weights)
        bad = differs(answer(lists, weights), want)
        assert bad is None, (lists, weights, bad)
        ties += sum(1 for g, _ in want if g and sum(1 for x in g if x == max(g)) > 1)
    assert ties >= 10, "the cases hold exact ties"


def test_statistics_refusals_and_zeros_behind_lists():
    lists = [[[4, 5, 4], [5, 5]], [], [[4], [4, 4, 5, EOS], [5]]]
    cand, cand_len, cand_sent, off = MR.matrices(lists, width=5)
    cand_len = cand_len.copy()
    stats, status = MR.pair_stats(cand, cand_len, cand_sent, cand, cand_len, off, PAD, EOS, UNK)
    assert stats.shape == (5, 3, 10) and status.shape == (5, 3) and not status.any()
    assert stats[0, 1].tolist() == R.stats_counter([4, 5, 4], [5, 5], PAD, EOS, UNK) and stats[3, 0].tolist() == R.stats_counter([4, 4, 5, EOS], [4], PAD, EOS)
    assert not stats[0, 2].any() and not stats[1, 2].any(), "behind a list of two"
    cand_len[3] = 6                                                   # as a candidate and as a pseudo-reference
    sent = cand_sent.copy()
    sent[0] = 7
    stats, status = MR.pair_stats(cand, cand_len, sent, cand, cand_len, off, PAD, EOS, UNK)
    assert status.tolist() == [[2, 2, 2], [0, 0, 0], [0, 2, 0], [2, 2, 2], [0, 2, 0]] and not stats[3].any() and stats[4, 2].any()
    _, gain, best = MR.select(stats, status, cand_len, 5, sent, off, 5)
    assert gain[0] == gain[3] == -1.0 and gain[2] > 0 and best[1] == -1 and best[0] == 1
    for bad_off in ([0, 2, 1, 5], [0, 2, 2, 6], [-1, 2, 2, 5]):
        _, status = MR.pair_stats(cand, cand_len, cand_sent, cand, cand_len, bad_off, PAD, EOS, UNK, M=3)
        assert (status == 2).all(1).any() and not (status == 2).all(), bad_off


def test_every_twin_is_wrong_somewhere():
    all_cases = cases()
    for name in MR.TWINS:
        wrong = sum(1 for lists, weights in all_cases if differs(answer(lists, weights, twin=name), brute(lists, weights)) is not None)
        print("twin %-16s wrong on %d of %d cases" % (name, wrong, len(all_cases)))
        assert wrong >= 1, name
