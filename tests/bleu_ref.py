"""The BLEU statistics rule of include/s2t_hip.h (s2t_bleu_stats) in plain Python, twice: the Counter form, which is how the
reference's libbleu states it (a map of n-grams of the hypothesis, decremented by the reference's n-grams), and the position-wise
form the kernel uses (hypothesis position i matches at order n iff the number of earlier positions with the same n-gram is below
the number of reference positions with it).  Plus the arithmetic of the reference's Scorer (bleu.py:100-129) on the ten sums, the
smoothed sentence score, and wrong twins of the rule that the tests must tell from it."""
import math
from collections import Counter

import numpy as np

ORDERS = (1, 2, 3, 4)
FIELDS = ("reflen", "predlen", "match1", "count1", "match2", "count2", "match3", "count3", "match4", "count4")


class _Never:
    """what a reference `unk` becomes: equal to nothing, itself included (bleu.py:83-86 writes -999, ids are never negative there)"""
    __slots__ = ()

    def __eq__(self, other):
        return False

    def __hash__(self):
        return id(self)


def trim(tokens, pad, eos):
    """leading pads dropped; then trailing eos / pad dropped, never the first remaining token; empty after the left trim -> []"""
    t = [int(x) for x in tokens]
    start = 0
    while start < len(t) and t[start] == pad:
        start += 1
    t = t[start:]
    if not t:
        return t
    end = len(t) - 1
    while end > 0 and t[end] in (eos, pad):
        end -= 1
    return t[:end + 1]


def _sides(hyp, ref, pad, eos, unk):
    h, r = trim(hyp, pad, eos), trim(ref, pad, eos)
    if unk >= 0:
        r = [_Never() if x == unk else x for x in r]
    return h, r


def _grams(t, n):
    return [tuple(t[i:i + n]) for i in range(len(t) - n + 1)]


def stats_counter(hyp, ref, pad, eos, unk=-1):
    """the ten numbers of one pair in the order of FIELDS"""
    h, r = _sides(hyp, ref, pad, eos, unk)           # an empty side has length 0 and no matches: the documented deviation
    out = [len(r), len(h)]
    for n in ORDERS:
        left = Counter(_grams(h, n))
        match = 0
        for g in _grams(r, n):
            if left[g] > 0:
                match += 1
                left[g] -= 1
        out += [match, max(len(h) - n + 1, 0)]
    return out


def stats_positional(hyp, ref, pad, eos, unk=-1):
    h, r = _sides(hyp, ref, pad, eos, unk)
    out = [len(r), len(h)]
    for n in ORDERS:
        hg, rg = _grams(h, n), _grams(r, n)
        match = 0
        for i, g in enumerate(hg):
            rank = sum(1 for k in range(i) if hg[k] == g)
            cref = sum(1 for x in rg if x == g)
            match += rank < cref
        out += [match, max(len(h) - n + 1, 0)]
    return out


def bleu_stats_batch(hyp, hyp_len, ref, ref_len, pad, eos, unk=-1, ref_row=None, rule=stats_counter):
    """what kernels.bleu_stats returns, on numpy operands: (stats int32 [B, 10], status int32 [B]); a sentence with a length
    outside [0, width] or a ref_row entry outside [0, rows) is refused: status 2, zeros"""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    B = hyp.shape[0]
    stats, status = np.zeros((B, 10), np.int32), np.zeros((B,), np.int32)
    for b in range(B):
        row = b if ref_row is None else int(ref_row[b])
        if not 0 <= row < ref.shape[0]:
            status[b] = 2
            continue
        n, m = int(hyp_len[b]), int(ref_len[row])
        if not (0 <= n <= hyp.shape[1] and 0 <= m <= ref.shape[1]):
            status[b] = 2
            continue
        stats[b] = rule(hyp[b, :n], ref[row, :m], pad, eos, unk)
    return stats, status


# ---------------------------------------------------------------------------------------------- the Scorer's arithmetic
def _ratio(a, b):
    return a / b if b > 0 else 0


def precisions(s):
    return [_ratio(s[2 + 2 * k], s[3 + 2 * k]) for k in range(4)]


def brevity(s):
    return min(1, math.exp(1 - s[0] / s[1]))


def score(s, order=4):
    """bleu.py:100-103 on ten sums (predlen > 0)"""
    psum = sum(math.log(p) if p > 0 else float("-Inf") for p in precisions(s)[:order])
    return brevity(s) * math.exp(psum / order) * 100


def result_string(s, order=4):
    """bleu.py:120-129 on ten sums"""
    fmt = "BLEU{} = {:2.2f}, {:2.1f}"
    for _ in range(1, order):
        fmt += "/{:2.1f}"
    fmt += " (BP={:.3f}, ratio={:.3f}, syslen={}, reflen={})"
    bleup = [p * 100 for p in precisions(s)[:order]]
    return fmt.format(order, score(s, order), *bleup, brevity(s), s[1] / s[0], s[1], s[0])


def sentence_bleu(s):
    """the smoothed sentence score: the Scorer after reset(one_init=True) and one add -- orders 2 to 4 start from match = count = 1;
    0 for an empty hypothesis"""
    s = [int(x) for x in s]
    if s[1] == 0:
        return 0.0
    t = list(s)
    for k in (1, 2, 3):
        t[2 + 2 * k] += 1
        t[3 + 2 * k] += 1
    return score(t)


# ---------------------------------------------------------------------------------------------- wrong twins
def _twin(clip="both", unk_matches=False, do_trim=True, keep_first=True):
    def rule(hyp, ref, pad, eos, unk=-1):
        if do_trim:
            h, r = trim(hyp, pad, eos), trim(ref, pad, eos)
            if not keep_first:
                h = [] if h and h[-1] in (eos, pad) else h
                r = [] if r and r[-1] in (eos, pad) else r
        else:
            h, r = [int(x) for x in hyp], [int(x) for x in ref]
        if unk >= 0 and not unk_matches:
            r = [_Never() if x == unk else x for x in r]
        out = [len(r), len(h)]
        for n in ORDERS:
            hc, rc = Counter(_grams(h, n)), Counter(_grams(r, n))
            if clip == "both":
                match = sum(min(c, rc[g]) for g, c in hc.items())
            elif clip == "none":                      # every reference n-gram that occurs in the hypothesis at all
                match = sum(c for g, c in rc.items() if hc[g] > 0)
            else:                                     # "hyp": every hypothesis n-gram that occurs in the reference at all
                match = sum(c for g, c in hc.items() if rc[g] > 0)
            out += [match, max(len(h) - n + 1, 0)]
        return out
    return rule


TWINS = {
    "unclipped matches": _twin(clip="none"),
    "unk allowed to match": _twin(unk_matches=True),
    "no trim": _twin(do_trim=False),
    "trim to length 0": _twin(keep_first=False),
    "clip by the hypothesis count only": _twin(clip="hyp"),
}
