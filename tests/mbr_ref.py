"""Minimum-Bayes-risk selection over n-best lists in plain Python, on top of tests/bleu_ref.py: what kernels.bleu_pairs writes (the ten
statistics of every candidate against every pseudo-reference of its sentence, by `stats_counter`, with the refusals of
include/s2t_hip.h s2t_bleu_pairs), and what MBRDecoder.expected_bleu makes of it (utilities by `sentence_bleu`, gains and the
first-best in Python float64).  Plus wrong twins of the selection that the tests must tell from it."""
import numpy as np

import bleu_ref as R


def pair_stats(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, M=None, rule=R.stats_counter, swap=False):
    """-> (stats int32 [Rc, M, 10], status int32 [Rc, M]) on numpy operands.  Refused (status 2, zeros): a pair whose pseudo-reference
    length lies outside [0, Pmax]; every pair of a candidate whose length lies outside [0, Hmax]; all M entries of a candidate whose
    sentence lies outside [0, B) or whose sentence's offsets descend, leave [0, Rr] or span more than M rows.  Behind a list: zeros."""
    cand, ref = np.asarray(cand), np.asarray(ref)
    Rc, Hmax, Rr, Pmax, B = cand.shape[0], cand.shape[1], ref.shape[0], ref.shape[1], len(ref_off) - 1
    if M is None:
        M = max([min(max(int(ref_off[b + 1]) - int(ref_off[b]), 0), 256) for b in range(B)] + [0])
    stats, status = np.zeros((Rc, M, 10), np.int32), np.zeros((Rc, M), np.int32)
    for c in range(Rc):
        lst = list_of(int(cand_sent[c]), ref_off, Rr, M)
        if lst is None:
            status[c, :] = 2
            continue
        lo, n = lst
        h = int(cand_len[c])
        if not 0 <= h <= Hmax:
            status[c, :n] = 2
            continue
        for k in range(n):
            m = int(ref_len[lo + k])
            if not 0 <= m <= Pmax:
                status[c, k] = 2
                continue
            a, b = cand[c, :h], ref[lo + k, :m]
            stats[c, k] = rule(b, a, pad, eos, unk) if swap else rule(a, b, pad, eos, unk)
    return stats, status


def list_of(sent, ref_off, Rr, M):
    """(first row, rows) of a sentence's list, None when it has none"""
    if not 0 <= sent < len(ref_off) - 1:
        return None
    lo, hi = int(ref_off[sent]), int(ref_off[sent + 1])
    if lo < 0 or hi < lo or hi > Rr or hi - lo > M:
        return None
    return lo, hi - lo


def select(stats, status, cand_len, Hmax, cand_sent, ref_off, Rr, weights=None, skip_self=False, last_on_ties=False, mean=True):
    """-> (utility [Rc][M], gain [Rc], best [B]) as Python floats and ints.  weights: one number per pseudo-reference row, None for
    ones.  gain = sum_k w U / sum_k w over the pairs with status 0 inside the list; 0 without such weight; -1 for a refused
    candidate.  best: the first candidate row of the sentence's highest gain, -1 without candidates.  The keywords are the twins'."""
    Rc, M = status.shape
    B = len(ref_off) - 1
    utility = [[R.sentence_bleu(stats[c, k]) for k in range(M)] for c in range(Rc)]
    gain = []
    for c in range(Rc):
        lst = list_of(int(cand_sent[c]), ref_off, Rr, M)
        if lst is None or not 0 <= int(cand_len[c]) <= Hmax:
            gain.append(-1.0)
            continue
        lo, n = lst
        num = den = 0.0
        for k in range(n):
            if status[c, k] != 0 or (skip_self and lo + k == c):
                continue
            w = 1.0 if weights is None else float(weights[lo + k])
            num += w * utility[c][k]
            den += w
        gain.append((num / den if mean else num) if den > 0 else 0.0)
    best = []
    for b in range(B):
        rows = [c for c in range(Rc) if int(cand_sent[c]) == b]
        if not rows:
            best.append(-1)
            continue
        top = max(gain[c] for c in rows)
        tied = [c for c in rows if gain[c] == top]
        best.append(tied[-1] if last_on_ties else tied[0])
    return utility, gain, best


def expected_bleu(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk=-1, weights=None, M=None, twin=None):
    """what MBRDecoder.expected_bleu returns, as numpy integers and Python floats; twin: a key of TWINS"""
    kw = dict(TWINS[twin]) if twin else {}
    swap = kw.pop("swap", False)
    if kw.pop("no_weights", False):
        weights = None
    stats, status = pair_stats(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk, M, swap=swap)
    utility, gain, best = select(stats, status, cand_len, np.asarray(cand).shape[1], cand_sent, ref_off, np.asarray(ref).shape[0], weights, **kw)
    return {"stats": stats, "status": status, "utility": utility, "gain": gain, "best": best}


def matrices(lists, width=None, dtype=np.int64, fill=0):
    """token lists per sentence -> (matrix, lengths, sentence of each row, offsets)"""
    rows = [t for ts in lists for t in ts]
    width = max([len(t) for t in rows] + [0]) if width is None else width
    mat = np.full((len(rows), width), fill, dtype)
    for i, t in enumerate(rows):
        mat[i, :len(t)] = t
    sent = np.array([b for b, ts in enumerate(lists) for _ in ts], np.int32)
    off = np.cumsum([0] + [len(ts) for ts in lists]).astype(np.int32)
    return mat, np.array([len(t) for t in rows], dtype), sent, off


def rank_lists(hyps, pad, eos, unk=-1, pseudo=None, weights=None, twin=None):
    """hyps: per sentence a list of token lists; pseudo: the same shape of pseudo-references, None for hyps itself; weights: None or
    per sentence a list of numbers.  -> per sentence (gains in the list's order, the stable order by descending gain)"""
    same = pseudo is None
    pseudo = hyps if same else pseudo
    cand, cand_len, cand_sent, _ = matrices(hyps)
    ref, ref_len, _, ref_off = (cand, cand_len, None, matrices(hyps)[3]) if same else matrices(pseudo)
    w = None if weights is None else [x for ws in weights for x in ws]
    if twin == "self" and not same:
        raise ValueError("the self pair exists only when the lists are judged against themselves")
    got = expected_bleu(cand, cand_len, cand_sent, ref, ref_len, ref_off, pad, eos, unk, w, twin=twin)
    out, at = [], 0
    for ts in hyps:
        g = got["gain"][at:at + len(ts)]
        out.append((g, sorted(range(len(ts)), key=lambda k: -g[k])))
        at += len(ts)
    return out


# ---------------------------------------------------------------------------------------------- wrong twins
TWINS = {
    "roles swapped": dict(swap=True),                 # the pseudo-reference as the hypothesis of the pair
    "self": dict(skip_self=True),                     # the self pair left out (rows of one matrix judged against themselves)
    "weights ignored": dict(no_weights=True),
    "last on ties": dict(last_on_ties=True),
    "sum": dict(mean=False),                          # gain as a sum: differs from the mean's order under ragged lists
}
