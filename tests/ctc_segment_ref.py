"""float64 NumPy statement of the segmentation rule of csrc/ctc_segment.hip (include/s2t_hip.h: s2t_ctc_segment), built on
tests/ctc_align_ref.py: the recursion with the two free ends, the utterance outputs, a path checker, enumeration of every path for tiny
cases, the generators of planted recordings (fixed seeds), the bounds, and three deliberately wrong twins:
  * `charge_free`: the free states charged lp[blank] (the flags ignored);
  * `span_from_blanks`: an utterance's span taken from the blanks around it instead of from its token frames;
  * `window_leaves_span`: the sliding window allowed to run past the span's end."""
import numpy as np

import ctc_align_ref as A

NEG = A.NEG
is_valid_path = A.is_valid_path


def emissions(lp, y, blank, free_start=True, free_end=True):
    """em [n, S]: what state s costs on frame t -- lp_t[z_s], 0 for the free outer blank states"""
    lp = np.asarray(lp, dtype=np.float64)
    z, _ = A.extended(list(y), blank)
    em = lp[:, z].copy()
    if free_start:
        em[:, 0] = 0.0
    if free_end:
        em[:, len(z) - 1] = 0.0
    return em


def viterbi(lp, y, blank, free_start=True, free_end=True, charge_free=False):
    """lp [n, V] float64, y the L >= 1 concatenated tokens.  dict(status 0 / 1, states [n], score, em)"""
    if charge_free:
        free_start = free_end = False
    L, n = len(y), np.asarray(lp).shape[0]
    S = 2 * L + 1
    em = emissions(lp, y, blank, free_start, free_end)
    fail = dict(status=1, states=np.zeros(0, np.int64), score=NEG, em=em)
    if n == 0:
        return fail
    _, skip = A.extended(list(y), blank)
    v = np.full(S, NEG)
    v[:2] = em[0, :2]
    bp = np.zeros((n, S), np.int8)
    for t in range(1, n):
        a1 = np.concatenate([[NEG], v[:-1]])
        a2 = np.where(skip, np.concatenate([[NEG, NEG], v[:-2]])[:S], NEG)
        best, k = v.copy(), np.zeros(S, np.int8)
        m1 = a1 > best                                                # ties: stay over advance over skip
        best[m1], k[m1] = a1[m1], 1
        m2 = a2 > best
        best[m2], k[m2] = a2[m2], 2
        bp[t] = k
        v = em[t] + best
    e1, e2 = v[S - 1], v[S - 2]
    if not max(e1, e2) > NEG:
        return fail
    states = np.zeros(n, np.int64)
    states[n - 1] = S - 2 if e2 > e1 else S - 1
    for t in range(n - 1, 0, -1):
        states[t - 1] = states[t] - bp[t, states[t]]
    return dict(status=0, states=states, score=float(max(e1, e2)), em=em)


def path_values(em, states):
    """the path's emission on every frame"""
    return em[np.arange(len(states)), np.asarray(states, dtype=np.int64)]


def values_on_path(lp, states, y, blank, free_start=True, free_end=True):
    """path_values without the [n, S] matrix, for recordings of many tokens"""
    lp, states = np.asarray(lp, dtype=np.float64), np.asarray(states, dtype=np.int64)
    z, _ = A.extended(list(y), blank)
    vals = lp[np.arange(len(states)), z[states]]
    if free_start:
        vals[states == 0] = 0.0
    if free_end:
        vals[states == len(z) - 1] = 0.0
    return vals


def sums_of_values(vals, states, L):
    """(score, frames [L][2], tok_score [L]) of a path by float64 sums of its per-frame emissions"""
    states = np.asarray(states, dtype=np.int64)
    frames, tok = np.full((L, 2), -1, np.int64), np.zeros(L)
    change = np.nonzero(np.diff(states))[0] + 1
    for a, b in zip(np.concatenate([[0], change]), np.concatenate([change, [len(states)]])):
        s = states[a]
        if s & 1:
            frames[s >> 1] = (a, b)
            tok[s >> 1] = vals[a:b].sum()
    return float(vals.sum()), frames, tok


def path_sums(em, states, L):
    return sums_of_values(path_values(em, states), states, L)


def utterances(vals, states, utt_end, window, n=None, span_from_blanks=False, window_leaves_span=False):
    """per utterance (frames [U][2], score [U], conf_mean [U], conf_min [U]) from the path's per-frame emissions `vals`"""
    states = np.asarray(states, dtype=np.int64)
    n = len(states) if n is None else n
    U = len(utt_end)
    fr, sc, mean, low = np.zeros((U, 2), np.int64), np.zeros(U), np.zeros(U), np.zeros(U)
    for u in range(U):
        i0, i1 = (utt_end[u - 1] if u else 0), utt_end[u] - 1
        s_lo, s_hi = (2 * i0, 2 * i1 + 2) if span_from_blanks else (2 * i0 + 1, 2 * i1 + 1)
        at = np.nonzero((states >= s_lo) & (states <= s_hi))[0]
        f0, f1 = int(at[0]), int(at[-1]) + 1
        fr[u], sc[u], mean[u] = (f0, f1), vals[f0:f1].sum(), vals[f0:f1].sum() / (f1 - f0)
        if window_leaves_span:
            low[u] = min(vals[s:min(s + window, n)].mean() for s in range(f0, f1))
        elif f1 - f0 < window:
            low[u] = mean[u]
        else:
            c = np.concatenate([[0.0], np.cumsum(vals[f0:f1])])     # float64: the difference of two prefix sums is exact enough
            low[u] = (c[window:] - c[:-window]).min() / window
    return fr, sc, mean, low


def segment(logits, n, utts, blank, window=30, free_start=True, free_end=True, **twin):
    """the rule for one recording: logits [T, V], utts a list of token lists.  dict(status, states, score, frames, tok_score,
    utt_frames, utt_score, utt_conf_mean, utt_conf_min, em, lp)"""
    y = [int(c) for u in utts for c in u]
    utt_end = np.cumsum([len(u) for u in utts])
    lp = A.log_softmax64(np.asarray(logits)[:n]) if n else np.zeros((0, np.asarray(logits).shape[-1]))
    r = viterbi(lp, y, blank, free_start, free_end, charge_free=twin.get("charge_free", False))
    r["lp"] = lp
    if r["status"] == 0:
        r["score"], r["frames"], r["tok_score"] = path_sums(r["em"], r["states"], len(y))
        r["utt_frames"], r["utt_score"], r["utt_conf_mean"], r["utt_conf_min"] = utterances(
            path_values(r["em"], r["states"]), r["states"], utt_end, window, span_from_blanks=twin.get("span_from_blanks", False),
            window_leaves_span=twin.get("window_leaves_span", False))
    return r


def brute_force(em, y):
    """(best value, the path the tie rule picks) over every valid path, values summed in frame order as the recursion sums them:
    among paths of equal value the one whose states read from the LAST frame backwards are highest"""
    best, arg = NEG, None
    for p in A.all_paths(em.shape[0], list(y)):
        val = em[0, p[0]]
        for t in range(1, len(p)):
            val = em[t, p[t]] + val
        if val > best or (val == best and val > NEG and p[::-1] > arg[::-1]):
            best, arg = float(val), p
    return best, arg


# ------------------------------------------------------------------ bounds
def bound_short(x):
    """n <= 2,048: the project's 1e-4, relative to max(1, |x|)"""
    return 1e-4 * max(1.0, abs(x))


def bound_u(n, vals):
    """longer sums: a sequential f32 sum of n terms carries up to (n - 1) 2^-24 sum|x|; 8 more for the f32 log-sum-exp and the
    subtraction.  vals: the emissions summed"""
    return (n + 8) * 2.0 ** -24 * float(np.maximum(1.0, np.abs(vals)).sum())


# ------------------------------------------------------------------ planted recordings
def split_utterances(rng, L, U):
    """U >= 1 utterance lengths that sum to L, each at least 1"""
    cuts = np.sort(rng.choice(np.arange(1, L), size=U - 1, replace=False)) if U > 1 else np.zeros(0, np.int64)
    return np.diff(np.concatenate([[0], cuts, [L]])).astype(np.int64).tolist()


def draw_free_path(rng, y, T, pre, post):
    """a valid path of T frames that spends `pre` frames in state 0 and `post` in state S - 1, and the frames between as
    ctc_align_ref.draw_path spreads them -- except that the first and the last token get ONE frame each: with free ends a second
    frame of theirs is worth less than another free frame, so no other path is the best one"""
    L = len(y)
    S = 2 * L + 1
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    open_ = np.ones(S, bool)
    open_[[0, 1, S - 2, S - 1]] = False
    for s in range(2, S - 1, 2):
        if y[s // 2 - 1] == y[s // 2]:
            need[s] = 1
        elif rng.random() < 0.5:
            open_[s] = False
    rest = T - pre - post - need.sum()
    assert rest >= 0, "too few frames for this transcript"
    counts = need.copy()
    if open_.any():
        counts += rng.multinomial(rest, open_ / open_.sum())
    else:
        pre += rest
    counts[0], counts[S - 1] = pre, post
    path = np.repeat(np.arange(S), counts)
    assert A.is_valid_path(path, y, T)
    return path


def planted_recording(seed, T, V, L, U, name, pre, post, bonus=8.0, p_repeat=0.2):
    """dict(x [T, V] f32 rounded to `name`, utts, y, path, blank): N(0, 1) logits with `bonus` added along the text part of a drawn
    path; the `pre` frames before and the `post` frames after the text stay noise"""
    rng = np.random.default_rng(seed)
    blank = V - 1
    y = A.draw_transcript(rng, L, V, blank, p_repeat)
    path = draw_free_path(rng, y, T, pre, post)
    z, _ = A.extended(y, blank)
    x = rng.standard_normal((T, V)).astype(np.float32)
    text = (path > 0) & (path < 2 * L)
    x[np.nonzero(text)[0], z[path[text]]] += bonus
    lens = split_utterances(rng, L, U)
    ends = np.cumsum(lens)
    utts = [y[e - c:e] for e, c in zip(ends, lens)]
    return dict(x=A.round_to(x, name), utts=utts, y=y, path=path, blank=blank, T=T, V=V, L=L)
