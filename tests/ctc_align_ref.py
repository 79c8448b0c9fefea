"""float64 NumPy statement of the forced-alignment rule of csrc/ctc_align.hip (include/s2t_hip.h: s2t_ctc_align), plus what the tests
need around it: the margin of a case's closest decision, a checker of paths, enumeration of every path for tiny cases, two
deliberately wrong twins, the batch form with the kernel's output layout, and the generators of planted cases (fixed seeds)."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def round_to(x, dtype_name):
    """the f32 array rounded to the kernel's input format (what the reference is fed too)"""
    if dtype_name == "f32":
        return np.asarray(x, dtype=np.float32)
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()


def extended(y, blank):
    """z_s for the S = 2L + 1 states, and which states may take the skip from s - 2"""
    L = len(y)
    z = np.full(2 * L + 1, blank, dtype=np.int64)
    z[1::2] = y
    skip = np.zeros(2 * L + 1, dtype=bool)
    for s in range(3, 2 * L + 1, 2):
        skip[s] = y[(s - 1) // 2] != y[(s - 3) // 2]
    return z, skip


def _margin(a, b):
    """of the decision for a over b (a >= b), relative to the larger value and never to less than 1"""
    if b == NEG:
        return np.inf
    return (a - b) / max(1.0, abs(a))


def viterbi(lp, y, blank, skip_equal=False, end_last_only=False):
    """lp [n, V] float64 log-probabilities, y the transcript.  Returns dict(status 0 / 1, states [n], score = the path's value,
    margin = the smallest relative margin among the predecessor decisions ON the best path and the end decision).
    skip_equal / end_last_only: the two wrong twins (the skip between equal tokens allowed; the path may end in S - 1 only)."""
    lp = np.asarray(lp, dtype=np.float64)
    n, L = lp.shape[0], len(y)
    S = 2 * L + 1
    if n == 0:
        return dict(status=0 if L == 0 else 1, states=np.zeros(0, np.int64), score=0.0 if L == 0 else NEG, margin=np.inf)
    z, skip = extended(list(y), blank)
    if skip_equal:
        skip[3::2] = True

    def step(v):
        a1 = np.concatenate([[NEG], v[:-1]])
        a2 = np.where(skip, np.concatenate([[NEG, NEG], v[:-2]])[:S], NEG)
        best, k = v.copy(), np.zeros(S, np.int8)
        m1 = a1 > best                                                # ties: the higher predecessor, stay over advance over skip
        best[m1], k[m1] = a1[m1], 1
        m2 = a2 > best
        best[m2], k[m2] = a2[m2], 2
        return best, k, a1, a2

    v = np.full(S, NEG)
    v[:2] = lp[0, z[:2]]
    bp = np.zeros((n, S), np.int8)
    for t in range(1, n):
        best, bp[t], _, _ = step(v)
        v = lp[t, z] + best
    e1, e2 = v[S - 1], (v[S - 2] if S >= 2 and not end_last_only else NEG)
    end = S - 2 if e2 > e1 else S - 1
    if not max(e1, e2) > NEG:
        return dict(status=1, states=np.zeros(0, np.int64), score=NEG, margin=np.inf)
    margin = _margin(max(e1, e2), min(e1, e2)) if S >= 2 and not end_last_only else np.inf
    states = np.zeros(n, np.int64)
    states[n - 1] = end
    for t in range(n - 1, 0, -1):
        states[t - 1] = states[t] - bp[t, states[t]]
    v = np.full(S, NEG)                                               # once more, for the margins of the decisions on the path
    v[:2] = lp[0, z[:2]]
    for t in range(1, n):
        best, _, a1, a2 = step(v)
        s = states[t]
        c = sorted([v[s], a1[s], a2[s]], reverse=True)
        margin = min(margin, _margin(c[0], c[1]))
        v = lp[t, z] + best
    return dict(status=0, states=states, score=float(max(e1, e2)), margin=float(margin))


def path_sums(lp, states, y, blank):
    """(score, frames [L][2], tok_score [L]) of a path by float64 sums along it; frames of a token that has none are (-1, -1)"""
    lp = np.asarray(lp, dtype=np.float64)
    L = len(y)
    z, _ = extended(list(y), blank)
    vals = lp[np.arange(len(states)), z[states]]
    frames, tok = np.full((L, 2), -1, np.int64), np.zeros(L)
    for i in range(L):
        at = np.nonzero(states == 2 * i + 1)[0]
        if len(at):
            frames[i] = (at[0], at[-1] + 1)
            tok[i] = vals[at].sum()
    return float(vals.sum()), frames, tok


def is_valid_path(states, y, n):
    """starts in 0 or 1, moves of 0, 1 or an allowed 2, ends in S - 1 or S - 2 (S = 1: in 0)"""
    states = [int(s) for s in states]
    L = len(y)
    S = 2 * L + 1
    if len(states) != n or n == 0:
        return len(states) == n and L == 0
    if states[0] not in (0, 1) or states[0] >= S or states[-1] not in (S - 1, S - 2) or states[-1] < 0:
        return False
    for a, b in zip(states, states[1:]):
        d = b - a
        if d not in (0, 1, 2) or b >= S:
            return False
        if d == 2 and not (b % 2 == 1 and b >= 3 and y[(b - 1) // 2] != y[(b - 3) // 2]):
            return False
    return True


def align(logits, n, y, blank, **twin):
    """the rule on logits [T, V] for one sentence: dict(status, states, score, frames, tok_score, margin, lp)"""
    lp = log_softmax64(np.asarray(logits)[:n]) if n else np.zeros((0, np.asarray(logits).shape[-1]))
    r = viterbi(lp, y, blank, **twin)
    r["lp"] = lp
    if r["status"] == 0:
        r["score"], r["frames"], r["tok_score"] = path_sums(lp, r["states"], y, blank)
    else:
        r["frames"], r["tok_score"] = np.full((len(y), 2), -1, np.int64), np.full(len(y), NEG)
    return r


def all_paths(n, y):
    """every valid path of n frames for y (tiny cases), by extension frame by frame; is_valid_path is the judge of each"""
    S = 2 * len(y) + 1
    if n == 0:
        return [()] if not y else []
    paths = [(s,) for s in (0, 1) if s < S]
    for _ in range(n - 1):
        paths = [p + (s,) for p in paths for s in range(p[-1], min(p[-1] + 3, S))]
    return [p for p in paths if is_valid_path(p, y, n)]


def brute_force(lp, y, blank):
    """(best value, the path the tie rule picks) over every valid path: among paths of equal value, the one whose states read from
    the LAST frame backwards are highest -- what `end in S - 1` and `the higher predecessor wins` amount to"""
    lp = np.asarray(lp, dtype=np.float64)
    z, _ = extended(list(y), blank)
    best, arg = NEG, None
    for p in all_paths(lp.shape[0], y):
        val = float(sum(lp[t, z[s]] for t, s in enumerate(p)))
        if val > best or (val == best and val > NEG and p[::-1] > arg[::-1]):
            best, arg = val, p
    return best, arg


def align_batch(logits, in_len, targets, tgt_len, blank, fill=-7):
    """the kernel's outputs for a batch: logits [T, B, V]; (states [B, T], frames [B, Lmax, 2], tok_score [B, Lmax], score [B],
    status [B]) with `fill` (NaN in tok_score) wherever the rule says "not written" """
    logits, targets = np.asarray(logits), np.asarray(targets)
    T, B, V = logits.shape
    Lmax = targets.shape[1]
    states = np.full((B, T), -1, np.int32)
    frames = np.full((B, Lmax, 2), fill, np.int32)
    tok_score = np.full((B, Lmax), np.nan, np.float32)
    score, status = np.zeros(B, np.float32), np.zeros(B, np.int32)
    for b in range(B):
        n, L = min(max(int(in_len[b]), 0), T), int(tgt_len[b])
        if not 0 <= L <= Lmax:
            status[b], score[b] = 2, NEG
            continue
        y = [int(c) for c in targets[b, :L]]
        if any(c < 0 or c >= V or c == blank for c in y):
            status[b], score[b], frames[b, :L], tok_score[b, :L] = 2, NEG, -1, NEG
            continue
        r = align(logits[:, b], n, y, blank)
        status[b], score[b], frames[b, :L], tok_score[b, :L] = r["status"], r["score"], r["frames"], r["tok_score"]
        if r["status"] == 0:
            states[b, :n] = r["states"]
    return states, frames, tok_score, score, status


# ------------------------------------------------------------------ planted cases
def draw_transcript(rng, L, V, blank, p_repeat=0.2):
    """L non-blank tokens, each repeating its predecessor with probability p_repeat (always, when there is one symbol only)"""
    symbols = [c for c in range(V) if c != blank]
    y = []
    for i in range(L):
        if i and (len(symbols) == 1 or rng.random() < p_repeat):
            y.append(y[-1])
            continue
        c = int(symbols[int(rng.integers(0, len(symbols)))])
        while i and c == y[-1]:
            c = int(symbols[int(rng.integers(0, len(symbols)))])
        y.append(c)
    return y


def min_frames(y):
    """tokens plus the blanks that repeated tokens force: the length at which exactly one path exists"""
    return len(y) + sum(a == b for a, b in zip(y, y[1:]))


def draw_path(rng, y, T):
    """a valid path of T frames: every token at least one frame, required blanks at least one, about half of the optional blank
    slots emptied (so that skips occur), the remaining frames spread multinomially"""
    L = len(y)
    S = 2 * L + 1
    need = np.zeros(S, np.int64)
    need[1::2] = 1
    open_ = np.ones(S, bool)
    for s in range(0, S, 2):
        forced = 0 < s < S - 1 and y[s // 2 - 1] == y[s // 2]
        if forced:
            need[s] = 1
        elif rng.random() < 0.5:
            open_[s] = False
    assert T >= need.sum(), "too few frames for this transcript"
    if L == 0:
        open_[0] = True                                               # the one state there is takes every frame
    counts = need + rng.multinomial(T - need.sum(), open_ / open_.sum())
    path = np.repeat(np.arange(S), counts)
    assert is_valid_path(path, y, T)
    return path


def planted_case(seed, T, V, L, name, bonus=6.0, blank=None, p_repeat=0.2):
    """dict(x [T, V] f32 rounded to `name`, y, path, blank): N(0, 1) logits with `bonus` added along a drawn path"""
    rng = np.random.default_rng(seed)
    blank = V - 1 if blank is None else blank
    y = draw_transcript(rng, L, V, blank, p_repeat)
    path = draw_path(rng, y, T)
    z, _ = extended(y, blank)
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[np.arange(T), z[path]] += bonus
    return dict(x=round_to(x, name), y=y, path=path, blank=blank, T=T, V=V, L=L)


# ------------------------------------------------------------------ the cases that contradict the wrong twins
TWIN_V, TWIN_BLANK = 4, 3


def twin_case_equal_tokens():
    """y = [a, a] on three frames: the one valid path is a, blank, a.  Frame 1 favours a: a twin that skips between equal tokens
    takes a, a, a (states 1, 3, 3) -- which collapses to [a], not to y."""
    x = np.zeros((3, TWIN_V), np.float32)
    x[:, 0] = 5.0
    return x, [0, 0]


def twin_case_ends_in_a_token():
    """the planted path a, a, b, b ends in its last token (state S - 2): the last frame's blank is unlikely"""
    x = np.zeros((4, TWIN_V), np.float32)
    x[[0, 1], 0] = 5.0
    x[[2, 3], 1] = 5.0
    x[:, TWIN_BLANK] = -3.0
    return x, [0, 1]
