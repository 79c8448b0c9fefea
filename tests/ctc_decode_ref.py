"""float64 NumPy statement of the two CTC decoding rules of csrc/ctc_decode.hip (include/s2t_hip.h: s2t_ctc_greedy,
s2t_ctc_prefix_beam), keyed by token tuples, plus what the tests need around it: the per-case tie margin, the detector of a pruned
prefix re-created under a live child, a deliberately WRONG twin that identifies a prefix by the entry it came from, the brute-force
marginals, a plain Levenshtein distance and the random-case generator."""
import itertools

import numpy as np

NEG = -np.inf


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))


def lae(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    return float(np.logaddexp(a, b))


# ------------------------------------------------------------------ greedy
def collapse(pred, blank):
    """runs of equal predictions collapse, blanks drop: [(token, first frame, one past the last frame)]"""
    out, t, n = [], 0, len(pred)
    while t < n:
        e = t
        while e < n and pred[e] == pred[t]:
            e += 1
        if pred[t] != blank:
            out.append((int(pred[t]), t, e))
        t = e
    return out


def greedy(logits, n, blank):
    """logits [T, V], n frames count.  Returns (tokens, frames [(first, end)], tok_score, score)"""
    x = np.asarray(logits[:n], dtype=np.float64)
    if n == 0:
        return [], [], [], 0.0
    lp = log_softmax64(x)
    pred = x.argmax(-1)                                              # the first index of the maximum
    best = lp[np.arange(n), pred]
    runs = collapse(pred, blank)
    return ([r[0] for r in runs], [(r[1], r[2]) for r in runs], [float(best[r[1]:r[2]].sum()) for r in runs], float(best.sum()))


# ------------------------------------------------------------------ prefix beam search
def candidates(row, blank, cand):
    """the cand non-blank symbols of highest logit, ties to the lower index"""
    order = np.argsort(-np.asarray(row, dtype=np.float64), kind="stable")
    return [int(j) for j in order if j != blank][:cand]


def _rank(new):
    items = [(k, v, lae(*v)) for k, v in new.items()]
    items = [it for it in items if it[2] > NEG]                      # probability zero: no prefix
    items.sort(key=lambda it: -it[2])
    return items


def _gap(items, keep):
    """relative distance between the last kept and the first dropped total"""
    if len(items) <= keep:
        return np.inf
    a, b = items[keep - 1][2], items[keep][2]
    return (a - b) / max(1.0, abs(a))


def prefix_beam(logits, n, blank, beam, cand, nbest=1):
    """Hannun et al. 2014 without a language model; a prefix IS its token tuple.
    Returns dict(hyps=[(tokens tuple, total)] best first (at most nbest), gap=smallest relative margin of any keep / drop decision
    and of the order of the written hypotheses, recreated=whether a pruned prefix came back while a child of it was live,
    totals={tuple: total} of the final survivors)"""
    x = np.asarray(logits[:n], dtype=np.float64)
    lp = log_softmax64(x) if n else x
    live = {(): (0.0, NEG)}
    gap, recreated = np.inf, False
    for t in range(n):
        C = candidates(x[t], blank, cand)
        new = {}

        def add(key, pb, pnb):
            a, b = new.get(key, (NEG, NEG))
            new[key] = (lae(a, pb), lae(b, pnb))
        for p, (pb, pnb) in live.items():
            tot = lae(pb, pnb)
            add(p, lp[t, blank] + tot, NEG)
            for c in C:
                if p and c == p[-1]:
                    add(p, NEG, lp[t, c] + pnb)
                    add(p + (c,), NEG, lp[t, c] + pb)
                else:
                    add(p + (c,), NEG, lp[t, c] + tot)
        items = _rank(new)
        gap = min(gap, _gap(items, beam))
        kept = items[:beam]
        names = {k for k, _, _ in kept}
        for k in names:
            if k not in live and any(q[:-1] == k for q in live if q):      # k is new, survives, and a child of it was live
                recreated = True
        live = {k: v for k, v, _ in kept}
    final = _rank(live)
    for i in range(1, min(nbest, len(final)) + 1):                   # the order of what is written, and the cut behind it
        gap = min(gap, _gap(final, i))
    return dict(hyps=[(k, tot) for k, _, tot in final[:nbest]], gap=gap, recreated=recreated, totals={k: tot for k, _, tot in final})


def prefix_beam_by_parent(logits, n, blank, beam, cand, nbest=1):
    """The WRONG twin: an entry is identified by (the entry it was extended from, the token), looked up among the live entries only.
    A prefix that was pruned and comes back from its own parent gets a new identity, so its extension no longer meets the child
    that stayed live: the string is then held twice and its probability is split."""
    x = np.asarray(logits[:n], dtype=np.float64)
    lp = log_softmax64(x) if n else x
    live = {0: dict(parent=-1, tok=-1, s=(), pb=0.0, pnb=NEG)}      # id -> entry
    next_id = 1
    for t in range(n):
        C = candidates(x[t], blank, cand)
        new = {}

        def add(key, proto, pb, pnb):
            e = new.setdefault(key, dict(proto, pb=NEG, pnb=NEG))
            e["pb"], e["pnb"] = lae(e["pb"], pb), lae(e["pnb"], pnb)
        for i, p in live.items():
            tot = lae(p["pb"], p["pnb"])
            add(i, p, lp[t, blank] + tot, NEG)
            for c in C:
                child = next((j for j, q in live.items() if q["parent"] == i and q["tok"] == c), None)
                key = child if child is not None else ("new", i, c)
                proto = live[child] if child is not None else dict(parent=i, tok=c, s=p["s"] + (c,))
                if p["s"] and c == p["s"][-1]:
                    add(i, p, NEG, lp[t, c] + p["pnb"])
                    add(key, proto, NEG, lp[t, c] + p["pb"])
                else:
                    add(key, proto, NEG, lp[t, c] + tot)
        items = [(k, e, lae(e["pb"], e["pnb"])) for k, e in new.items()]
        items = sorted((it for it in items if it[2] > NEG), key=lambda it: -it[2])[:beam]
        live = {}
        for k, e, _ in items:
            if not isinstance(k, int):
                k, next_id = next_id, next_id + 1
            live[k] = e
    final = sorted(((e["s"], lae(e["pb"], e["pnb"])) for e in live.values()), key=lambda it: -it[1])
    return dict(hyps=final[:nbest])


def brute_force_marginals(logits, blank):
    """{token tuple: log of the summed probability of all V^T alignments that collapse to it} (tiny T and V only)"""
    lp = log_softmax64(logits)
    T, V = lp.shape
    out = {}
    for path in itertools.product(range(V), repeat=T):
        s = tuple(r[0] for r in collapse(path, blank))
        out[s] = lae(out.get(s, NEG), float(sum(lp[t, v] for t, v in enumerate(path))))
    return out


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        row = [i]
        for j, y in enumerate(b, 1):
            row.append(min(prev[j] + 1, row[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = row
    return prev[-1]


# ------------------------------------------------------------------ random cases
def random_case(seed):
    """peaky logits: randn x {1, 3, 6} per segment, every segment held for 1 to 3 frames, 0.3 noise on top, rounded to f32.
    Returns dict(x f32 [T, V], T, V, blank, beam, cand)"""
    rng = np.random.default_rng(1000 + seed)
    T = int(rng.integers(5, 81))
    V = int(rng.choice([6, 12, 33, 100]))
    beam = int(rng.choice([1, 2, 4, 8, 16]))
    cand = min(int(rng.choice([1, 2, 4, 8])), V - 1)
    scale = float(rng.choice([1, 3, 6]))
    blank = int(rng.integers(0, V))
    rows = []
    while len(rows) < T:
        rows += [rng.standard_normal(V) * scale] * int(rng.integers(1, 4))
    x = (np.stack(rows[:T]) + 0.3 * rng.standard_normal((T, V))).astype(np.float32)
    return dict(x=x, T=T, V=V, blank=blank, beam=beam, cand=cand)


GPU_SEEDS = tuple(range(60))          # the seeds tests/test_ctc_decode_gpu.py runs; test_ctc_decode_ref_cpu.py holds them to its conditions
MIN_GAP = 1e-5                        # cases whose closest keep / drop decision is nearer than this (relative) are skipped by name
MAX_SKIPPED = 0.15                    # of GPU_SEEDS
# Rounded to bf16 the logits lie on a grid of 8-bit mantissas, equal DIFFERENCES of two logits in two frames are common, and with
# them prefixes of exactly equal probability (`a` then `b` against `b` then `a`): a third of the seeds above has a tie in float64
# itself.  The bf16 run therefore draws 90 seeds, so that as many cases stay as the f32 run keeps at its worst (85 % of 60).
GPU_SEEDS_BF16 = tuple(range(90))
MIN_KEPT_BF16 = 51


_REFS = {}


def case_reference(seed, dtype_name):
    """(case, rounded logits, reference result, wrong twin's result) of one generator seed, all beam hypotheses asked for; computed
    once per process and left unchanged"""
    key = (seed, dtype_name)
    if key not in _REFS:
        c = random_case(seed)
        x = round_to(c["x"], dtype_name)
        _REFS[key] = (c, x, prefix_beam(x, c["T"], c["blank"], c["beam"], c["cand"], nbest=c["beam"]),
                      prefix_beam_by_parent(x, c["T"], c["blank"], c["beam"], c["cand"], nbest=c["beam"]))
    return _REFS[key]


def same_hyps(a, b, rel=1e-9):
    return ([h[0] for h in a] == [h[0] for h in b] and all(abs(p[1] - q[1]) <= rel * max(1.0, abs(p[1])) for p, q in zip(a, b)))


def round_to(x, dtype_name):
    """the f32 array rounded to the kernel's input format (what the reference is fed too)"""
    if dtype_name == "f32":
        return np.asarray(x, dtype=np.float32)
    import torch
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).bfloat16().float().numpy()
