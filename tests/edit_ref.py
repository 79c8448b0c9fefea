"""The edit-distance alignment rule of include/s2t_hip.h (s2t_edit_align) in plain Python, for the tests.

`align(a, b, costs)` fills the whole matrix with the direction of every cell and walks back from (n, m): cost, counts (M, S, B, A)
and the path's step codes in forward order (0 M, 1 S, 2 B, 3 A).  `align_np` is the same rule swept by anti-diagonals with numpy,
for the large cases.  `carried(a, b, costs)` carries the counts forward with the costs, the way the kernel does, without a matrix of
directions.  The wrong twins differ from the rule in one decision each; the tests assert that their comparisons tell them apart.
"""
import numpy as np

M, S, B, A = 0, 1, 2, 3


def _table(a, b, costs, up_first=False, non_strict=False):
    cs, ca, cb = costs
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    step = [[M] * (m + 1) for _ in range(n + 1)]
    less = (lambda x, y: x <= y) if non_strict else (lambda x, y: x < y)
    for j in range(1, m + 1):
        D[0][j], step[0][j] = D[0][j - 1] + cb, B
    for i in range(1, n + 1):
        D[i][0], step[i][0] = D[i - 1][0] + ca, A
        for j in range(1, m + 1):
            eq = a[i - 1] == b[j - 1]
            best, st = D[i - 1][j - 1] + (0 if eq else cs), (M if eq else S)
            moves = ((D[i][j - 1] + cb, B), (D[i - 1][j] + ca, A))
            for val, code in (moves[::-1] if up_first else moves):
                if less(val, best):
                    best, st = val, code
            D[i][j], step[i][j] = best, st
    return D, step


def _walk(step, n, m):
    ops, i, j = [], n, m
    while i > 0 or j > 0:
        st = step[i][j]
        ops.append(st)
        i -= st != B
        j -= st != A
    ops.reverse()
    return ops


def _result(D, step, n, m):
    ops = _walk(step, n, m)
    return int(D[n][m]), tuple(ops.count(k) for k in range(4)), ops


def align(a, b, costs=(1, 1, 1)):
    """(cost, (M, S, B, A), ops) by the rule"""
    a, b = [int(x) for x in a], [int(x) for x in b]
    D, step = _table(a, b, costs)
    return _result(D, step, len(a), len(b))


def carried(a, b, costs=(1, 1, 1)):
    """(cost, (M, S, B, A)) with the counts carried forward beside the costs: no direction is stored, nothing is walked"""
    cs, ca, cb = costs
    a, b = [int(x) for x in a], [int(x) for x in b]
    m = len(b)
    row = [(j * cb, (0, 0, j, 0)) for j in range(m + 1)]
    bump = lambda c, k: tuple(v + (q == k) for q, v in enumerate(c))
    for i in range(1, len(a) + 1):
        new = [(i * ca, (0, 0, 0, i))]
        for j in range(1, m + 1):
            eq = a[i - 1] == b[j - 1]
            best = (row[j - 1][0] + (0 if eq else cs), bump(row[j - 1][1], M if eq else S))
            if new[j - 1][0] + cb < best[0]:
                best = (new[j - 1][0] + cb, bump(new[j - 1][1], B))
            if row[j][0] + ca < best[0]:
                best = (row[j][0] + ca, bump(row[j][1], A))
            new.append(best)
        row = new
    return row[m]


def align_np(a, b, costs=(1, 1, 1)):
    """the rule swept by anti-diagonals (cells i + j = d depend on d - 1 and d - 2 only); same result as align()"""
    cs, ca, cb = costs
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    n, m = len(a), len(b)
    D = np.zeros((n + 1, m + 1), np.int64)
    step = np.zeros((n + 1, m + 1), np.uint8)
    D[0, :] = np.arange(m + 1) * cb
    step[0, 1:] = B
    D[:, 0] = np.arange(n + 1) * ca
    step[1:, 0] = A
    for d in range(2, n + m + 1):
        i = np.arange(max(1, d - m), min(n, d - 1) + 1)
        j = d - i
        eq = a[i - 1] == b[j - 1]
        best = D[i - 1, j - 1] + np.where(eq, 0, cs)
        st = np.where(eq, M, S).astype(np.uint8)
        left = D[i, j - 1] + cb
        take = left < best
        best, st = np.where(take, left, best), np.where(take, B, st)
        up = D[i - 1, j] + ca
        take = up < best
        best, st = np.where(take, up, best), np.where(take, A, st)
        D[i, j], step[i, j] = best, st
    return _result(D, step, n, m)


# ---------------------------------------------------------------------------------------------- the wrong twins
def twin_up_first(a, b, costs=(1, 1, 1)):
    """up is tried before left"""
    D, step = _table([int(x) for x in a], [int(x) for x in b], costs, up_first=True)
    return _result(D, step, len(a), len(b))


def twin_non_strict(a, b, costs=(1, 1, 1)):
    """`<=` where the rule has `<`: the later candidate wins ties"""
    D, step = _table([int(x) for x in a], [int(x) for x in b], costs, non_strict=True)
    return _result(D, step, len(a), len(b))


def twin_swapped(a, b, costs=(1, 1, 1)):
    """ca and cb change places"""
    return align(a, b, (costs[0], costs[2], costs[1]))


def twin_levenshtein_counts(a, b, costs=(1, 1, 1)):
    """the right cost, but the counts and the path of the (1, 1, 1) alignment"""
    cost = align(a, b, costs)[0]
    _, counts, ops = align(a, b, (1, 1, 1))
    return cost, counts, ops


TWINS = {"up before left": twin_up_first, "non-strict comparisons": twin_non_strict, "ca and cb swapped": twin_swapped,
         "counts of a Levenshtein path": twin_levenshtein_counts}


# ---------------------------------------------------------------------------------------------- helpers of the tests
def collapse(frames, blank):
    """repeats collapsed, then the blank dropped (s2t_host_ctc_uer's greedy path)"""
    out, prev = [], None
    for t, x in enumerate(int(v) for v in frames):
        if (t == 0 or x != prev) and x != blank:
            out.append(x)
        prev = x
    return out


def replay(a, b, ops):
    """True when the steps consume a and b entirely and M / S sit on equal / different tokens"""
    i = j = 0
    for st in ops:
        if st in (M, S):
            if i >= len(a) or j >= len(b) or (int(a[i]) == int(b[j])) != (st == M):
                return False
            i, j = i + 1, j + 1
        elif st == B:
            j += 1
        elif st == A:
            i += 1
        else:
            return False
    return i == len(a) and j == len(b)


def edit_align_batch(a, a_len, b, b_len, costs=(1, 1, 1), collapse_blank=None, want_ops=False):
    """kernels.edit_align on numpy arrays: (counts, cost, status, a_n, a_out, ops, n_ops), zeros where the kernel writes nothing
    that a caller may look at"""
    a, b = np.asarray(a), np.asarray(b)
    Bn, Amax, Bmax = a.shape[0], a.shape[1], b.shape[1]
    counts, cost = np.zeros((Bn, 4), np.int32), np.zeros((Bn,), np.int32)
    status, a_n = np.zeros((Bn,), np.int32), np.zeros((Bn,), np.int32)
    a_out = np.zeros((Bn, Amax), a.dtype) if collapse_blank is not None else None
    ops = np.zeros((Bn, Amax + Bmax), np.uint8) if want_ops else None
    n_ops = np.zeros((Bn,), np.int32) if want_ops else None
    for s in range(Bn):
        n, m = int(a_len[s]), int(b_len[s])
        if not (0 <= n <= Amax and 0 <= m <= Bmax):
            status[s] = 2
            continue
        row = [int(x) for x in a[s, :n]]
        if collapse_blank is not None:
            row = collapse(row, collapse_blank)
            a_out[s, :len(row)] = row
        a_n[s] = len(row)
        c, cnt, path = align_np(row, b[s, :m], costs)
        cost[s], counts[s] = c, cnt
        if want_ops:
            ops[s, :len(path)] = path
            n_ops[s] = len(path)
    return counts, cost, status, a_n, a_out, ops, n_ops
