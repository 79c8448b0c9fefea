"""Restatement (numpy) of the draw of the sampling search (include/s2t_hip.h `s2t_sample_rows`, csrc/sample.hpp), independent of the
package's own host code (fbk_fairseq_st_amd/sampling.py): the hash and the uniform bit for bit in Python integers / uint64 arrays, the
Gumbel keys, the kept sets and the arg-max in float64 -- so a device result is held against exact arithmetic, and a draw or a kept set
that hangs on an f32 rounding is NAMED (near tie, near boundary) instead of being compared.

Also `sent_step_sample`: the SAMPLE form of dec_sent_kernel on decode_ref's host state -- `beam` candidates, candidate r = slot r's
draw with parent slot r (slot 0 at step 0), then the bookkeeping of decode_ref.sent_step.
"""
import numpy as np

M32 = 0xFFFFFFFF
NEAR_TIE = 1e-4          # keys lie in (-40, 40): the f32 errors of logf(logf) and of the log-softmax are a few ulp of 64, ~1e-5
NEAR_P = 1e-5            # relative distance of a boundary mass from P under which the f32 sums may fall on either side


def _mix(x):
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def _mix_int(x):
    x ^= x >> 16; x = (x * 0x7feb352d) & M32
    x ^= x >> 15; x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def row_key(key, step, slot):
    lo, hi = key & M32, (key >> 32) & M32
    a = _mix_int(lo ^ 0x9E3779B9); a = _mix_int((a + hi) & M32); a = _mix_int((a + step) & M32); a = _mix_int((a + slot) & M32)
    b = _mix_int(hi ^ 0x85EBCA6B); b = _mix_int((b + lo) & M32); b = _mix_int((b + slot) & M32); b = _mix_int((b + step) & M32)
    return a, b


def hash32(key, step, slot, cols):
    """uint32 [len(cols)]: the hash of (key, step, slot, column)"""
    a, b = row_key(int(key), int(step), int(slot))
    c = np.asarray(cols, np.int64).astype(np.uint64)
    return _mix((_mix(c ^ np.uint64(a)) + np.uint64(b)) & np.uint64(M32)).astype(np.uint32)


def hash32_scalar(key, step, slot, col):
    a, b = row_key(int(key), int(step), int(slot))
    return _mix_int((_mix_int((int(col) & M32) ^ a) + b) & M32)


def uniform(h):
    """(2k + 1) * 2^-24 with k = h >> 9, in float64 (exactly the f32 value)"""
    return ((h >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def kept_set(lp, topk, topp):
    """lp [V] (f32 values) -> (bool [V] kept, near): order value descending, column ascending; topp > 0 first (kept iff the float64
    mass strictly before the column is < P), else topk > 0, else all; finite columns only.  near: a top-p boundary lies within
    NEAR_P * P of P (the size of the set may then differ by one in f32)."""
    lp = np.asarray(lp, np.float64)
    V = lp.shape[0]
    order = sorted((c for c in range(V) if lp[c] > -np.inf), key=lambda c: (-lp[c], c))
    keep = np.zeros(V, bool)
    near = False
    if topp > 0:
        P = float(np.float32(topp))
        before = 0.0
        for c in order:
            near = near or abs(before - P) <= NEAR_P * P
            if not before < P:
                break
            keep[c] = True
            before += float(np.exp(lp[c]))
    elif topk > 0:
        keep[order[:int(topk)]] = True
    else:
        keep[order] = True
    return keep, near


def draw(lp, keep, key, step, slot):
    """-> (token, second, gap): the arg-max of the float64 keys over the kept columns (the smaller column on ties), the runner-up and
    the distance between their keys (inf with fewer than two kept columns).  Nothing kept: (0, None, inf)."""
    cols = np.nonzero(keep)[0]
    if cols.size == 0:
        return 0, None, np.inf
    u = uniform(hash32(key, step, slot, cols))
    k = np.asarray(lp, np.float64)[cols] - np.log(-np.log(u))
    o = sorted(range(cols.size), key=lambda i: (-k[i], cols[i]))
    if cols.size == 1:
        return int(cols[o[0]]), None, np.inf
    return int(cols[o[0]]), int(cols[o[1]]), float(k[o[0]] - k[o[1]])


def sample_rows(lprobs, draws, topk, topp, key, step):
    """s2t_sample_rows: lprobs [rows, V] -> dict(tok [rows, draws], second (-1 = none), gap, n_kept [rows], near_p bool [rows])"""
    rows = lprobs.shape[0]
    out = dict(tok=np.zeros((rows, draws), np.int64), second=np.full((rows, draws), -1, np.int64), gap=np.full((rows, draws), np.inf),
               n_kept=np.zeros(rows, np.int64), near_p=np.zeros(rows, bool), keep=[])
    for r in range(rows):
        keep, near = kept_set(lprobs[r], topk, topp)
        out["n_kept"][r], out["near_p"][r] = int(keep.sum()), near
        out["keep"].append(keep)
        for j in range(draws):
            t, s, g = draw(lprobs[r], keep, key, step, r * draws + j)
            out["tok"][r, j], out["gap"][r, j] = t, g
            if s is not None:
                out["second"][r, j] = s
    return out


def sent_step_sample(st, cand_val, cand_tok, beam, eos, max_len):
    """One launch of the SAMPLE form of dec_sent_kernel on host state `st` (decode_ref.new_state's arrays, modified in place).
    cand_val float32 [N] / cand_tok [N]: slot n's draw (score = lp[token] + its cumulative score).  The bookkeeping of
    decode_ref.sent_step with k = beam candidates in slot order."""
    B = st["steps"].shape[0]
    for s in range(B):
        n0 = s * beam
        t = int(st["steps"][s])
        if t > max_len:
            continue
        k = beam
        val = [np.float32(cand_val[n0 + r]) for r in range(k)]
        tok = [int(cand_tok[n0 + r]) for r in range(k)]
        row = [n0 if t == 0 else n0 + r for r in range(k)]
        bl = [bool(st["blacklist"][n0 + i]) for i in range(beam)]
        done = bool(st["finished"][s])
        nf = int(st["nfin"][s])
        eosm = [tok[i] == eos and val[i] != -np.inf and not bl[i] for i in range(k)]
        nm = 0
        for i in range(k):
            if eosm[i] and not done:
                slot = nf + nm
                nm += 1
                if slot < beam:
                    st["fin_step"][s, slot], st["fin_row"][s, slot], st["fin_score"][s, slot] = t, row[i], val[i]
        nf_new = min(beam, nf + nm)
        st["nfin"][s] = nf_new
        if nm and (nf_new == beam or t == max_len):
            st["finished"][s] = 1
        eosm = [eosm[i] or bl[i] for i in range(k)]
        pick = [i for i in range(k) if not eosm[i]] + [i for i in range(k) if eosm[i]]
        for place, i in enumerate(pick):
            st["tok_hist"][t + 1, n0 + place] = tok[i]
            st["par_hist"][t + 1, n0 + place] = row[i]
            st["cum_hist"][t + 1, n0 + place] = val[i]
            st["blacklist"][n0 + place] = 1 if eosm[i] else 0
        if t < max_len:
            old = st["anc"][n0:n0 + beam, :t].copy()
            for j, i in enumerate(pick):
                st["anc"][n0 + j, :t] = old[row[i] - n0]
                st["anc"][n0 + j, t] = row[i]
        st["steps"][s] = t + 1


# ------------------------------------------------------------------ the same, all rows at once (numpy; the GPU tests' large shapes)
def _mix_u32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def hash32_rows(key, step, slots, V):
    """uint32 [len(slots), V]: row i holds the hashes of (key, step, slots[i], 0 .. V-1); uint32 arithmetic wraps as the device's does"""
    ab = np.array([row_key(int(key), int(step), int(s)) for s in slots], dtype=np.uint32).reshape(-1, 2)
    c = np.arange(V, dtype=np.uint32)[None, :]
    return _mix_u32(_mix_u32(c ^ ab[:, :1]) + ab[:, 1:])


class Rows:
    """lprobs [R, V] (f32 values) sorted once (value descending, column ascending); kept sets and draws in float64"""

    def __init__(self, lprobs):
        self.lp = np.asarray(lprobs, np.float64)
        self.R, self.V = self.lp.shape
        self.order = np.argsort(-self.lp, axis=1, kind="stable")
        self.sorted = np.take_along_axis(self.lp, self.order, 1)

    def kept(self, topk, topp):
        """-> (keep bool [R, V], near bool [R], margin [R]): near = a cumulative mass lies within NEAR_P * P of P; margin = the distance
        of P from the closest cumulative mass (inf without top-p)"""
        fin = self.sorted > -np.inf
        near, margin = np.zeros(self.R, bool), np.full(self.R, np.inf)
        if topp > 0:
            P = float(np.float32(topp))
            p = np.exp(self.sorted)
            before = np.cumsum(p, 1) - p
            ks = (before < P) & fin
            dist = np.where(fin, np.abs(before - P), np.inf)
            margin = dist.min(1)
            near = margin <= NEAR_P * P
        elif topk > 0:
            ks = (np.arange(self.V)[None, :] < int(topk)) & fin
        else:
            ks = fin
        keep = np.zeros((self.R, self.V), bool)
        np.put_along_axis(keep, self.order, ks, 1)
        return keep, near, margin

    def gumbel(self, key, step, slots):
        return -np.log(-np.log(uniform(hash32_rows(key, step, slots, self.V))))

    def draw(self, keep, g):
        """-> (tok [R], second [R] (-1 = none), gap [R]) for the Gumbel variates g [R, V] of the rows' slots"""
        k = np.where(keep, self.lp + g, -np.inf)
        r = np.arange(self.R)
        tok = np.argmax(k, 1)                                     # the first of equal maxima: the smaller column
        best = k[r, tok].copy()
        k[r, tok] = -np.inf
        sec = np.argmax(k, 1)
        sv = k[r, sec]
        none = ~keep.any(1)
        tok[none] = 0
        second = np.where(sv > -np.inf, sec, -1)
        with np.errstate(invalid="ignore"):                       # (-inf) - (-inf) where nothing is kept
            gap = np.where(sv > -np.inf, best - sv, np.inf)
        return tok, second, gap
