"""A plain CTC forward-backward in numpy, the reference of tests/test_ctc_loss_elements_gpu.py, and the element bound of that test.

One utterance at a time, nothing clever: rows are log-softmaxed, the extended target carries blanks at the even positions, alpha and
beta run in the log domain with the maximum subtracted at every step (the subtracted offsets are summed in Python floats, so the
vectors stay near zero whatever the frame count), the s-2 skip is allowed only for a unit that differs from the unit two back, and
the posteriors of a frame are normalised by their own sum.  `dtype` lets the same code run in float32: tests/test_ctc_ref_cpu.py uses
that run to show that the bound below can be met by f32 arithmetic, and deliberately wrong variants to show that it cannot be met by
a wrong recursion.  The pieces (extended_target, utterance_posteriors, occupancy) are separate functions so that those variants can
be put together from them.
"""
import math

import numpy as np

LN2 = math.log(2.0)


def log_softmax(x):
    m = x.max(-1, keepdims=True)
    return x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))


def extended_target(units, blank):
    """ext[S] (blank, u1, blank, u2, ..., blank) and skip[S]: position s may be entered from s-2 (a unit that differs from the unit
    two positions back; blanks never)"""
    L = len(units)
    ext = np.full(2 * L + 1, blank, dtype=np.int64)
    ext[1::2] = units
    skip = np.zeros(2 * L + 1, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    return ext, skip


def _lse3(a, b, c):
    m = np.maximum(np.maximum(a, b), c)
    m0 = np.where(np.isfinite(m), m, 0).astype(a.dtype)
    return m0 + np.log(np.exp(a - m0) + np.exp(b - m0) + np.exp(c - m0))


def utterance_posteriors(lp, ext, skip):
    """lp [Tb, V] log-probabilities of the utterance's frames (Tb >= 1) -> (nll as a Python float, post [Tb, S] in lp's dtype: the
    posterior of position s at frame t, every frame summing to 1); (inf, zeros) when no alignment exists"""
    dt = lp.dtype
    Tb, S = lp.shape[0], len(ext)
    em = lp[:, ext]                                                  # [Tb, S]
    never = np.full(2, -np.inf, dtype=dt)
    a = np.full(S, -np.inf, dtype=dt)
    a[0] = 0
    alpha = np.empty((Tb, S), dtype=dt)
    off = 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in range(Tb):
            p = np.concatenate([never, a])
            a = _lse3(a, p[1:-1], np.where(skip, p[:-2], -np.inf).astype(dt)) + em[t]      # alpha_-1 = delta(s = 0): one ordinary step
            m = a.max()
            if not np.isfinite(m):
                return math.inf, np.zeros((Tb, S), dtype=dt)
            a = a - m
            off += float(m)
            alpha[t] = a
        tail = a[-2:] if S >= 2 else a[-1:]
        mt = tail.max()
        if not np.isfinite(mt):
            return math.inf, np.zeros((Tb, S), dtype=dt)
        nll = -(off + float(mt) + math.log(float(np.exp(tail - mt).sum())))
        b = np.full(S, -np.inf, dtype=dt)
        b[-1] = 0
        skip_to = np.concatenate([skip, np.zeros(2, dtype=bool)])[2:]    # s may go to s+2
        for t in range(Tb - 1, -1, -1):
            p = np.concatenate([b, never])
            b = _lse3(b, p[1:-1], np.where(skip_to, p[2:], -np.inf).astype(dt)) + em[t]    # beta_t includes frame t's emission
            b = b - b.max()
            w = alpha[t] + b - em[t]
            w = np.exp(w - w[np.isfinite(w)].max())
            alpha[t] = w / w.sum()
    return nll, alpha


def occupancy(post, ext, V):
    """post [Tb, S] -> [Tb, V]: the posterior mass of every column"""
    out = np.zeros((post.shape[0], V), dtype=post.dtype)
    for t in range(post.shape[0]):
        out[t] = np.bincount(ext, weights=post[t], minlength=V)
    return out


def ctc_forward_backward(logits, targets, in_len, tgt_len, blank, dtype=np.float64):
    """logits [T, B, V], targets [B, Lmax], in_len / tgt_len [B] -> nll [B] float64 (inf where no alignment exists or in_len <= 0),
    occ [T, B, V] (posterior mass per column, 0 outside the utterance and where nll is inf) and softmax [T, B, V], both `dtype`"""
    x = np.asarray(logits).astype(dtype)
    T, B, V = x.shape
    lp = log_softmax(x)
    sm = np.exp(lp)
    occ = np.zeros((T, B, V), dtype=dtype)
    nll = np.full(B, math.inf)
    for b in range(B):
        Tb = min(int(in_len[b]), T)
        if Tb <= 0:
            continue
        ext, skip = extended_target(np.asarray(targets[b][: int(tgt_len[b])], dtype=np.int64), blank)
        nll[b], post = utterance_posteriors(lp[:Tb, b], ext, skip)
        if math.isfinite(nll[b]):
            occ[:Tb, b] = occupancy(post, ext, V)
    return nll, occ, sm


def live_mask(nll, in_len, T):
    """[T, B] bool: the rows that carry a gradient (t < min(in_len, T) and a finite nll)"""
    tb = np.minimum(np.asarray(in_len, dtype=np.int64), T)
    return (np.arange(T)[:, None] < tb[None, :]) & np.isfinite(np.asarray(nll))[None, :]


def gradient(nll, occ, sm, in_len):
    """d(sum of the finite nll) / d logits: softmax - occ on the live rows, else 0"""
    return np.where(live_mask(nll, in_len, occ.shape[0])[:, :, None], sm - occ, 0)


# ------------------------------------------------------------------ the bound of the element test
# a(Tb): the absolute error budget of alpha + beta in the log domain, which becomes a relative error of every posterior.  The
# kernels' recursion works in f32 on the hardware exp2 / log2 units with about 2^-20 of absolute error per step; a takes twice that
# over the Tb steps the alpha and the beta of one frame span together, plus 2^-15 for the f32 rounding of one emission.
# 2^-18 softmax: the hardware exp2 and the f32 log-sum-exp of the row.  2^-22: posteriors that underflow in f32.
# A_COEF: the kernels' "about 2^-20 per step" holds for values of magnitude below 16.  The recursion's vectors are kept relative to
# their MAXIMUM, and the states that carry the posterior can lie far below it: thousands of log2 units in a tight alignment (4,096
# units in 4,200 frames: the best unfinished prefix lags far behind the path that must finish), where one f32 ulp is 2^-12, and
# ~480 when the transcript's columns sit 80 below the rest (four emissions of -120 between two shifts).  This module's own float32
# run, which subtracts the maximum at every step and uses libm, needs 1.9 (columns lowered by 80) and 1.2 (4,096 units) times the
# coefficient-1 bound there, and 1.3 times its nll bound at 1,500 units in 1,520 frames; the kernels measured 2.55 and 1.43 on an
# MI355X.  So the coefficient is 4, the most the derivation's slack admits; tests/test_ctc_ref_cpu.py still finds every wrong
# reference more than 190 times outside.
A_COEF = 4.0


def a_of(Tb, coef=A_COEF):
    return coef * LN2 * (np.asarray(Tb, dtype=np.float64) * 2.0 ** -19 + 2.0 ** -15)


def grad_bound(occ, sm, g_ref, in_len, gs, r, coef=A_COEF):
    """element bound of gs * g_ref: gs (a(Tb) occ + 2^-18 softmax + 2^-22) + r gs |g_ref|, [T, B, V] float64; a(Tb) = coef ln 2
    (Tb 2^-19 + 2^-15)"""
    T = occ.shape[0]
    a = a_of(np.clip(np.asarray(in_len, dtype=np.int64), 0, T), coef)[None, :, None]
    return gs * (a * np.asarray(occ, dtype=np.float64) + 2.0 ** -18 * np.asarray(sm, dtype=np.float64) + 2.0 ** -22) + r * gs * np.abs(g_ref)


def nll_bound(nll_ref, in_len, T):
    """a(Tb) + 2^-23 |ref| per utterance (meaningful where the reference is finite)"""
    ref = np.asarray(nll_ref, dtype=np.float64)
    return a_of(np.clip(np.asarray(in_len, dtype=np.int64), 0, T)) + 2.0 ** -23 * np.where(np.isfinite(ref), np.abs(ref), 0.0)
