"""Kaldi's LinearResample as torchaudio.compliance.kaldi.resample_waveform restates it (include/s2t_hip.h, s2t_resample, states the
rule), in float64 numpy: the bank, the lengths, the resampling; a float32 restatement that sums sequentially as the kernel does; and
wrong twins of the rule.  No torchaudio result is stored anywhere: compatibility rests on this restatement.

The comparison of tests/test_resample_gpu.py: per output, |y - y64| <= (taps + 4) 2^-24 S[k] with S[k] = sum_j |w x| over the
float64 weights and taps the bank's widest tap count -- the dot-product bound for any summation order, and one rounding each for the
weight, the input conversion and the store.  `units` is that error in 2^-24 S[k]."""
import math
from fractions import Fraction

import numpy as np

PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 8000), (11, 10), (9, 10), (48000, 44100)]
QUOTED = {(48000, 16000): (1, 37, 37, 37), (44100, 16000): (160, 33, 34, 5440), (22050, 16000): (320, 16, 17, 5440),
          (8000, 16000): (2, 12, 13, 26), (16000, 8000): (1, 25, 25, 25), (11, 10): (10, 13, 14, 140), (9, 10): (10, 12, 13, 130),
          (48000, 44100): (147, 13, 14, 2058)}       # phases, fewest taps, most taps, weights (phases x most taps)

TWINS = {"rolloff_1": dict(rolloff=1.0), "width_5": dict(width=5), "first_off_by_one": dict(first_shift=1),
         "outermost_tap_dropped": dict(drop_outer=True), "length_floor_plus_1": dict(floor_len=True),
         "junk_behind_n": dict(junk=True), "not_divided_by_orig": dict(no_div=True)}


def reduce_pair(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def bank(orig, new, width=6, rolloff=0.99, first_shift=0, drop_outer=False, no_div=False, **_):
    """(in_unit, out_unit, first int64 [out_unit], count int64 [out_unit], w float64 [out_unit, taps] zero behind a phase's count)"""
    orig, new = reduce_pair(orig, new)
    cutoff = rolloff * 0.5 * min(orig, new)
    ww = width / (2.0 * cutoff)
    first = np.zeros(new, np.int64)
    count = np.zeros(new, np.int64)
    rows = []
    for i in range(new):
        t = i / new
        f, l = math.ceil((t - ww) * orig), math.floor((t + ww) * orig)
        row = []
        for j in range(l - f + 1):
            d = (f + j) / orig - t
            s = 2.0 * cutoff if d == 0.0 else math.sin(2.0 * math.pi * cutoff * d) / (math.pi * d)
            w = 0.5 * (1.0 + math.cos(2.0 * math.pi * cutoff / width * d)) * s
            row.append((w if no_div else w / orig) if abs(d) < ww else 0.0)
        if drop_outer:                                  # the outermost non-zero tap on the right
            nz = [j for j, w in enumerate(row) if w != 0.0]
            row[nz[-1]] = 0.0
        first[i], count[i] = f + first_shift, len(row)
        rows.append(row)
    w = np.zeros((new, int(count.max())))
    for i, row in enumerate(rows):
        w[i, :len(row)] = row
    return orig, new, first, count, w


def num_samples(n, orig, new, floor_len=False, **_):
    orig, new = reduce_pair(orig, new)
    return n * new // orig + 1 if floor_len else -((-n * new) // orig)


def brute_samples(n, orig, new):
    """the count of k with k / new < n / orig, by exact fractions"""
    k = 0
    while Fraction(k, new) < Fraction(n, orig):
        k += 1
    return k


def _gather(x, n, first, in_unit, out_unit, taps, m, junk):
    """xs [m, taps]: the samples under every output's taps, 0 outside [0, n) (a twin reads what lies behind n in the row)"""
    k = np.arange(m, dtype=np.int64)
    idx = (first[k % out_unit] + (k // out_unit) * in_unit)[:, None] + np.arange(taps, dtype=np.int64)[None, :]
    hi = len(x) if junk else n
    inside = (idx >= 0) & (idx < hi)
    return np.where(inside, np.asarray(x, dtype=np.float64)[np.clip(idx, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0), k % out_unit


def resample(x, n, orig, new, dtype=np.float64, **twin):
    """the first n samples of the row x (int16 or float32; what lies behind n is the row's padding) -> (y [m], S [m]): the rule in
    `dtype`.  float64: a numpy sum.  float32: weights rounded once, a sequential fused sum from 0 in ascending j."""
    orig, new = reduce_pair(orig, new)
    m = num_samples(n, orig, new, **twin)
    if orig == new:
        y = np.asarray(x[:n], dtype=np.float64)
        return y.astype(dtype), np.abs(y)
    in_unit, out_unit, first, _, w = bank(orig, new, **twin)
    xs, phase = _gather(x, n, first, in_unit, out_unit, w.shape[1], m, twin.get("junk", False))
    wk = w[phase]
    S = np.abs(wk * xs).sum(1)
    if dtype == np.float64:
        return (wk * xs).sum(1), S
    w32 = wk.astype(np.float32).astype(np.float64)
    acc = np.zeros(m, np.float32)
    for j in range(w.shape[1]):                         # a float64 product of two float32 plus a float32, rounded once: fmaf
        acc = (w32[:, j] * xs[:, j] + acc.astype(np.float64)).astype(np.float32)
    return acc, S


def units(y, y64, S):
    """|y - y64| in units of 2^-24 S[k]; where S is 0 the rule gives exactly 0"""
    err = np.abs(np.asarray(y, dtype=np.float64) - y64)
    return np.where(S > 0, err / np.where(S > 0, S * 2.0 ** -24, 1.0), np.where(err > 0, np.inf, 0.0))


def allowed(orig, new, **twin):
    """taps + 4 for the bank's widest tap count"""
    if reduce_pair(orig, new)[0] == reduce_pair(orig, new)[1]:
        return 4.0
    return float(bank(orig, new, **twin)[4].shape[1] + 4)


def within(y, x, n, orig, new):
    """the comparison: y has the rule's length and every element is within the bound (a NaN is not)"""
    y64, S = resample(x, n, orig, new)
    if len(y) != len(y64):
        return False
    return bool((units(y, y64, S) <= allowed(orig, new)).all())


def impulse_expected(x, n, orig, new, **twin):
    """what a row with at most one non-zero sample under every output must give, exactly: float32(float32(w) * x), the product
    itself being exact in float64 (24 + 15 bits).  Asserts that the row is such a row."""
    in_unit, out_unit, first, _, w = bank(orig, new, **twin)
    m = num_samples(n, orig, new, **twin)
    xs, phase = _gather(x, n, first, in_unit, out_unit, w.shape[1], m, twin.get("junk", False))
    assert ((xs != 0).sum(1) <= 1).all()
    return (w[phase].astype(np.float32).astype(np.float64) * xs).sum(1).astype(np.float32)


def impulse_rows(orig, new, dtype, n=None):
    """rows with +-32767 on a comb of spacing >= the widest tap count, shifted by one sample per row over a whole period: every
    (phase, tap) pair meets a non-zero sample, and no output more than one.  Returns (rows [P, n], n)."""
    in_unit, out_unit, first, count, w = bank(orig, new)
    taps = w.shape[1]
    period = taps + 1
    if n is None:
        n = max(2 * in_unit + 3 * period, 12 * period) + 5
    rows = np.zeros((period, n), dtype=dtype)
    for s in range(period):
        pos = np.arange(s, n, period)
        rows[s, pos] = np.where((pos // period) % 2 == 0, 32767, -32767)
    return rows, n
