#!/usr/bin/env python3
"""Time the BLEU statistics kernel (csrc/bleu_stats.hip: K.bleu_stats) beside a host route on the same inputs, in the same process:

    python tools/bleu_stats_time.py [--rounds 7] [--calls 10] > profiles/bleu_stats.txt

Shapes: B = 16 best hypotheses and a 16 x 5 n-best list (80 hypotheses sharing 16 references through the row map) at padded widths
60 (one wave per sentence) and 200 (one workgroup per sentence), and B = 4 at width 4,095 (the limit).  References are random
sentences over 5,000 symbols that end in eos and are padded; hypotheses are noisy copies of them (one token in ten dropped, one in
ten replaced), so the n-gram matches look like a translation's, not like two unrelated strings.  Tokens are int64, what the search
returns (staged as 64-bit); the int32 form of the same call is timed beside it.
Device figures are device events around `calls` back-to-back calls, per call; "to the sums on the host" figures are wall-clock per
call from the tokens on the device to the ten sums on the host (synchronising).  The host route copies the tokens to the host and
runs the reference's rule there with `collections.Counter`, one sentence at a time.  Rounds alternate between the routes; every
round is printed, then the median.  Needs an MI355X; there is no pass / fail threshold: the routes' sums are compared and the times
reported."""
import argparse
import os
import statistics
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402

PAD, EOS, UNK = 1, 2, 3
SHAPES = [(16, 5, 60), (16, 5, 200), (4, 0, 4095)]          # sentences, n-best (0: none), padded width


def make_case(B, N, width, dev, V=5000):
    """-> (best hyp, its lengths, n-best hyp, its lengths, its row map, ref, ref lengths), int64 on `dev`"""
    rng = np.random.default_rng(17)
    refs = [(4 + rng.integers(0, V, int(rng.integers(width // 2, width)))).tolist() + [EOS] for _ in range(B)]

    def noisy(r):
        h = [t if rng.random() > 0.1 else int(4 + rng.integers(0, V)) for t in r[:-1] if rng.random() > 0.1]
        return h[:width - 1] + [EOS]

    def matrix(rows):
        m = np.full((len(rows), width), PAD, np.int64)
        for s, r in enumerate(rows):
            m[s, :len(r)] = r
        return torch.from_numpy(m).to(dev), torch.tensor([len(r) for r in rows], device=dev)

    best = [noisy(r) for r in refs]
    nbest = [h if k == 0 else noisy(r) for r, h in zip(refs, best) for k in range(N)]
    rows = torch.tensor([b for b in range(B) for _ in range(N)], dtype=torch.int32, device=dev)
    return matrix(best) + (matrix(nbest) if N else (None, None)) + (rows,) + matrix(refs)


def host_stats(hyp, hyp_len, ref, ref_len, rows=None):
    """the rule on host tensors, a sentence at a time: trim, then a Counter per order -> the ten sums"""
    hyp, hyp_len, ref, ref_len = hyp.tolist(), hyp_len.tolist(), ref.tolist(), ref_len.tolist()
    rows = range(len(hyp)) if rows is None else rows.tolist()
    sums = [0] * 10

    def trim(t):
        a = 0
        while a < len(t) and t[a] == PAD:
            a += 1
        t = t[a:]
        e = len(t) - 1
        while e > 0 and t[e] in (EOS, PAD):
            e -= 1
        return t[:e + 1]

    for s, r in enumerate(rows):
        h, x = trim(hyp[s][:hyp_len[s]]), trim(ref[r][:ref_len[r]])
        sums[0] += len(x)
        sums[1] += len(h)
        for n in range(1, 5):
            hc = Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
            rc = Counter(tuple(x[i:i + n]) for i in range(len(x) - n + 1) if UNK not in x[i:i + n])
            sums[2 * n] += sum(min(c, rc[g]) for g, c in hc.items())
            sums[2 * n + 1] += max(len(h) - n + 1, 0)
    return sums


def device_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def wall_time(fn, calls):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e6 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bleu_stats_time.py measures on the GPU"
    print("device:", torch.cuda.get_device_name(0))
    print("pad %d, eos %d, unk %d; rounds %d x %d calls, alternating; us per call" % (PAD, EOS, UNK, a.rounds, a.calls))
    for B, N, width in SHAPES:
        best, best_len, nb, nb_len, rows, ref, ref_len = make_case(B, N, width, "cuda")
        lists = [("%d best hypotheses" % B, best, best_len, None)] + ([("%d x %d n-best" % (B, N), nb, nb_len, rows)] if N else [])
        for what, hyp, hyp_len, row in lists:
            h32, n32, r32, m32 = hyp.int(), hyp_len.int(), ref.int(), ref_len.int()
            device = lambda: K.bleu_stats(hyp, hyp_len, ref, ref_len, PAD, EOS, UNK, ref_row=row)
            device32 = lambda: K.bleu_stats(h32, n32, r32, m32, PAD, EOS, UNK, ref_row=row)
            device_sums = lambda: device()[0].sum(0).tolist()
            host_sums = lambda: host_stats(hyp.cpu(), hyp_len.cpu(), ref.cpu(), ref_len.cpu(), None if row is None else row.cpu())
            one, two = device_sums(), host_sums()
            print("width %d, %s (hypotheses %d .. %d tokens, references %d .. %d): match %s of count %s; the routes' sums are equal: %s"
                  % (width, what, int(hyp_len.min()), int(hyp_len.max()), int(ref_len.min()), int(ref_len.max()), one[2::2], one[3::2],
                     one == two == device32()[0].sum(0).tolist()))
            routes = [("device  K.bleu_stats, int64 tokens", device_time, device),
                      ("device  K.bleu_stats, int32 tokens", device_time, device32),
                      ("to the sums on the host  K.bleu_stats, ten sums copied", wall_time, device_sums),
                      ("to the sums on the host  tokens.cpu() + Counter loop", wall_time, host_sums)]
            for _, _, fn in routes:
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            times = [[] for _ in routes]
            for _ in range(a.rounds):
                for i, (_, timer, fn) in enumerate(routes):
                    times[i].append(timer(fn, a.calls))
            med = [statistics.median(ts) for ts in times]
            for (tag, _, _), ts, m in zip(routes, times, med):
                print("  %-58s %s -> median %.1f us" % (tag, " ".join("%.1f" % v for v in ts), m))
            print("  host route / device call, both to the sums on the host: %.2f x" % (med[3] / med[2]))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
