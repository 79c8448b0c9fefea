#!/usr/bin/env python3
"""Time the chrF statistics kernel (csrc/chrf_stats.hip: K.chrf_stats) beside a host route on the same inputs, in the same process:

    python tools/chrf_time.py [--rounds 7] [--calls 10] > profiles/chrf.txt

Dictionary: 5,000 synthetic sentencepiece-style symbols of 2 to 6 lower-case letters (about 4 characters a piece), four in ten
starting a word.  References are random rows that end in eos; hypotheses are noisy copies (one token in ten dropped, one in ten
replaced).  Shapes: 16 best hypotheses at padded width 60; a 16 x 5 n-best list (the list shares its references through the row
map); MBR lists of 16 x 32 and 16 x 64 hypotheses judged against themselves (every pair of a sentence through the two row maps, one
matrix as both sides: 16,384 and 65,536 pairs); and 4 rows near the character limit.  chrF (6, 0) and chrF++ (6, 2) are timed.
Device figures are device events around `calls` back-to-back calls, per call, as Python makes the call; "to the sums on the host"
figures are wall-clock per call from the tokens on the device to the 24 sums on the host (synchronising).  The host route copies the
tokens to the host and runs tests/chrf_ref.py there: `Dictionary.string` per row, then one Counter per side and order, each row's
tables computed once per call.  Rounds alternate between the routes; every round is printed, then the median; the host route of the
MBR shapes runs once per round.  Needs an MI355X; there is no pass / fail threshold: the routes' sums are compared and the times
reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import chrf_ref as R  # noqa: E402
from fbk_fairseq_st_amd import chrf_scorer as CS  # noqa: E402
from fbk_fairseq_st_amd import kernels as K  # noqa: E402
from fbk_fairseq_st_amd.data import Dictionary  # noqa: E402

BPE = "sentencepiece"


def make_dictionary(n=5000):
    rng = np.random.default_rng(11)
    d = Dictionary()
    while len(d) < n + 4:
        s = "".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 7))))
        d.add_symbol(("▁" if rng.random() < 0.4 else "") + s)
    return d


def make_rows(d, B, N, lo, hi, seed=17):
    """-> (references, best hypotheses, n-best hypotheses) as token lists"""
    rng = np.random.default_rng(seed)
    refs = [(4 + rng.integers(0, len(d) - 4, int(rng.integers(lo, hi)))).tolist() + [d.eos()] for _ in range(B)]

    def noisy(r):
        return [t if rng.random() > 0.1 else int(4 + rng.integers(0, len(d) - 4)) for t in r[:-1] if rng.random() > 0.1] + [d.eos()]
    best = [noisy(r) for r in refs]
    nbest = [h if k == 0 else noisy(r) for r, h in zip(refs, best) for k in range(N)]
    return refs, best, nbest


def matrix(rows, width, pad, dev):
    m = np.full((len(rows), width), pad, np.int64)
    for s, r in enumerate(rows):
        m[s, :len(r)] = r
    return torch.from_numpy(m).to(dev), torch.tensor([len(r) for r in rows], device=dev)


def host_sums(d, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, wo):
    """copy, Dictionary.string, the Counter loop -> the 24 sums"""
    R.side_counts.cache_clear()
    hyp, hyp_len, ref, ref_len = hyp.cpu().tolist(), hyp_len.cpu().tolist(), ref.cpu().tolist(), ref_len.cpu().tolist()
    ht = [R.text_of(d, h[:n], BPE, False) for h, n in zip(hyp, hyp_len)]
    rt = [R.text_of(d, r[:n], BPE, True) for r, n in zip(ref, ref_len)]
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else len(ht)
    hr = range(P) if hyp_row is None else hyp_row.cpu().tolist()
    rr = range(P) if ref_row is None else ref_row.cpu().tolist()
    sums = [0] * 24
    for i, j in zip(hr, rr):
        for k, v in enumerate(R.pair_stats(ht[i], rt[j], 6, wo)):
            sums[k] += v
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
    assert torch.cuda.is_available(), "chrf_time.py measures on the GPU"
    dev = "cuda"
    print("device:", torch.cuda.get_device_name(0))
    d = make_dictionary()
    table = CS.piece_table(d, BPE)
    pieces, off = torch.from_numpy(table["pieces"].view(np.int32).copy()).to(dev), torch.from_numpy(table["piece_off"].copy()).to(dev)
    print("%d symbols, %.2f characters a piece; rounds %d x %d calls, alternating; us per call"
          % (len(d), float((table["pieces"] != CS.SEP).sum()) / (len(d) - 4), a.rounds, a.calls))
    cases = []
    refs, best, nbest = make_rows(d, 16, 5, 30, 59)
    ref, ref_len = matrix(refs, 60, d.pad(), dev)
    cases.append(("width 60, 16 best hypotheses",) + matrix(best, 60, d.pad(), dev) + (None, ref, ref_len, None))
    rows = torch.tensor([b for b in range(16) for _ in range(5)], dtype=torch.int32, device=dev)
    cases.append(("width 60, 16 x 5 n-best",) + matrix(nbest, 60, d.pad(), dev) + (None, ref, ref_len, rows))
    for n in (32, 64):
        _, _, lists = make_rows(d, 16, n, 30, 59, seed=n)
        m, ln = matrix(lists, 60, d.pad(), dev)
        hr = torch.tensor([b * n + i for b in range(16) for i in range(n) for _ in range(n)], dtype=torch.int32, device=dev)
        rr = torch.tensor([b * n + j for b in range(16) for _ in range(n) for j in range(n)], dtype=torch.int32, device=dev)
        cases.append(("width 60, MBR 16 x %d (%d pairs, one matrix as both sides)" % (n, 16 * n * n), m, ln, hr, m, ln, rr))
    refs, best, _ = make_rows(d, 4, 0, 930, 980)
    cases.append(("width 1024, 4 rows near the character limit",) + matrix(best, 1024, d.pad(), dev) + (None,) + matrix(refs, 1024, d.pad(), dev) + (None,))
    for what, hyp, hyp_len, hyp_row, ref, ref_len, ref_row in cases:
        for wo in (0, 2):
            call = lambda: K.chrf_stats(hyp, hyp_len, ref, ref_len, pieces, off, unk=d.unk(), char_order=6, word_order=wo,
                                        hyp_row=hyp_row, ref_row=ref_row)
            device_sums = lambda: call()[0].sum(0).tolist()
            host = lambda: host_sums(d, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, wo)
            stats, status = call()
            one, two = device_sums(), host()
            P = status.shape[0]
            print("%s, word_order %d: %d pairs, %d refused, %d .. %d hypothesis characters; character matches %s; the routes' sums are equal: %s"
                  % (what, wo, P, int((status != 0).sum()), int(stats[:, 0].min()), int(stats[:, 0].max()), one[2:18:3], one == two))
            big = P > 1000
            routes = [("device  K.chrf_stats", device_time, call, a.calls),
                      ("to the sums on the host  K.chrf_stats, 24 sums copied", wall_time, device_sums, a.calls),
                      ("to the sums on the host  tokens.cpu() + Dictionary.string + Counter loop", wall_time, host, 1 if big else a.calls)]
            for _, _, fn, _ in routes[:2]:
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            times = [[] for _ in routes]
            for _ in range(min(a.rounds, 3) if big else a.rounds):
                for i, (_, timer, fn, calls) in enumerate(routes):
                    times[i].append(timer(fn, calls))
            med = [statistics.median(ts) for ts in times]
            for (tag, _, _, _), ts, m in zip(routes, times, med):
                print("  %-76s %s -> median %.1f us" % (tag, " ".join("%.1f" % v for v in ts), m))
            print("  host route / device call, both to the sums on the host: %.2f x" % (med[2] / med[1]))
            sys.stdout.flush()


if __name__ == "__main__":
    main()
