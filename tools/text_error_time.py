#!/usr/bin/env python3
"""Time TextErrorRate (text_error_rate.py: kernels.text_units, then kernels.edit_align) beside a host route on the same inputs, in the
same process:

    python tools/text_error_time.py [--rounds 5] [--calls 10] [--chrf-ab OTHER.so] > profiles/text_error.txt

Dictionary and rows are those of tools/chrf_time.py (5,000 synthetic sentencepiece-style symbols, about 4 characters a piece, four in
ten starting a word; references end in eos, hypotheses are noisy copies), int64 tokens.  Shapes: 16 best hypotheses at padded width
60; a 16 x 5 n-best list (the list shares its references through the row map); 16 pairs at width 200; 4 pairs near 4,095 characters;
and the MBR shape, lists of 16 x 32 hypotheses judged against themselves (16,384 pairs through two row maps, one matrix as both
sides).  Units: words and characters with spaces; near the character limit characters without spaces, since there the spaces push
a side past S2T_TEXT_MAX_UNITS and the kernel refuses it.
Device figures are device events around `calls` back-to-back calls, per call, as Python makes the call: `score_pairs` whole (both
launches and the torch arithmetic behind them), and each launch alone on the same operands.  "To the sums on the host" figures are
wall-clock per call from the tokens on the device to the error count on the host (synchronising).  The host route copies the tokens
to the host and runs `Dictionary.string` per row and a two-row Python Levenshtein loop per pair (the distance only: fewer numbers than
the device route gives); it is not run where one call would take more than 2e7 cells of that loop, and once per round above 1e6.
Rounds alternate between the routes; every round is printed, then the median.  Needs an MI355X; there is no pass / fail threshold:
the routes' error counts are compared and the times reported.

--chrf-ab OTHER.so [MORE.so ...]: also time s2t_chrf_stats of this build's library against the others (any library that exports
s2t_chrf_stats, such as the parent commit's chrf_stats.hip compiled alone, or this tree's compiled alone the same way) on this
file's shapes, all through ctypes, alternating per round in this process: the check that moving the text functions into
csrc/text_rows.hpp did not slow chrF."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chrf_ref as C  # noqa: E402
import chrf_time as CT  # noqa: E402
from fbk_fairseq_st_amd import chrf_scorer as CS  # noqa: E402
from fbk_fairseq_st_amd import kernels as K  # noqa: E402
from fbk_fairseq_st_amd import lib as L  # noqa: E402
from fbk_fairseq_st_amd import text_error_rate as TE  # noqa: E402

BPE = "sentencepiece"


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[len(b)]


def host_units(d, hyp, hyp_len, ref, ref_len, unit):
    """copy, Dictionary.string, split -> the unit lists of every row"""
    hyp, hyp_len, ref, ref_len = hyp.cpu().tolist(), hyp_len.cpu().tolist(), ref.cpu().tolist(), ref_len.cpu().tolist()
    cut = (lambda t: t.split()) if unit == "word" else list if unit == "char" else (lambda t: list(t.replace(" ", "")))
    return ([cut(C.text_of(d, h[:n], BPE, False)) for h, n in zip(hyp, hyp_len)],
            [cut(C.text_of(d, r[:n], BPE, True)) for r, n in zip(ref, ref_len)])


def host_errors(d, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, unit):
    hu, ru = host_units(d, hyp, hyp_len, ref, ref_len, unit)
    P = len(hyp_row) if hyp_row is not None else len(ref_row) if ref_row is not None else len(hu)
    hr = range(P) if hyp_row is None else hyp_row.cpu().tolist()
    rr = range(P) if ref_row is None else ref_row.cpu().tolist()
    return sum(levenshtein(hu[i], ru[j]) for i, j in zip(hr, rr))


def cases_of(d, dev):
    cases = []
    refs, best, nbest = CT.make_rows(d, 16, 5, 30, 59)
    ref, ref_len = CT.matrix(refs, 60, d.pad(), dev)
    both = ("word", "char")
    cases.append(("width 60, 16 best hypotheses", both) + CT.matrix(best, 60, d.pad(), dev) + (None, ref, ref_len, None))
    rows = torch.tensor([b for b in range(16) for _ in range(5)], dtype=torch.int32, device=dev)
    cases.append(("width 60, 16 x 5 n-best", both) + CT.matrix(nbest, 60, d.pad(), dev) + (None, ref, ref_len, rows))
    refs, best, _ = CT.make_rows(d, 16, 0, 150, 199, seed=3)
    cases.append(("width 200, 16 pairs", both) + CT.matrix(best, 200, d.pad(), dev) + (None,) + CT.matrix(refs, 200, d.pad(), dev) + (None,))
    refs, best, _ = CT.make_rows(d, 4, 0, 930, 980)
    cases.append(("width 1024, 4 pairs near 4,095 characters", ("word", "char_nospace")) + CT.matrix(best, 1024, d.pad(), dev) + (None,) + CT.matrix(refs, 1024, d.pad(), dev) + (None,))
    n = 32
    _, _, lists = CT.make_rows(d, 16, n, 30, 59, seed=n)
    m, ln = CT.matrix(lists, 60, d.pad(), dev)
    hr = torch.tensor([b * n + i for b in range(16) for i in range(n) for _ in range(n)], dtype=torch.int32, device=dev)
    rr = torch.tensor([b * n + j for b in range(16) for _ in range(n) for j in range(n)], dtype=torch.int32, device=dev)
    cases.append(("width 60, MBR 16 x %d (%d pairs, one matrix as both sides)" % (n, 16 * n * n), both, m, ln, hr, m, ln, rr))
    return cases


def report(routes, rounds):
    times = [[] for _ in routes]
    for _ in range(rounds):
        for i, (_, timer, fn, calls) in enumerate(routes):
            times[i].append(timer(fn, calls))
    med = [statistics.median(ts) for ts in times]
    for (tag, _, _, _), ts, m in zip(routes, times, med):
        print("  %-76s %s -> median %.1f us" % (tag, " ".join("%.1f" % v for v in ts), m))
    sys.stdout.flush()
    return med


def time_units(a, d, table, dev):
    for what, units_, hyp, hyp_len, hyp_row, ref, ref_len, ref_row in cases_of(d, dev):
        for unit in units_:
            te = TE.TextErrorRate(table, unit)
            score = lambda: te.score_pairs(hyp, hyp_len, hyp_row, ref, ref_len, ref_row)
            out = score()
            pieces, off = te.table_on(dev)
            Uh, Ur = te.unit_width(hyp.shape[1], "hyp"), te.unit_width(ref.shape[1], "ref")
            units = lambda: K.text_units(hyp, hyp_len, ref, ref_len, pieces, off, te.unk, te.mode, Uh, Ur, hyp_row=hyp_row, ref_row=ref_row)
            hu, hn, ru, rn, _ = units()
            align = lambda: K.edit_align(hu, hn, ru, rn, (1, 1, 1))
            device_errors = lambda: int(score()["errors"].sum())
            P = out["status"].shape[0]
            cells = int((out["hyp_units_n"].long() * out["ref_units_n"].long()).sum())
            run_host = cells <= 2e7
            host = lambda: host_errors(d, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, unit)
            same = (device_errors() == host()) if run_host else "not compared"
            print("%s, unit %s: %d pairs, %d refused, unit rows %d and %d wide, %d .. %d reference units, %d errors, %d alignment cells; "
                  "the routes' error counts are equal: %s" % (what, unit, P, int((out["status"] != 0).sum()), Uh, Ur, int(out["ref_units_n"].min()),
                                                              int(out["ref_units_n"].max()), int(out["errors"].sum()), cells, same))
            routes = [("device  TextErrorRate.score_pairs (both launches and the arithmetic)", CT.device_time, score, a.calls),
                      ("device  K.text_units alone", CT.device_time, units, a.calls),
                      ("device  K.edit_align alone, on the unit rows", CT.device_time, align, a.calls),
                      ("to the sums on the host  TextErrorRate.score_pairs, the error count copied", CT.wall_time, device_errors, a.calls)]
            if run_host:
                routes.append(("to the sums on the host  tokens.cpu() + Dictionary.string + Levenshtein loop", CT.wall_time, host,
                               1 if cells > 1e6 else a.calls))
            for _, _, fn, _ in routes[:4]:
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            med = report(routes, min(a.rounds, 3) if cells > 1e6 else a.rounds)
            if run_host:
                print("  host route / device route, both to the sums on the host: %.2f x -- the device route %s at this shape"
                      % (med[4] / med[3], "wins" if med[4] > med[3] else "loses"))
            else:
                print("  host route: not measured at this shape (one call is %d cells of the Python loop)" % cells)
            te.reset()


def time_chrf_ab(a, d, table, dev):
    sig = L.SIGNATURES["s2t_chrf_stats"]
    libs = []
    for tag, path in [("this build", L.LIB_PATH)] + [(os.path.basename(p), p) for p in a.chrf_ab]:
        lib = ctypes.CDLL(path)
        lib.s2t_chrf_stats.argtypes, lib.s2t_chrf_stats.restype = sig, ctypes.c_int
        libs.append((tag, lib.s2t_chrf_stats))
    print("chrF A/B: s2t_chrf_stats of this build's library against %s, through ctypes, device events, alternating per round; us per call"
          % ", ".join(tag for tag, _ in libs[1:]))
    pieces, off = torch.from_numpy(table["pieces"].view(np.int32).copy()).to(dev), torch.from_numpy(table["piece_off"].copy()).to(dev)
    cases = cases_of(d, dev)
    for what, _, hyp, hyp_len, hyp_row, ref, ref_len, ref_row in cases:
        P = hyp_row.shape[0] if hyp_row is not None else ref_row.shape[0] if ref_row is not None else hyp.shape[0]
        for wo in (0, 2):
            outs = []

            def caller(fn):
                stats = torch.empty((P, 24), dtype=torch.int32, device=dev)
                status = torch.empty((P,), dtype=torch.int32, device=dev)
                outs.append((stats, status))
                args = (L.ptr(hyp), L.ptr(hyp_len), 8, L.ptr(ref), L.ptr(ref_len), 8, L.ptr(hyp_row) if hyp_row is not None else None,
                        L.ptr(ref_row) if ref_row is not None else None, P, hyp.shape[1], ref.shape[1], hyp.shape[0], ref.shape[0],
                        L.ptr(pieces), L.ptr(off), pieces.shape[0], table["V"], table["unk"], 6, wo, L.ptr(stats), L.ptr(status), L.stream())
                return lambda: L.check(fn(*args), "s2t_chrf_stats")
            routes = [("device  s2t_chrf_stats, %s" % tag, CT.device_time, caller(fn), a.calls) for tag, fn in libs]
            for _, _, fn, _ in routes:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            equal = all(torch.equal(x, y) for o in outs[1:] for x, y in zip(outs[0], o))
            print("%s, word_order %d: %d pairs; the libraries' statistics are equal: %s" % (what, wo, P, equal))
            med = report(routes, a.rounds)
            print("  " + "; ".join("this build / %s: %.3f" % (tag, med[0] / m) for (tag, _), m in zip(libs[1:], med[1:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--chrf-ab", nargs="+", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "text_error_time.py measures on the GPU"
    dev = "cuda"
    print("device:", torch.cuda.get_device_name(0))
    d = CT.make_dictionary()
    table = CS.piece_table(d, BPE)
    print("%d symbols, %.2f characters a piece; rounds %d x %d calls, alternating; us per call"
          % (len(d), float((table["pieces"] != CS.SEP).sum()) / (len(d) - 4), a.rounds, a.calls))
    time_units(a, d, table, dev)
    if a.chrf_ab:
        time_chrf_ab(a, d, table, dev)


if __name__ == "__main__":
    main()
