#!/usr/bin/env python3
"""Time the pairwise BLEU kernel (csrc/bleu_pairs.hip: K.bleu_pairs) beside the two routes to the same N x M statistics that exist
without it, on the same inputs, in the same process:

    python tools/mbr_time.py [--rounds 7] [--calls 10] [--twin LIB ...] > profiles/mbr.txt

Shapes: int64 tokens (what the search returns; staged as 64-bit), every sentence's hypotheses against themselves: 16 sentences x 8
(a beam's list), 16 x 32 and 16 x 64 at padded width 60 (one wave per candidate), 4 x 128 at width 200 (a workgroup per candidate).
The hypotheses of a sentence are noisy copies of one sentence over 5,000 symbols (one token in ten dropped, one in ten replaced) that
end in eos and are padded, so the n-gram matches look like an n-best list's, not like unrelated strings.
Routes:
  pairs     K.bleu_pairs on the list as it lies: one launch.
  repeated  the route without the kernel: every candidate row repeated once per pseudo-reference (an index_select: the copy is part
            of the route) and K.bleu_stats on the repeated rows behind a ref_row map.
  host      the tokens copied to the host and a collections.Counter loop over every pair.
Device figures are device events around `calls` back-to-back calls as Python makes them, per call; the host route is wall-clock and
runs `--host-rounds` times.  Rounds alternate between the routes; every round is printed, then the median.
--twin LIB: a build of the kernel with another slice of the list per workgroup (make -C fbk_fairseq_st_amd/csrc mbr_twin SLICE=64
makes libs2t_hip_mbr_s64.so: one workgroup per candidate for lists up to 64); its s2t_bleu_pairs is timed in the same rounds on the
same tensors.  A twin is called through ctypes on preallocated-size outputs, without the checks of K.bleu_pairs: pass the library
itself (fbk_fairseq_st_amd/libs2t_hip.so) as a twin too, and compare the twins with that line.
Needs an MI355X; there is no pass / fail threshold: the routes' statistics are compared and the times reported."""
import argparse
import ctypes
import os
import statistics
import sys
import time
from collections import Counter

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402
from fbk_fairseq_st_amd import lib as L  # noqa: E402

PAD, EOS, UNK = 1, 2, 3
SHAPES = [(16, 8, 60), (16, 32, 60), (16, 64, 60), (4, 128, 200)]          # sentences, hypotheses per sentence, padded width


def make_case(B, N, width, dev, V=5000):
    """-> (hyp [B * N, width], lengths, sentence of each row int32, offsets int32), int64 tokens on `dev`"""
    rng = np.random.default_rng(17)
    rows = []
    for _ in range(B):
        base = (4 + rng.integers(0, V, int(rng.integers(width // 2, width)))).tolist()
        for _ in range(N):
            h = [t if rng.random() > 0.1 else int(4 + rng.integers(0, V)) for t in base if rng.random() > 0.1]
            rows.append(h[:width - 1] + [EOS])
    m = np.full((len(rows), width), PAD, np.int64)
    for s, r in enumerate(rows):
        m[s, :len(r)] = r
    sent = torch.tensor([b for b in range(B) for _ in range(N)], dtype=torch.int32, device=dev)
    off = torch.arange(0, B * N + 1, N, dtype=torch.int32, device=dev)
    return torch.from_numpy(m).to(dev), torch.tensor([len(r) for r in rows], device=dev), sent, off


def host_stats(hyp, hyp_len, B, N):
    """the rule on host tensors, a pair at a time: trim, then a Counter per order -> the ten sums over all pairs"""
    hyp, hyp_len = hyp.tolist(), hyp_len.tolist()

    def trim(t):
        a = 0
        while a < len(t) and t[a] == PAD:
            a += 1
        t = t[a:]
        e = len(t) - 1
        while e > 0 and t[e] in (EOS, PAD):
            e -= 1
        return t[:e + 1]

    rows = [trim(h[:n]) for h, n in zip(hyp, hyp_len)]
    sums = [0] * 10
    for b in range(B):
        for h in rows[b * N:(b + 1) * N]:
            for x in rows[b * N:(b + 1) * N]:
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


def twin_call(path):
    """s2t_bleu_pairs of another build of the library, on the tensors of K.bleu_pairs"""
    lib = ctypes.CDLL(path)
    lib.s2t_bleu_pairs.argtypes = L.SIGNATURES["s2t_bleu_pairs"]

    def call(hyp, hyp_len, sent, off, M):
        stats = torch.empty((hyp.shape[0], M, 10), dtype=torch.int32, device=hyp.device)
        status = torch.empty((hyp.shape[0], M), dtype=torch.int32, device=hyp.device)
        rc = lib.s2t_bleu_pairs(L.ptr(hyp), L.ptr(hyp_len), 8, L.ptr(hyp), L.ptr(hyp_len), 8, L.ptr(sent), L.ptr(off), hyp.shape[0], off.shape[0] - 1,
                                hyp.shape[1], hyp.shape[1], hyp.shape[0], M, PAD, EOS, UNK, L.ptr(stats), L.ptr(status), L.stream())
        assert rc == 0, rc
        return stats, status
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--twin", action="append", default=[])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mbr_time.py measures on the GPU"
    print("device:", torch.cuda.get_device_name(0))
    print("pad %d, eos %d, unk %d; int64 tokens; rounds %d x %d calls, alternating; us per call" % (PAD, EOS, UNK, a.rounds, a.calls))
    twins = [(os.path.basename(p), twin_call(p)) for p in a.twin]
    for B, N, width in SHAPES:
        hyp, hyp_len, sent, off = make_case(B, N, width, "cuda")
        pairs = lambda: K.bleu_pairs(hyp, hyp_len, sent, hyp, hyp_len, off, PAD, EOS, UNK, max_list=N)
        idx = torch.arange(B * N, device="cuda").repeat_interleave(N)                       # candidate of every pair
        row = (off[:-1].long()[sent.long()][:, None] + torch.arange(N, device="cuda")[None, :]).reshape(-1).int()   # its pseudo-reference

        def repeated():
            return K.bleu_stats(hyp.index_select(0, idx), hyp_len.index_select(0, idx), hyp, hyp_len, PAD, EOS, UNK, ref_row=row)
        host = lambda: host_stats(hyp.cpu(), hyp_len.cpu(), B, N)
        one, two = pairs()[0], repeated()[0]
        same = torch.equal(one.reshape(-1, 10), two) and all(torch.equal(t(hyp, hyp_len, sent, off, N)[0], one) for _, t in twins)
        sums = one.sum((0, 1), dtype=torch.int64).tolist()
        t0 = time.perf_counter()
        host_sums = host()
        host_us = [(time.perf_counter() - t0) * 1e6] + [wall_time(host, 1) for _ in range(a.host_rounds - 1)]
        print("%d sentences x %d hypotheses, width %d (%d .. %d tokens): %d pairs, match %s of count %s; the routes' statistics are equal: %s"
              % (B, N, width, int(hyp_len.min()), int(hyp_len.max()), B * N * N, sums[2::2], sums[3::2], same and sums == host_sums))
        print("  the repeated-rows route allocates %d bytes for the repeated candidates (%d rows x %d x 8) and %d for their lengths and the map"
              % (B * N * N * width * 8, B * N * N, width, B * N * N * 12))
        routes = [("pairs     K.bleu_pairs", pairs), ("repeated  index_select + K.bleu_stats with a ref_row map", repeated)]
        routes += [("pairs     %s" % name, (lambda t=t: t(hyp, hyp_len, sent, off, N))) for name, t in twins]
        for _, fn in routes:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in routes]
        for _ in range(a.rounds):
            for i, (_, fn) in enumerate(routes):
                times[i].append(device_time(fn, a.calls))
        med = [statistics.median(ts) for ts in times]
        for (tag, _), ts, m in zip(routes, times, med):
            print("  device  %-58s %s -> median %.1f us" % (tag, " ".join("%.1f" % v for v in ts), m))
        print("  host    %-58s %s -> median %.0f us" % ("tokens.cpu() + Counter loop over the pairs", " ".join("%.0f" % v for v in host_us), statistics.median(host_us)))
        print("  repeated / pairs: %.2f x; host / pairs: %.0f x" % (med[1] / med[0], statistics.median(host_us) / med[0]))
        for (tag, _), m in list(zip(routes, med))[2:]:
            print("  %s / pairs: %.2f x" % (tag.split()[-1], m / med[0]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
