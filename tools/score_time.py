#!/usr/bin/env python3
"""Time K.score_targets (s2t_score_targets, csrc/score.hip) against the only route the package had for the same numbers, on the same
buffers:

    n = 1:  K.log_softmax(rows) -> gather of the target column
    n > 1:  K.softmax_probs(rows) per member -> gather; the gathered probabilities are added, divided by n and the log is taken
            (the order of fairseq/sequence_scorer.py:65-92)

    python tools/score_time.py [--rounds 7] [--calls 20] > profiles/score_targets.txt

Shapes: rows in {2,560, 20,480} (B = 64 / 512, L = 40), V = 8,000, bf16 and f32, n in {1, 2, 4}.  Per shape both routes are warmed up,
then timed in alternating rounds with device events around `calls` back-to-back calls; every round's per-call figure is printed, then
the medians.  Also printed: the bytes each route has to move (computed from the shapes), torch.cuda.max_memory_allocated around one
call of each route (above what the inputs hold), and the largest difference between the two routes' results.  Needs an MI355X; there
is no pass / fail threshold.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402

DEV = "cuda"


def old_route(bufs, target):
    """what a caller had to do before: one f32 [rows, V] tensor per member.  bufs: time-major [L, B, V] (row stride padded)"""
    Ln, B, V = bufs[0].shape
    col = target.t().reshape(-1, 1)                             # time-major rows t*B + b
    if len(bufs) == 1:
        return K.log_softmax(bufs[0].view(Ln * B, V)).gather(1, col).view(Ln, B).t()
    acc = None
    for x in bufs:
        p = K.softmax_probs(x.view(Ln * B, V)).gather(1, col)
        acc = p if acc is None else acc.add_(p)
    return acc.div_(len(bufs)).log_().view(Ln, B).t()


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls                     # us per call


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--V", type=int, default=8000)
    ap.add_argument("--L", type=int, default=40)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "score_time.py measures on the GPU"
    print("device:", torch.cuda.get_device_name(0))
    print("rounds %d x %d calls, alternating; us per call" % (a.rounds, a.calls))
    V, Ln = a.V, a.L
    for dtype in (torch.bfloat16, torch.float32):
        esz = 2 if dtype == torch.bfloat16 else 4
        for B in (64, 512):
            rows = B * Ln
            for n in (1, 2, 4):
                g = torch.Generator(device=DEV).manual_seed(rows + n)
                bufs = [K.alloc_rows((Ln, B), V, dtype, DEV) for _ in range(n)]
                for buf in bufs:
                    buf.copy_((torch.randn(Ln, B, V, generator=g, device=DEV) * 3).to(dtype))
                views = [buf.transpose(0, 1) for buf in bufs]
                target = torch.randint(0, V, (B, Ln), generator=g, device=DEV)
                new = lambda: K.score_targets(views, target)
                old = lambda: old_route(bufs, target)
                diff = float((new().double() - old().double()).abs().max())
                for _ in range(3):
                    new(); old()
                torch.cuda.synchronize()
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(timed(new, a.calls))
                    to.append(timed(old, a.calls))
                read = n * rows * V * esz
                new_bytes = read + rows * 12                                       # + targets (8) and scores (4)
                old_bytes = n * rows * V * (3 * esz + 4) + n * rows * (4 + 8) * 2    # three reads, one f32 write, then the gathers
                tag = "%s rows=%d V=%d n=%d" % (str(dtype).replace("torch.", ""), rows, V, n)
                print("%s\n  score_targets   %s -> median %.1f us  (%.1f MB to move: %.0f GB/s)" % (
                    tag, " ".join("%.1f" % v for v in tn), statistics.median(tn), new_bytes / 1e6, new_bytes / statistics.median(tn) / 1e3))
                print("  softmax + gather %s -> median %.1f us  (%.1f MB to move)" % (
                    " ".join("%.1f" % v for v in to), statistics.median(to), old_bytes / 1e6))
                print("  peak memory above the inputs: score_targets %.2f MB, softmax + gather %.2f MB; max |difference| of the results %.3g"
                      % (peak_above_inputs(new) / 1e6, peak_above_inputs(old) / 1e6, diff))
                sys.stdout.flush()
                del bufs, views


if __name__ == "__main__":
    main()
