#!/usr/bin/env python3
"""Time the edit-distance aligner (csrc/edit_align.hip: K.edit_align in collapse mode) beside the host pass the criterion runs
(`K.host_ctc_uer`, the copy of `pred` to the host included) on the same inputs, in the same process:

    python tools/edit_align_time.py [--rounds 7] [--calls 10] > profiles/edit_align.txt

Shapes: B = 64 with 375 frames per sentence and targets of width 60 (the criterion's shape: one wave per sentence, one column per
lane), and B = 16 with 1,500 frames and targets of width 1,024 (one workgroup per sentence).  Frame labels come in runs of 1 to 8
frames, four in ten of them blank; the targets are a noisy copy of the collapsed labels, so the alignments look like a trained
model's, not like two unrelated strings.  Costs (4, 3, 3), the reference's.
Device figures are device events around `calls` back-to-back calls, per call, with and without `ops`; "to the sums on the host"
figures are wall-clock per call from `pred` on the device to the two sums on the host (synchronising).  Rounds alternate between
the routes; every round is printed, then the median.  Needs an MI355X; there is no pass / fail threshold: the two routes' sums are
compared and the times reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402

DEV = "cuda"
SHAPES = [(64, 375, 60), (16, 1500, 1024)]          # B, frames, padded target width
COSTS = (4, 3, 3)


def make_case(B, T, Bmax, V, blank):
    rng = np.random.default_rng(11)
    pred = np.empty((B, T), np.int32)
    tgt = rng.integers(0, V - 1, (B, Bmax))
    tgt_len = np.zeros((B,), np.int64)
    for b in range(B):
        t, toks, last = 0, [], None
        while t < T:
            run = int(rng.integers(1, 9))
            x = blank if rng.random() < 0.4 else int(rng.integers(0, V - 1))
            pred[b, t:t + run] = x
            if x != blank and x != last:
                toks.append(x)
            last = x
            t += run
        keep = [x if rng.random() > 0.1 else int(rng.integers(0, V - 1)) for x in toks if rng.random() > 0.05][:Bmax]
        tgt[b, :len(keep)] = keep
        tgt_len[b] = len(keep)
    in_len = np.full((B,), T, np.int32)
    return (torch.from_numpy(pred).to(DEV), torch.from_numpy(in_len).to(DEV), torch.from_numpy(tgt).to(DEV), torch.from_numpy(tgt_len).to(DEV))


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
    ap.add_argument("--V", type=int, default=5001)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "edit_align_time.py measures on the GPU"
    V, blank = a.V, a.V - 1
    print("device:", torch.cuda.get_device_name(0))
    print("V = %d, costs %s; rounds %d x %d calls, alternating; us per call" % (V, COSTS, a.rounds, a.calls))
    for B, T, Bmax in SHAPES:
        pred, in_len, tgt, tgt_len = make_case(B, T, Bmax, V, blank)
        in_len64, tgt_host, tgt_len_host = in_len.long().cpu(), tgt.cpu(), tgt_len.cpu()

        def device(want_ops):
            return K.edit_align(pred, in_len, tgt, tgt_len, COSTS, collapse_blank=blank, want_ops=want_ops)

        def device_sums():
            counts = device(False)[0]
            return torch.stack([counts[:, 1:].sum(), tgt_len.sum()]).tolist()

        def host_sums():
            return K.host_ctc_uer(pred.cpu(), in_len64, tgt_host, tgt_len_host, blank)

        e_dev, n_dev = device_sums()
        e_host, n_host = host_sums()
        a_n = device(False)[3]
        print("B = %d, %d frames, target width %d (hypotheses %d .. %d tokens, targets %d .. %d): errors %d of %d tokens; "
              "the two routes' sums are equal: %s" % (B, T, Bmax, int(a_n.min()), int(a_n.max()), int(tgt_len.min()), int(tgt_len.max()),
                                                      e_dev, n_dev, (float(e_dev), float(n_dev)) == (e_host, n_host)))
        routes = [("device  K.edit_align, collapse + counts", device_time, lambda: device(False)),
                  ("device  K.edit_align, collapse + counts + ops", device_time, lambda: device(True)),
                  ("to the sums on the host  K.edit_align, two sums copied", wall_time, device_sums),
                  ("to the sums on the host  pred.cpu() + K.host_ctc_uer", wall_time, host_sums),
                  ("host  K.host_ctc_uer alone (pred already on the host)", wall_time,
                   (lambda p: lambda: K.host_ctc_uer(p, in_len64, tgt_host, tgt_len_host, blank))(pred.cpu()))]
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
        print("  host pass / device call, both to the sums on the host: %.2f x" % (med[3] / med[2]))
        sys.stdout.flush()


if __name__ == "__main__":
    main()
