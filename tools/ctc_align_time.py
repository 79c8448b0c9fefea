#!/usr/bin/env python3
"""Time the forced aligner (csrc/ctc_align.hip: K.ctc_align) beside a torch-on-device formulation of the same rule -- `log_softmax`, a
`gather` of the extended transcript's columns, a loop of T steps of `torch.maximum` / `torch.where` over [B, S], the back-pointers
copied to the host and walked there with NumPy -- on the same logits, in the same process:

    python tools/ctc_align_time.py [--rounds 7] [--calls 10] > profiles/ctc_align.txt

Shapes: T4 = 375 frames, V = 5,001, B = 16 with a padded transcript width of 60 and of 511 (one wave per sentence, 2 and 16 states
per lane), and T4 = 1,500, B = 4 with a width of 1,024 (one workgroup per sentence); bf16 and f32, row stride padded as the engine
pads it.  Sentences have min(width, frames / 2 - 2) tokens so that every one has a path (511 tokens do not fit 375 frames: the width
still selects the kernel and sets the torch route's S).  The logits look like a trained head's: randn x 3 with 22 added along a valid
path of the transcript.
Device figures are device events around `calls` back-to-back calls, per call; "to states on the host" figures are wall-clock per call
from the logits on the device to the path on the host (synchronising).  Rounds alternate between the routes; every round is printed,
then the median.  `--device-only` times K.ctc_align alone (for a kernel trace).  Needs an MI355X; there is no pass / fail threshold:
the two routes' paths are compared and the ratios reported."""
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
COPY_RATE = 6.3e12          # bytes / s, the achievable copy rate the row phase is held against
SHAPES = [(375, 16, 60), (375, 16, 511), (1500, 4, 1024)]          # T, B, padded transcript width


def make_case(T, B, V, Lmax, dtype, blank):
    rng = np.random.default_rng(11)
    lens = [T - (b * (T // 5)) // max(B - 1, 1) for b in range(B)]
    x = (rng.standard_normal((T, B, V)) * 3).astype(np.float32)
    targets = rng.integers(0, V - 1, size=(B, Lmax))
    tgt_len = []
    for b, n in enumerate(lens):
        L = min(Lmax, n // 2 - 2)
        tgt_len.append(L)
        # a valid path: token, blank, token, ... with the spare frames spread over all 2L + 1 states
        counts = np.ones(2 * L + 1, np.int64)
        counts[0] = counts[-1] = 0
        counts += rng.multinomial(n - counts.sum(), np.full(2 * L + 1, 1.0 / (2 * L + 1)))
        z = np.full(2 * L + 1, blank)
        z[1::2] = targets[b, :L]
        x[np.arange(n), b, np.repeat(z, counts)] += 22
    buf = K.alloc_rows((T, B), V, dtype, DEV)
    buf.copy_(torch.from_numpy(x).to(DEV).to(dtype))
    return (buf, torch.tensor(lens, dtype=torch.int32, device=DEV), torch.from_numpy(targets).to(DEV),
            torch.tensor(tgt_len, dtype=torch.int64, device=DEV))


def torch_forward(logits, in_len, targets, tgt_len, blank):
    """the rule's recursion in torch ops: (back-pointers [T, B, S] int8, final values [B, S])"""
    T, B, V = logits.shape
    Lmax = targets.shape[1]
    S = 2 * Lmax + 1
    ninf = float("-inf")
    lp = torch.log_softmax(logits.float(), -1)
    z = torch.full((B, S), blank, dtype=torch.int64, device=logits.device)
    z[:, 1::2] = targets
    em = lp.gather(2, z.unsqueeze(0).expand(T, B, S))
    live = torch.arange(S, device=logits.device)[None, :] < (2 * tgt_len + 1)[:, None]
    em = em.masked_fill(~live.unsqueeze(0), ninf)
    skip = torch.zeros((B, S), dtype=torch.bool, device=logits.device)
    skip[:, 3::2] = targets[:, 1:] != targets[:, :-1]
    pad1, pad2 = em.new_full((B, 1), ninf), em.new_full((B, 2), ninf)
    v = em.new_full((B, S), ninf)
    v[:, :2] = em[0, :, :2]
    bps = [torch.zeros((B, S), dtype=torch.int8, device=logits.device)]
    for t in range(1, T):
        a1 = torch.cat([pad1, v[:, :-1]], 1)
        a2 = torch.where(skip, torch.cat([pad2, v[:, :-2]], 1), pad1)
        m1 = torch.maximum(v, a1)
        k = (a1 > v).to(torch.int8) + (a2 > m1).to(torch.int8) * 2 - ((a2 > m1) & (a1 > v)).to(torch.int8)
        new = em[t] + torch.maximum(m1, a2)
        v = torch.where((t < in_len)[:, None], new, v)
        bps.append(k)
    return torch.stack(bps), v


def torch_route(logits, in_len, targets, tgt_len, blank):
    """states [B, T] on the host (NumPy), -1 behind in_len"""
    bp, v = torch_forward(logits, in_len, targets, tgt_len, blank)
    bp, v, n, L = bp.cpu().numpy(), v.cpu().numpy(), in_len.cpu().numpy(), tgt_len.cpu().numpy()
    T, B, _ = bp.shape
    rows = np.arange(B)
    last = 2 * L
    s = np.where(v[rows, np.maximum(last - 1, 0)] > v[rows, last], np.maximum(last - 1, 0), last)
    states = np.full((B, T), -1, np.int32)
    for t in range(T - 1, -1, -1):
        on = t < n
        states[on, t] = s[on]
        s = np.where(on & (t > 0), s - bp[t, rows, s], s)
    return states


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
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_align_time.py measures on the GPU"
    V, blank = a.V, a.V - 1
    print("device:", torch.cuda.get_device_name(0))
    print("V = %d; rounds %d x %d calls, alternating; us per call" % (V, a.rounds, a.calls))
    for T, B, Lmax in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            logits, in_len, targets, tgt_len = make_case(T, B, V, Lmax, dtype, blank)
            args = (logits, in_len, targets, tgt_len, blank)
            routes = [("device  K.ctc_align (row phase + sentence phase)", device_time, lambda: K.ctc_align(*args))]
            if not a.device_only:
                routes += [("device  torch route, recursion only (no back-trace)", device_time, lambda: torch_forward(*args)),
                           ("to states on the host  K.ctc_align, states.cpu()", wall_time, lambda: K.ctc_align(*args)[0].cpu()),
                           ("to states on the host  torch route, NumPy back-trace", wall_time, lambda: torch_route(*args))]
            states, _, _, _, status = K.ctc_align(*args)
            name = str(dtype).replace("torch.", "")
            head = "T4 = %d, B = %d, width %d (tokens %d .. %d), %s" % (T, B, Lmax, int(tgt_len.min()), int(tgt_len.max()), name)
            if a.device_only:
                print("%s: status %s" % (head, sorted(set(status.tolist()))))
            else:
                same = np.array_equal(states.cpu().numpy(), torch_route(*args))
                print("%s: status %s; the two routes' paths are equal: %s" % (head, sorted(set(status.tolist())), same))
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
            floor = T * B * V * logits.element_size() / COPY_RATE * 1e6
            print("  the logits' %.1f MB at 6.3 TB/s: %.1f us; K.ctc_align takes %.1f x that" % (T * B * V * logits.element_size() / 1e6, floor, med[0] / floor))
            if not a.device_only:
                print("  torch route / K.ctc_align: device %.1f x, to states on the host %.1f x" % (med[1] / med[0], med[3] / med[2]))
            sys.stdout.flush()
            del logits


if __name__ == "__main__":
    main()
