#!/usr/bin/env python3
"""Time the CTC segmenter (csrc/ctc_segment.hip: K.ctc_segment), phase by phase, beside a torch-on-device formulation of the same rule
-- `log_softmax`, a `gather` of the extended transcript's columns with the two free columns zeroed, a loop of T steps of
`torch.maximum` / `torch.where` over [B, S], the back-pointers copied to the host and walked there with NumPy -- on the same logits, in
the same process, and beside the workgroup form of the aligner (K.ctc_align at 1,024 tokens) on the same library:

    python tools/ctc_segment_time.py [--rounds 5] [--calls 3] > profiles/ctc_segment.txt

Shapes, V = 5,001: (a) one recording of 22,500 frames with 5,000 tokens in 150 utterances, (b) the same with 15,000 tokens, (c) eight
recordings of 7,500 frames and 2,000 tokens in 60 utterances; bf16 and f32, row stride padded as the engine pads it.  The logits look
like a trained head's: randn x 3 with 22 added along a valid path of the transcript that leaves 5 % of the frames free at either end.
The phases are bracketed by device events inside the library (s2t_prof_*); whole calls by device events around `calls` back-to-back
calls.  Rounds alternate between the routes; every round is printed, then the median.  The torch route is timed once per shape (it
takes seconds).  Needs an MI355X; there is no pass / fail threshold: the two routes' paths are compared and the ratios reported."""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402

DEV = "cuda"
SHAPES = [("a", 22500, 1, 5000, 150), ("b", 22500, 1, 15000, 150), ("c", 7500, 8, 2000, 60)]     # name, T, B, tokens, utterances
PHASES = ("ctc_segment_rows", "ctc_segment_recording", "ctc_segment_utterances")
ALIGN_SHAPE = (1500, 4, 1024)


def make_case(T, B, V, L, U, dtype, blank):
    rng = np.random.default_rng(11)
    x = (rng.standard_normal((T, B, V)) * 3).astype(np.float32)
    targets = rng.integers(0, V - 1, size=(B, L))
    same = targets[:, 1:] == targets[:, :-1]
    targets[:, 1:][same] = (targets[:, 1:][same] + 1) % (V - 1)        # no token repeats its predecessor: no blank is forced
    for b in range(B):
        counts = np.zeros(2 * L + 1, np.int64)
        counts[1::2] = 1                                              # every token a frame; 15,000 tokens on 22,500 frames leave few blanks
        counts[0] = counts[-1] = T // 20
        counts[1:-1] += rng.multinomial(T - counts.sum(), np.full(2 * L - 1, 1.0 / (2 * L - 1)))
        z = np.full(2 * L + 1, blank)
        z[1::2] = targets[b]
        path = np.repeat(np.arange(2 * L + 1), counts)
        text = (path > 0) & (path < 2 * L)
        x[np.nonzero(text)[0], b, z[path[text]]] += 22
    buf = K.alloc_rows((T, B), V, dtype, DEV)
    buf.copy_(torch.from_numpy(x).to(DEV).to(dtype))
    ends = torch.tensor(np.linspace(L / U, L, U).round().astype(np.int64)).repeat(B, 1)
    i64 = lambda v: torch.full((B,), v, dtype=torch.int64, device=DEV)
    return buf, torch.full((B,), T, dtype=torch.int32, device=DEV), torch.from_numpy(targets).to(DEV), i64(L), ends.to(DEV), i64(U)


def torch_forward(logits, in_len, targets, tgt_len, blank):
    """the rule's recursion with both ends free in torch ops: (back-pointers [T, B, S] int8, final values [B, S])"""
    T, B, V = logits.shape
    S = 2 * targets.shape[1] + 1
    ninf = float("-inf")
    lp = torch.log_softmax(logits.float(), -1)
    z = torch.full((B, S), blank, dtype=torch.int64, device=logits.device)
    z[:, 1::2] = targets
    em = lp.gather(2, z.unsqueeze(0).expand(T, B, S))
    del lp
    em[:, :, 0] = 0
    em[:, :, S - 1] = 0
    skip = torch.zeros((B, S), dtype=torch.bool, device=logits.device)
    skip[:, 3::2] = targets[:, 1:] != targets[:, :-1]
    pad1, pad2 = em.new_full((B, 1), ninf), em.new_full((B, 2), ninf)
    v = em.new_full((B, S), ninf)
    v[:, :2] = em[0, :, :2]
    bps = torch.zeros((T, B, S), dtype=torch.int8, device=logits.device)
    for t in range(1, T):
        a1 = torch.cat([pad1, v[:, :-1]], 1)
        a2 = torch.where(skip, torch.cat([pad2, v[:, :-2]], 1), pad1)
        m1 = torch.maximum(v, a1)
        bps[t] = (a1 > v).to(torch.int8) + (a2 > m1).to(torch.int8) * 2 - ((a2 > m1) & (a1 > v)).to(torch.int8)
        v = em[t] + torch.maximum(m1, a2)
    return bps, v


def torch_route(logits, in_len, targets, tgt_len, blank):
    """states [B, T] on the host (NumPy)"""
    bp, v = torch_forward(logits, in_len, targets, tgt_len, blank)
    bp, v = bp.cpu().numpy(), v.cpu().numpy()
    T, B, S = bp.shape
    rows = np.arange(B)
    s = np.where(v[:, S - 2] > v[:, S - 1], S - 2, S - 1)
    states = np.zeros((B, T), np.int32)
    for t in range(T - 1, -1, -1):
        states[:, t] = s
        if t:
            s = s - bp[t, rows, s]
    return states


def device_time(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def phases(fn, calls, names):
    """us per call of each named family, from the library's own device events"""
    K.prof_reset()
    K.prof_enable(True)
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    out = [K.prof_read(n)["ms"] * 1e3 / calls for n in names]
    K.prof_enable(False)
    return out


def copy_rate(nbytes=1 << 30):
    a = torch.empty((nbytes,), dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    for _ in range(2):
        b.copy_(a)
    return 2 * nbytes / (statistics.median(device_time(lambda: b.copy_(a), 5) for _ in range(5)) * 1e-6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--V", type=int, default=5001)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_segment_time.py measures on the GPU"
    V, blank = a.V, a.V - 1
    rate = copy_rate()
    print("device:", torch.cuda.get_device_name(0))
    print("V = %d; rounds %d x %d calls; us per call; this run's copy rate (1 GiB, read + write): %.2f TB/s" % (V, a.rounds, a.calls, rate / 1e12))
    per_frame = {}
    for name, T, B, L, U in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            args = make_case(T, B, V, L, U, dtype, blank) + (blank,)
            fn = lambda: K.ctc_segment(*args)
            out = fn()
            dt = str(dtype).replace("torch.", "")
            head = "(%s) T = %d, B = %d, %d tokens in %d utterances, %s" % (name, T, B, L, U, dt)
            print("%s: status %s" % (head, sorted(set(out[-1].tolist()))))
            fn()
            whole = [device_time(fn, a.calls) for _ in range(a.rounds)]
            ph = [phases(fn, a.calls, PHASES) for _ in range(a.rounds)]
            med = [statistics.median(p[i] for p in ph) for i in range(3)]
            print("  %-46s %s -> median %.1f us" % ("K.ctc_segment, whole call", " ".join("%.1f" % v for v in whole), statistics.median(whole)))
            for i, tag in enumerate(("row phase", "recording phase", "utterance phase")):
                print("  %-46s %s -> median %.1f us" % (tag, " ".join("%.1f" % p[i] for p in ph), med[i]))
            floor = T * B * V * args[0].element_size() / rate * 1e6
            per_frame[(name, dt)] = med[1] / T
            print("  recording phase: %.3f us per frame; the logits' %.1f MB at this run's copy rate: %.1f us; row phase %.2f x, whole call "
                  "%.1f x that" % (med[1] / T, T * B * V * args[0].element_size() / 1e6, floor, med[0] / floor, statistics.median(whole) / floor))
            if not a.no_torch:
                same = np.array_equal(out[0].cpu().numpy(), torch_route(*args[:4], blank))
                t_torch = device_time(lambda: torch_forward(*args[:4], blank), 1)
                print("  torch route, recursion only (no back-trace), one call: %.0f us = %.0f x K.ctc_segment; the two routes' paths are equal: %s"
                      % (t_torch, t_torch / statistics.median(whole), same))
            sys.stdout.flush()
            del args, out
            torch.cuda.empty_cache()
    T, B, Lmax = ALIGN_SHAPE
    for dtype in (torch.bfloat16, torch.float32):
        x, n, tg, ln, _, _ = make_case(T, B, V, Lmax, 1, dtype, blank)
        ln = torch.full_like(ln, T // 2 - 2)
        fn = lambda: K.ctc_align(x, n, tg, ln, blank)
        fn()
        ph = [phases(fn, a.calls, ("ctc_align_sentences",))[0] for _ in range(a.rounds)]
        dt = str(dtype).replace("torch.", "")
        m = statistics.median(ph)
        print("K.ctc_align, workgroup form, T4 = %d, B = %d, width %d, %s: sentence phase %s -> median %.1f us = %.3f us per frame; the "
              "segmenter's recording phase at shape (c) takes %.2f x that per frame" % (T, B, Lmax, dt, " ".join("%.1f" % v for v in ph), m, m / T,
                                                                                        per_frame[("c", dt)] / (m / T)))


if __name__ == "__main__":
    main()
