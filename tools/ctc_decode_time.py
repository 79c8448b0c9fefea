#!/usr/bin/env python3
"""Time the CTC decoders (csrc/ctc_decode.hip: K.ctc_greedy, K.ctc_prefix_beam, ctc_decoder.CTCDecoder) beside the host route they
replace -- `K.ctc_argmax(logits)[0].cpu()` plus a Python `itertools.groupby` per sentence, what the `ctc_acc` logging does -- on the same
logits:

    python tools/ctc_decode_time.py [--rounds 7] [--calls 20] > profiles/ctc_decode.txt

Shape: T4 = 375 frames, V = 5,001, B = 16 sentences (lengths 375 down to 300), bf16 and f32, row stride padded as the engine pads it.
The logits look like a trained head's: segments of 1 to 3 frames with one symbol (the blank in 6 of 10) 22 above randn x 3.
Device figures are device events around `calls` back-to-back calls, per call; "to transcripts" figures are wall-clock per call from the
logits on the device to Python lists on the host (synchronising), which is what a user of either route waits for.  Rounds alternate
between the routes; every round is printed, then the median.  Needs an MI355X; there is no pass / fail threshold."""
import argparse
import itertools
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fbk_fairseq_st_amd import kernels as K  # noqa: E402
from fbk_fairseq_st_amd.ctc_decoder import CTCDecoder  # noqa: E402
from fbk_fairseq_st_amd.data import Dictionary  # noqa: E402

DEV = "cuda"


def make_logits(T, B, V, dtype):
    rng = np.random.default_rng(11)
    x = np.empty((T, B, V), dtype=np.float32)
    for b in range(B):
        rows = []
        while len(rows) < T:
            r = rng.standard_normal(V).astype(np.float32) * 3
            r[V - 1 if rng.random() < 0.6 else int(rng.integers(0, V - 1))] += 22
            rows += [r] * int(rng.integers(1, 4))
        x[:, b] = np.stack(rows[:T]) + 0.3 * rng.standard_normal((T, V)).astype(np.float32)
    buf = K.alloc_rows((T, B), V, dtype, DEV)
    buf.copy_(torch.from_numpy(x).to(DEV).to(dtype))
    return buf


def host_route(logits, lens, blank):
    pred = K.ctc_argmax(logits)[0].cpu()
    return [[k for k, _ in itertools.groupby(pred[b, :n].tolist()) if k != blank] for b, n in enumerate(lens)]


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
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--T", type=int, default=375)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--V", type=int, default=5001)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "ctc_decode_time.py measures on the GPU"
    T, B, V = a.T, a.B, a.V
    print("device:", torch.cuda.get_device_name(0))
    print("T4 = %d, B = %d, V = %d; rounds %d x %d calls, alternating; us per call" % (T, B, V, a.rounds, a.calls))
    d = Dictionary.synthetic(V - 5)
    d.add_symbol("<ctc_blank>")
    blank = d.index("<ctc_blank>")
    lens = [T - (b * 75) // max(B - 1, 1) for b in range(B)]
    in_len = torch.tensor(lens, dtype=torch.int32, device=DEV)
    for dtype in (torch.bfloat16, torch.float32):
        logits = make_logits(T, B, V, dtype)
        greedy, pre8, pre16 = CTCDecoder(d), CTCDecoder(d, "prefix", 8, 8, 1), CTCDecoder(d, "prefix", 16, 16, 1)
        routes = [
            ("device  K.ctc_argmax alone (the host route's kernel)", device_time, lambda: K.ctc_argmax(logits)),
            ("device  K.ctc_greedy (row phase + collapse)", device_time, lambda: K.ctc_greedy(logits, in_len, blank)),
            ("device  K.ctc_prefix_beam beam 8 cand 8", device_time, lambda: K.ctc_prefix_beam(logits, in_len, blank, 8, 8, 1)),
            ("device  K.ctc_prefix_beam beam 16 cand 16", device_time, lambda: K.ctc_prefix_beam(logits, in_len, blank, 16, 16, 1)),
            ("to transcripts  host route: ctc_argmax, .cpu(), groupby", wall_time, lambda: host_route(logits, lens, blank)),
            ("to transcripts  CTCDecoder greedy", wall_time, lambda: [h[0]["tokens"].tolist() for h in greedy.decode_logits(logits, in_len)]),
            ("to transcripts  CTCDecoder prefix beam 8 cand 8", wall_time, lambda: [h[0]["tokens"].tolist() for h in pre8.decode_logits(logits, in_len)]),
            ("to transcripts  CTCDecoder prefix beam 16 cand 16", wall_time, lambda: [h[0]["tokens"].tolist() for h in pre16.decode_logits(logits, in_len)]),
        ]
        host = host_route(logits, lens, blank)
        dev = [h[0]["tokens"].tolist() for h in greedy.decode_logits(logits, in_len)]
        p8 = [h[0]["tokens"].tolist() for h in pre8.decode_logits(logits, in_len)]
        print("%s: greedy transcripts equal the host route's: %s; mean length %.1f tokens; prefix (8, 8) differs from greedy in %d of %d sentences"
              % (str(dtype).replace("torch.", ""), host == dev, sum(map(len, dev)) / B, sum(x != y for x, y in zip(p8, dev)), B))
        for _, _, fn in routes:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = [[] for _ in routes]
        for _ in range(a.rounds):
            for i, (_, timer, fn) in enumerate(routes):
                times[i].append(timer(fn, a.calls))
        for (tag, _, _), ts in zip(routes, times):
            print("  %-62s %s -> median %.1f us" % (tag, " ".join("%.1f" % v for v in ts), statistics.median(ts)))
        sys.stdout.flush()
        del logits


if __name__ == "__main__":
    main()
