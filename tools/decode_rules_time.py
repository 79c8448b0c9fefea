#!/usr/bin/env python3
"""ms per decode step of beam-5 generation at the Cfg5 shape (bench.py cfg5_beam5: s2t_transformer_m, 16 utterances x 1000 frames,
max_len_b 200, random-init weights) with and without the score rules of s2t_decode_step_rules, in ONE process:

  a  plain        the device-resident search (s2t_decode_step)
  b  ngram3       the device-resident search with --no-repeat-ngram-size 3
  c  prefix2      the device-resident search with two forced tokens per sentence
  d  step-ngram3  the step-by-step search (S2T_DEVICE_SEARCH=0) with --no-repeat-ngram-size 3: what b replaced

  python tools/decode_rules_time.py [--dtypes bf16,fp32] [--variants a,b,c,d] [--runs 3]

Per variant: one warm-up call, then `runs` timed calls; a call's figure is search time / steps (SequenceGenerator.record_stats: two
host synchronisations around the search, the encoder is outside).  Printed: every call's figure, so that the run-to-run spread is on the
page beside the differences.  `--variants a` runs on a tree that predates the rules (the parent commit's plain route on the same box).
"""
import argparse
import os
import socket
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VARIANTS = {"a": ("plain", True, 0, False), "b": ("ngram3", True, 3, False), "c": ("prefix2", True, 0, True),
            "d": ("step-ngram3", False, 3, False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--variants", default="a,b,c,d")
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    import bench
    from fbk_fairseq_st_amd import lib as L
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    B, T, BEAM, MAXLEN = 16, 1000, 5, 200
    dev = torch.device("cuda:0")
    print("# host %s, %s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0), L.load().s2t_build_info().decode()))
    print("# s2t_transformer_m, %d x %d frames, beam %d, max_len_b %d; ms per decode step = search time / steps" % (B, T, BEAM, MAXLEN))
    for dn in args.dtypes.split(","):
        dtype = torch.bfloat16 if dn == "bf16" else torch.float32
        a, task, model, crit, trainer, _ = bench.build_all("s2t_transformer_m", B, T, 40, 0, 1e-9, dtype, dev,
                                                           criterion="label_smoothed_cross_entropy", max_target_positions=1024)
        model.eval()
        sample = trainer.prepare(task.dummy_batch(seed=100))
        net = {"net_input": {k: v for k, v in sample["net_input"].items() if k in ("src_tokens", "src_lengths")}}
        prefix = torch.stack([torch.arange(B) % 50 + 10, torch.arange(B) % 70 + 100], 1).to(dev)       # neither pad nor EOS
        mean = {}
        for v in args.variants.split(","):
            name, device_route, ngram, with_prefix = VARIANTS[v]
            os.environ["S2T_DEVICE_SEARCH"] = "1" if device_route else "0"
            kw = dict(no_repeat_ngram_size=ngram) if ngram else {}
            gen = SequenceGenerator([model], task.target_dictionary, beam_size=BEAM, max_len_a=0.0, max_len_b=MAXLEN, min_len=1, **kw)
            gen.record_stats = True
            call = lambda: gen.generate([model], net, prefix_tokens=prefix if with_prefix else None)
            call()
            ms, steps = [], 0
            for _ in range(args.runs if device_route else 1):
                gen.last_stats = {}
                call()
                st = gen.last_stats
                assert ("launches_per_step" in st) == device_route, "variant %s took the other route" % name
                steps = st["steps"]
                ms.append(st["search_s"] * 1e3 / steps)
            mean[v] = sum(ms) / len(ms)
            print("%-5s %s %-12s steps %3d  ms/step %s  mean %.4f" % (dn, v, name, steps, " ".join("%.4f" % m for m in ms), mean[v]))
        os.environ["S2T_DEVICE_SEARCH"] = "1"
        if "a" in mean and "b" in mean:
            print("%-5s rules phase (b - a) %+.4f ms/step%s" % (dn, mean["b"] - mean["a"],
                                                                "; prefix (c - a) %+.4f" % (mean["c"] - mean["a"]) if "c" in mean else ""))
        if "d" in mean and "b" in mean:
            print("%-5s step route / device route with n = 3: %.1fx" % (dn, mean["d"] / mean["b"]))
        del trainer, model, crit, task
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
