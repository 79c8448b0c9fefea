#!/usr/bin/env python3
"""ms per decode step of generation at the Cfg5 shape (bench.py cfg5_beam5: s2t_transformer_m, 16 utterances x 1000 frames, beam 5,
max_len_b 200, random-init weights) with the sampling search (`Sampling`: unrestricted, top-k 10, top-p 0.9), on ONE box in one job:

  (a) plain beam search at beam 5, another build of the library (--parent-lib: the parent commit's libs2t_hip.so) against this one,
      alternating, each call of a build in a process of its own (a process loads one library; both through S2T_HIP_LIB, i.e. the
      ctypes binding): the sampling forms are template parameters of the per-row and per-sentence kernels and may not cost the plain
      ones anything;
  (b) the three sampling searches beside the plain search, device route, one process;
  (c) the same sampling searches on the step-by-step route (S2T_DEVICE_SEARCH=0: s2t_sample_rows per step).

  python tools/decode_sampling_time.py [--parent-lib PATH] [--dtypes bf16,fp32] [--runs 3] [--rounds 2]

A call's figure is search time / steps (SequenceGenerator.record_stats: two host synchronisations around the search, the encoder is
outside).  Every call's figure is printed, so that the run-to-run spread is on the page beside the differences.
"""
import argparse
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, T, MAXLEN, BEAM = 16, 1000, 200, 5
NEW_SYMBOLS = ("s2t_sample_rows", "s2t_decode_step_sample", "s2t_decode_graph_create_sample")
#            name               device route  sampling  topk  topp
VARIANTS = {"plain": ("plain b5", True, False, -1, -1.0), "samp": ("sampling b5", True, True, -1, -1.0),
            "topk": ("sampling b5 top-k 10", True, True, 10, -1.0), "topp": ("sampling b5 top-p 0.9", True, True, -1, 0.9),
            "step_samp": ("step-route sampling b5", False, True, -1, -1.0), "step_topk": ("step-route top-k 10", False, True, 10, -1.0),
            "step_topp": ("step-route top-p 0.9", False, True, -1, 0.9)}


def child(args):
    import torch
    from fbk_fairseq_st_amd import lib as L
    if args.label == "parent":                                  # a library from before the sampling entry points: bind what it has
        for n in NEW_SYMBOLS:
            L.SIGNATURES.pop(n, None)
    import bench
    from fbk_fairseq_st_amd import sequence_generator as SG
    dev = torch.device("cuda:0")
    print("# %s: host %s, %s, %s" % (args.label, socket.gethostname(), torch.cuda.get_device_name(0), L.load().s2t_build_info().decode()), flush=True)
    for dn in args.dtypes.split(","):
        dtype = torch.bfloat16 if dn == "bf16" else torch.float32
        a, task, model, crit, trainer, _ = bench.build_all("s2t_transformer_m", B, T, 40, 0, 1e-9, dtype, dev,
                                                           criterion="label_smoothed_cross_entropy", max_target_positions=1024)
        model.eval()
        sample = trainer.prepare(task.dummy_batch(seed=100))
        net = {"net_input": {k: v for k, v in sample["net_input"].items() if k in ("src_tokens", "src_lengths")}}
        for v in args.variants.split(","):
            name, device_route, sampling, topk, topp = VARIANTS[v]
            os.environ["S2T_DEVICE_SEARCH"] = "1" if device_route else "0"
            kw = dict(search_strategy=SG.Sampling(task.target_dictionary, topk, topp, seed=1)) if sampling else {}
            gen = SG.SequenceGenerator([model], task.target_dictionary, beam_size=BEAM, max_len_a=0.0, max_len_b=MAXLEN, min_len=1, **kw)
            gen.record_stats = True
            gen.generate([model], net)
            ms, steps = [], []
            for _ in range(args.runs if device_route else 1):
                gen.last_stats = {}
                gen.generate([model], net)
                st = gen.last_stats
                assert ("launches_per_step" in st) == device_route, "variant %s took the other route" % name
                steps.append(st["steps"])
                ms.append(st["search_s"] * 1e3 / st["steps"])
            print("%-5s %-8s %-26s steps %-12s ms/step %s  mean %.4f" % (dn, args.label, name, ",".join(str(s) for s in steps),
                                                                        " ".join("%.4f" % m for m in ms), sum(ms) / len(ms)), flush=True)
        del trainer, model, crit, task
        torch.cuda.empty_cache()


def run_child(label, lib, variants, args):
    """one fresh process per call of a build: the library is loaded once per process"""
    env = dict(os.environ)
    if lib:
        env["S2T_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--variants", variants, "--dtypes", args.dtypes,
           "--runs", str(args.runs)]
    res = subprocess.run(cmd, env=env, timeout=args.child_timeout)
    if res.returncode != 0:
        raise SystemExit("%s: child exited with %d; nothing more is started" % (label, res.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--variants", default="plain,samp,topk,topp,step_samp,step_topk,step_topp")
    args = ap.parse_args()
    if args.child:
        return child(args)
    print("# s2t_transformer_m, %d x %d frames, beam %d, max_len_b %d; ms per decode step = search time / steps" % (B, T, BEAM, MAXLEN), flush=True)
    if args.parent_lib:
        from fbk_fairseq_st_amd import lib as L           # the path only: nothing is loaded in this process
        this = os.path.join(os.path.dirname(L.__file__), "libs2t_hip.so")
        print("# (a) plain beam 5: parent build / this build, alternating, one process per call", flush=True)
        for _ in range(args.rounds):
            run_child("parent", os.path.abspath(args.parent_lib), "plain", args)
            run_child("this", this, "plain", args)
    print("# (b) sampling beside plain on the device route, (c) the step-by-step route; one process", flush=True)
    run_child("this", "", args.variants, args)


if __name__ == "__main__":
    main()
