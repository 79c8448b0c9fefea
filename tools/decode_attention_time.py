#!/usr/bin/env python3
"""ms per decode step of generation at the Cfg5 shape (bench.py cfg5_beam5: s2t_transformer_m, 16 utterances x 1000 frames, beam 5,
max_len_b 200, random-init weights) with the two S2TDecodeExtras options of the device search, on ONE box in one job:

  (a) the plain search, another build of the library (--parent-lib: the parent commit's libs2t_hip.so) against this one, alternating,
      each call of a build in a process of its own (a process loads one library; both through S2T_HIP_LIB, i.e. the ctypes binding):
      the recording and LayerNorm forms are template parameters and may not cost the plain instantiations anything;
  (b) the search with attention recorded (retain_attention) beside the plain one, and the same search on the step-by-step route
      (S2T_DEVICE_SEARCH=0), one process;
  (c) a --layernorm-embedding model: device route, device route with attention, step-by-step route, one process.

  python tools/decode_attention_time.py [--parent-lib PATH] [--dtypes bf16,fp32] [--runs 3] [--rounds 3]

A call's figure is search time / steps (SequenceGenerator.record_stats: two host synchronisations around the search, the encoder is
outside; the hypotheses' read-back, with the attention gather, is inside).  Every call's figure is printed, so that the run-to-run spread
is on the page beside the differences.
"""
import argparse
import os
import socket
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

B, T, MAXLEN, BEAM = 16, 1000, 200, 5
NEW = ("s2t_decode_begin_ex", "s2t_decode_step_ex", "s2t_decode_graph_create_ex")
#            name                         device route  attention
VARIANTS = {"plain": ("plain", True, False), "attn": ("attention", True, True), "step": ("step-route plain", False, False),
            "step_attn": ("step-route attention", False, True)}


def child(args):
    import torch
    import bench
    from fbk_fairseq_st_amd import lib as L
    from fbk_fairseq_st_amd import sequence_generator as SG
    if args.label == "parent":                                  # a library from before the *_ex entry points: bind what it has
        for n in NEW:
            L.SIGNATURES.pop(n, None)
    dev = torch.device("cuda:0")
    print("# %s: host %s, %s, %s" % (args.label, socket.gethostname(), torch.cuda.get_device_name(0), L.load().s2t_build_info().decode()), flush=True)
    over = dict(layernorm_embedding=True) if args.lne else {}
    for dn in args.dtypes.split(","):
        dtype = torch.bfloat16 if dn == "bf16" else torch.float32
        a, task, model, crit, trainer, _ = bench.build_all("s2t_transformer_m", B, T, 40, 0, 1e-9, dtype, dev,
                                                           criterion="label_smoothed_cross_entropy", max_target_positions=1024, **over)
        assert bool(model.hp.layernorm_embedding) == bool(args.lne)
        model.eval()
        sample = trainer.prepare(task.dummy_batch(seed=100))
        net = {"net_input": {k: v for k, v in sample["net_input"].items() if k in ("src_tokens", "src_lengths")}}
        for v in args.variants.split(","):
            name, device_route, attention = VARIANTS[v]
            name = ("lne " if args.lne else "") + name
            os.environ["S2T_DEVICE_SEARCH"] = "1" if device_route else "0"
            gen = SG.SequenceGenerator([model], task.target_dictionary, beam_size=BEAM, max_len_a=0.0, max_len_b=MAXLEN, min_len=1,
                                       retain_attention=attention)
            gen.record_stats = True
            hyps = gen.generate([model], net)
            assert (hyps[0][0]["attention"] is not None) == attention
            ms, steps = [], 0
            for _ in range(args.runs if device_route else 1):
                gen.last_stats = {}
                gen.generate([model], net)
                st = gen.last_stats
                assert ("launches_per_step" in st) == device_route, "variant %s took the other route" % name
                steps = st["steps"]
                ms.append(st["search_s"] * 1e3 / steps)
            print("%-5s %-8s %-26s steps %3d  ms/step %s  mean %.4f" % (dn, args.label, name, steps, " ".join("%.4f" % m for m in ms),
                                                                       sum(ms) / len(ms)), flush=True)
        del trainer, model, crit, task
        torch.cuda.empty_cache()


def run_child(label, lib, variants, args, lne=False):
    """one fresh process per call of a build: the library is loaded once per process"""
    env = dict(os.environ)
    if lib:
        env["S2T_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--variants", variants, "--dtypes", args.dtypes,
           "--runs", str(args.runs)] + (["--lne"] if lne else [])
    res = subprocess.run(cmd, env=env, timeout=args.child_timeout)
    if res.returncode != 0:
        raise SystemExit("%s: child exited with %d; nothing more is started" % (label, res.returncode))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lne", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--variants", default="plain,attn,step,step_attn")
    args = ap.parse_args()
    if args.child:
        return child(args)
    print("# s2t_transformer_m, %d x %d frames, beam %d, max_len_b %d; ms per decode step = search time / steps" % (B, T, BEAM, MAXLEN), flush=True)
    if args.parent_lib:
        from fbk_fairseq_st_amd import lib as L           # the path only: nothing is loaded in this process
        this = os.path.join(os.path.dirname(L.__file__), "libs2t_hip.so")
        print("# (a) plain search: parent build / this build, alternating, one process per call", flush=True)
        for _ in range(args.rounds):
            run_child("parent", os.path.abspath(args.parent_lib), "plain", args)
            run_child("this", this, "plain", args)
    print("# (b) attention recorded beside the plain search, and the step-by-step route; one process", flush=True)
    run_child("this", "", args.variants, args)
    print("# (c) a --layernorm-embedding model: device route, with attention, step-by-step route; one process", flush=True)
    run_child("this", "", "plain,attn,step", args, lne=True)


if __name__ == "__main__":
    main()
