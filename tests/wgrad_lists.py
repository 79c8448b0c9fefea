"""Named product lists of the grouped weight-gradient tests: each reaches one kind of plan of the host planners
(fbk_fairseq_st_amd/csrc/wgrad_plan.hpp) with tiny products -- the planners count tiles, not their size.

A list is a sequence of (n_out, n_in, tokens).  PLANS states, per list, what the planner makes of it: tests/test_wgrad_plan_cpu.py
proves every row through the host program (tests/host/wgrad_plan_check.cpp), and tests/test_wgrad_group_gpu.py runs the same lists
on the kernels, so a GPU case that says "this list has cut tiles" or "this list runs the fill layout" stands on the CPU assertion.
Pure Python, no torch."""


def one_264x264(tokens):
    """one product of 2 x 2 tiles with ragged edges (8 rows / columns past 256); from 16 K-tiles (961 tokens) on the tiles are cut"""
    return [(264, 264, tokens)]


def whole_round(tokens):
    """256 one-tile products: exactly one round of 256 workgroups, nothing cut; on 240 workgroups a cut tail round of 16"""
    return [(16, 16, tokens)] * 256


def tail_round():
    """260 one-tile products: one whole round and a tail round of 4 tiles, cut into 4 pieces each"""
    return [(16, 16, 2048)] * 260


def fill():
    """two long reductions next to 600 short ones: the fill layout pours the long ones into what the short ones leave free"""
    return [(16, 16, 4096)] * 2 + [(16, 16, 64)] * 600


def second_round():
    """255 one-tile products, then one of three column tiles: 258 whole items on 256 workgroups, nothing cut (two K-tiles are too
    short to cut), so the wide product's tiles (0, 1) and (0, 2) are items 256 and 257: the SECOND items of workgroup slots 0 and 1,
    which start only when tile (0, 0) -- the first and only item of slot 255, as long as theirs -- is about done"""
    return [(16, 16, 128)] * 255 + [(8, 520, 128)]


def cut_f32(tokens):
    """528 one-tile products on the f32 planner's 512 workgroups: at 16 stages (512 tokens) the 16 of the tail round are cut in 8"""
    return [(8, 8, tokens)] * 528


# (name, list, planner, workgroups G (bf16 only), facts).  Facts: items = non-empty work items, cut_tiles = tiles of more than one
# piece, atomic_items = items that add with f32 atomics, pieces = pieces per cut tile (all alike in these lists), layout, and for
# the fill layout its makespan.
PLANS = [
    ("one_264x264 960", one_264x264(960), "bf16", 256, dict(items=4, cut_tiles=0, atomic_items=0, layout="rounds")),
    ("one_264x264 961", one_264x264(961), "bf16", 256, dict(items=8, cut_tiles=4, atomic_items=8, pieces=2, layout="rounds")),
    ("one_264x264 1024", one_264x264(1024), "bf16", 256, dict(items=8, cut_tiles=4, atomic_items=8, pieces=2, layout="rounds")),
    ("one_264x264 1087", one_264x264(1087), "bf16", 256, dict(items=8, cut_tiles=4, atomic_items=8, pieces=2, layout="rounds")),
    ("one_264x264 1536", one_264x264(1536), "bf16", 256, dict(items=12, cut_tiles=4, atomic_items=12, pieces=3, layout="rounds")),
    ("one_264x264 1600", one_264x264(1600), "bf16", 256, dict(items=12, cut_tiles=4, atomic_items=12, pieces=3, layout="rounds")),
    ("whole_round 128", whole_round(128), "bf16", 256, dict(items=256, cut_tiles=0, atomic_items=0, layout="rounds")),
    ("whole_round 2048", whole_round(2048), "bf16", 256, dict(items=256, cut_tiles=0, atomic_items=0, layout="rounds")),
    ("whole_round 2048 G240", whole_round(2048), "bf16", 240, dict(items=304, cut_tiles=16, atomic_items=64, pieces=4, layout="rounds")),
    ("tail_round", tail_round(), "bf16", 256, dict(items=272, cut_tiles=4, atomic_items=16, pieces=4, layout="rounds")),
    ("fill", fill(), "bf16", 256, dict(items=616, cut_tiles=2, atomic_items=16, pieces=8, layout="fill", makespan=34)),
    ("fill G240", fill(), "bf16", 240, dict(items=616, cut_tiles=2, atomic_items=16, pieces=8, layout="fill", makespan=34)),
    ("second_round", second_round(), "bf16", 256, dict(items=258, cut_tiles=0, atomic_items=0, layout="rounds")),
    ("cut_f32 512", cut_f32(512), "f32", 0, dict(items=640, cut_tiles=16, atomic_items=128, pieces=8, layout="f32")),
    ("cut_f32 480", cut_f32(480), "f32", 0, dict(items=528, cut_tiles=0, atomic_items=0, layout="f32")),
]
