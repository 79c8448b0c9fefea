"""The comparison itself, tested with wrong twins: tests/grad_compare.py against planted defects of the size a lost tile leaves.

The reference is a random [2048, 512] tensor (an fc1 weight gradient's shape) and a random [8000, 512] one (the decoder embedding).
A clean `mine` is the reference plus iid noise of relative size 0.07 (what bf16 storage leaves on a gradient of the m preset:
1 - cos ~ 2.5e-3) or 1e-6 (fp32).  Planted into `mine`:
  (a) rows 960..991 zeroed (half a 64-row block)       (b) one 64-row block scaled by 2        (c) two 64-row blocks swapped
  (d) one 16-element run zeroed                        (e) one row of the embedding zeroed

What the whole-tensor criteria of test_configs_gpu.compare_grads (norm and cosine at TOL's values) make of them -- the hole:
  bf16 (norm 5e-2, cosine 0.99)     (a) removes 1/64 of the energy: cosine sqrt(1 - 1/64) = 0.9922, norm error 7.8e-3: ACCEPTED.
                                    (b) on the [8000, 512] tensor (1/125 of the energy doubled): cosine 0.9961, norm 1.2e-2: ACCEPTED.
  fp32 (norm 1e-3, cosine 0.9999)   (d) 16 of 2048 x 512 elements, 1.5e-5 of the energy: ACCEPTED.  (e) one of 8000 rows, 1.25e-4 of
                                    the energy: cosine 0.99994, norm 6.3e-5: ACCEPTED.
Those four are asserted on the defect alone (no noise): that is the arithmetic.  Arithmetic also says where the whole-tensor criteria
do NOT leave a hole, and the test states it instead of pretending: on top of 0.07 of noise (cosine 0.99756 by itself) defect (a)
comes to 0.9922 x 0.99756 = 0.98974, a hair UNDER 0.99 -- the present bound catches a lost half-block only when the honest noise is
already at its worst; at the 0.05 a typical tensor carries it passes (0.9909).  (b) on the [2048, 512] tensor has cosine 0.9861 and
(c) has 1 - 2/32 = 0.9375 (on 8000 rows 1 - 2/125 = 0.984): the old criteria reject those.

The new criteria must reject every one of (a)..(e) and accept the clean twin:
  fp32   elementwise():  max|mine - ref| <= 1e-4 max|ref|
  bf16   worst_block():  every block's error within margin x null spread of the whole tensor's; margin 3 (test_configs_gpu.BLOCK_MARGIN),
         null spread measured on a pair that differs by noise only.  (a) gives r_i = sqrt(1/2), r = sqrt(0.07^2 + 1/64) = 0.143, so
         4.9: margin x null spread may reach 4.9 before (a) passes, i.e. a null spread of 1.63 at margin 3.
"""
import math

import pytest
import torch

import grad_compare as gc
from test_configs_gpu import BLOCK_MARGIN, FP32_NORTH_STAR, TOL, compare_grads

BF16_NOISE, FP32_NOISE = 0.07, 1e-6


def _noisy(ref, level, seed):
    g = torch.Generator().manual_seed(seed)
    n = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    return ref + n * (level * float(ref.norm()) / float(n.norm()))


@pytest.fixture(scope="module")
def refs():
    g = torch.Generator().manual_seed(0)
    return dict(w=torch.randn(2048, 512, generator=g, dtype=torch.float64), emb=torch.randn(8000, 512, generator=g, dtype=torch.float64))


def plant(name, x):
    x = x.clone()
    if name == "a":
        x[960:992] = 0
    elif name == "b":
        x[640:704] *= 2
    elif name == "c":
        lo, hi = x[128:192].clone(), x[1792:1856].clone()
        x[128:192], x[1792:1856] = hi, lo
    elif name == "d":
        x[777, 208:224] = 0
    elif name == "e":
        x[4321] = 0
    return x


def old_accepts(mine, ref, dtype):
    """the whole-tensor criteria as the config tests apply them"""
    t = TOL[dtype]
    try:
        compare_grads({"w": mine.float()}, {"w": ref.float()}, t["grad"], t["cos"], what="twin")
    except AssertionError:
        return False
    return True


def new_accepts_fp32(mine, ref):
    return gc.elementwise(mine, ref)[0] <= FP32_NORTH_STAR


def new_accepts_bf16(mine, ref, null):
    return gc.worst_block(mine, ref, null)[0] <= BLOCK_MARGIN


def test_elementwise_names_the_element():
    ref = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    mine = ref.clone()
    mine[1, 2, 0] += 2.3
    e, idx = gc.elementwise(mine, ref)
    assert idx == (1, 2, 0) and abs(e - 2.3 / 23.0) < 1e-6
    assert gc.elementwise(ref, ref) == (0.0, (0, 0, 0))
    assert gc.elementwise({"x": mine}, {"x": ref})["x"][1] == (1, 2, 0)
    assert gc.elementwise(torch.ones(3), torch.zeros(3))[0] == math.inf


def test_blocks_shares_errors_and_the_low_energy_rule():
    ref = torch.zeros(200, 8, dtype=torch.float64)
    ref[:64] = 1.0                     # block 0 carries 64 x 8 of the energy
    ref[64:128] = 2.0                  # block 1 four times that
    ref[130, 3] = 0.5                  # block 2 next to nothing; block 3 (8 rows: the short tail) nothing at all
    mine = ref.clone()
    mine[:64] *= 1.5
    mine[199, 0] = 0.25
    k = gc.blocks(mine, ref)
    assert k["n"] == 4 and k["rows"] == 64
    e = 64 * 8.0
    tot = 5 * e + 0.25
    assert k["share"] == pytest.approx([e / tot, 4 * e / tot, 0.25 / tot, 0.0])
    assert list(k["low"]) == [False, False, True, True]
    assert k["rel"][0] == pytest.approx(0.5) and k["rel"][1] == 0 and math.isnan(k["rel"][3])
    assert k["cos"][0] == pytest.approx(1.0) and k["abs"][3] == pytest.approx(0.25)
    assert k["r"] == pytest.approx(math.sqrt((0.25 * e + 0.0625) / tot))
    # 1-D tensors: runs of 512
    v = torch.arange(1100, dtype=torch.float64) + 1
    k1 = gc.blocks(v * 1.01, v)
    assert k1["n"] == 3 and k1["rows"] == gc.RUN_1D and k1["rel"] == pytest.approx([0.01] * 3)
    assert gc.spread(v * 1.01, v) == pytest.approx(1.0) and gc.spread(v, v) == 1.0
    # an error that sits in a block whose reference is zero is seen through its absolute size
    fig, i, _ = gc.worst_block(mine, ref)
    assert i == 0 and fig == pytest.approx(0.5 / k["r"])
    only_tail = ref.clone()
    only_tail[199, 0] = 100.0
    fig, i, _ = gc.worst_block(only_tail, ref)
    assert i == 3 and fig == pytest.approx(2.0)          # the whole error in one of four blocks: sqrt(4) times its equal share


def test_null_spread_of_iid_noise_is_one(refs):
    for level in (BF16_NOISE, FP32_NOISE):
        s = gc.spread(_noisy(refs["w"], level, 5), refs["w"])
        assert 1.0 <= s < 1.03, s          # 32 blocks of 32768 elements: the largest block error is within ~1 % of the mean


@pytest.mark.parametrize("defect,which", [("a", "w"), ("b", "w"), ("b", "emb"), ("c", "w"), ("c", "emb")])
def test_bf16_block_criteria_reject_the_planted_defect(refs, defect, which):
    ref = refs[which]
    clean = _noisy(ref, BF16_NOISE, 1)
    null = gc.spread(_noisy(ref, BF16_NOISE, 2), ref)           # measured on another noise-only pair, never on `mine`
    assert old_accepts(clean, ref, torch.bfloat16) and new_accepts_bf16(clean, ref, null)
    bad = plant(defect, clean)
    fig, blk, k = gc.worst_block(bad, ref, null)
    print("defect (%s) on %s: block figure %.2f at block %d (whole-tensor r %.3f), old criteria accept the bare defect: %s" %
          (defect, tuple(ref.shape), fig, blk, k["r"], old_accepts(plant(defect, ref), ref, torch.bfloat16)))
    assert not new_accepts_bf16(bad, ref, null), (defect, fig)
    assert blk in {"a": (15,), "b": (10,), "c": (2, 28)}[defect]
    # the hole, where the arithmetic says there is one (module docstring)
    hole = (defect, which) in (("a", "w"), ("b", "emb"))
    assert old_accepts(plant(defect, ref), ref, torch.bfloat16) == hole
    if hole:
        assert not new_accepts_bf16(plant(defect, ref), ref, null)


def test_bf16_defect_a_figures_are_the_arithmetic(refs):
    ref = refs["w"]
    bare = plant("a", ref)
    cos = float(torch.nn.functional.cosine_similarity(bare.reshape(1, -1), ref.reshape(1, -1)))
    assert cos == pytest.approx(math.sqrt(1 - 1 / 64), abs=2e-4) and cos >= TOL[torch.bfloat16]["cos"]
    assert abs(float(bare.norm()) / float(ref.norm()) - 1) == pytest.approx(7.8e-3, abs=2e-4)
    noisy = plant("a", _noisy(ref, BF16_NOISE, 1))
    cosn = float(torch.nn.functional.cosine_similarity(noisy.reshape(1, -1), ref.reshape(1, -1)))
    assert cosn == pytest.approx(0.98974, abs=3e-4)             # with the worst honest noise on top: just under 0.99
    assert old_accepts(plant("a", _noisy(ref, 0.05, 1)), ref, torch.bfloat16)          # with typical noise: through the hole
    fig = gc.worst_block(noisy, ref)[0]
    assert fig == pytest.approx(math.sqrt(0.5 / (BF16_NOISE ** 2 + 1 / 64)), rel=0.02)  # 4.9
    # the largest null spread at which margin x null spread still rejects (a): what the GPU test's margin has to stay under
    assert BLOCK_MARGIN * 1.6 < fig


@pytest.mark.parametrize("defect,which", [("a", "w"), ("b", "w"), ("c", "w"), ("d", "w"), ("e", "emb")])
def test_fp32_element_criterion_rejects_the_planted_defect(refs, defect, which):
    ref = refs[which]
    clean = _noisy(ref, FP32_NOISE, 3)
    assert old_accepts(clean, ref, torch.float32) and new_accepts_fp32(clean, ref)
    bad = plant(defect, clean)
    e, idx = gc.elementwise(bad, ref)
    print("defect (%s): element figure %.3g at %s, old criteria accept: %s" % (defect, e, idx, old_accepts(bad, ref, torch.float32)))
    assert not new_accepts_fp32(bad, ref)
    assert old_accepts(bad, ref, torch.float32) == (defect in "de")          # the hole: (d) 1.5e-5 and (e) 1.25e-4 of the energy
    lo, hi = {"a": (960, 992), "b": (640, 704), "c": (128, 1856), "d": (777, 778), "e": (4321, 4322)}[defect]
    assert lo <= idx[0] < hi
    if defect == "d":
        assert 208 <= idx[1] < 224


@pytest.mark.parametrize("null", [1.0, 1.19, 1.39, 1.8])
def test_block_check_rejects_defect_a_on_the_ctc_head_at_its_class_margin(monkeypatch, null):
    """test_configs_gpu.block_check itself -- tensor selection, the class margin of encoder.ctc_fc.weight (7.2) and the half-block cap
    -- on a [5001, 512] tensor of that name (79 blocks) next to an fc1 weight (32 blocks, margin 3): the clean twin passes, half a
    block zeroed in either tensor fails, at the null spreads hosts have measured for the CTC head (1.19, 1.39) and beyond.  Without
    the cap, 7.2 x 1.19 = 8.6 would let the 6.6 of defect (a) on 79 blocks through."""
    import test_configs_gpu as C
    g = torch.Generator().manual_seed(4)
    ref = {"encoder.ctc_fc.weight": torch.randn(5001, 512, generator=g, dtype=torch.float64),
           "encoder.layers.0.fc1.weight": torch.randn(2048, 512, generator=g, dtype=torch.float64),
           "encoder.layers.0.self_attn.k_proj.bias": torch.zeros(512, dtype=torch.float64),        # never selected
           "tiny.weight": 1e-5 * torch.randn(64, 64, generator=g, dtype=torch.float64)}            # below 1e-3 of the largest norm
    monkeypatch.setattr(C, "null_spreads", lambda: dict(null={"encoder.ctc_fc.weight": null, "encoder.layers.0.fc1.weight": min(null, 1.55)}))
    clean = {k: _noisy(v, BF16_NOISE, 11 + i) if float(v.norm()) > 0 else v.clone() for i, (k, v) in enumerate(ref.items())}
    clean["tiny.weight"] = ref["tiny.weight"] * 3          # wrong, but carries no signal: the selection of compare_grads' cosine skips it
    worst = C.block_check(clean, ref, "twin")
    assert worst[0] < 0.5, worst
    for name, rows in (("encoder.ctc_fc.weight", slice(3520, 3552)), ("encoder.layers.0.fc1.weight", slice(960, 992))):
        bad = dict(clean)
        bad[name] = clean[name].clone()
        bad[name][rows] = 0
        assert old_accepts(bad[name], ref[name], torch.bfloat16) == (name == "encoder.ctc_fc.weight")      # 1/158 of the energy: the hole
        with pytest.raises(AssertionError, match="%s block %d" % (name, rows.start // 64)):
            C.block_check(bad, ref, "twin")
