"""The grouped weight-gradient kernels at their edges, element by element against float64:
    s2t_wgrad_group      (bf16 operands, csrc/wgrad_group.hip)       dW_p[n_out][n_in] += dY_p[tokens][n_out]^T X_p[tokens][n_in]
    s2t_wgrad_group_f32  (f32 operands,  csrc/wgrad_f32.hip)         db_p[n_out]       += column sums of dY_p
tests/test_kernels_gpu.py and tests/test_routes_gpu.py run training-sized lists; here are the smallest shapes at which each path of
the kernels and of their host planners (csrc/wgrad_plan.hpp) runs: reductions shorter than the software pipeline, outputs at the
minimum width and around every internal boundary, dW / db that are views inside guarded buffers (all three epilogue forms of the bf16
kernel), operand padding and the rows after `tokens` filled with NaN or Inf, the planner's cuts and its fill layout, the list cache
of the bf16 entry point, and the refusals.  WHICH plan a list gets (cut tiles, atomics, fill layout) is proven without a GPU by
tests/test_wgrad_plan_cpu.py on the named lists of tests/wgrad_lists.py; the cases here cite that table.

References: fp64 on the CPU from the exact operand values (bf16 widened exactly).  Every output element is compared, NaN and Inf
count as errors, and every element of the guarded buffers outside [n_out][n_in] must keep its bits.  Two operand sets per case:
  * integer-exact: integers in [-4, 4] for dY, X, dW0 and db0.  Every product and every partial sum is an integer below
    16 tokens + 4 < 2^24, hence exact in f32 in ANY order, cut or not, atomic or not: the result must equal the reference bit for
    bit, and a second run must repeat it.
  * normal: randn / 2.  Both kernels multiply exactly (bf16 x bf16 in f32) or with one rounding (the exact-f32 MFMA) and add T
    products in some f32 order: any order errs by at most (T - 1) u sum_t |dy_ti x_tj| (u = 2^-24), plus one u per product and the
    partial sums between K-tiles / stages, which the factor 4 covers (the derivation of Gemm in tests/test_routes_gpu.py).  The
    tile's token range may be cut into pieces, at most one per K-tile (bf16: 64 tokens) or stage (f32: 32 tokens), nk in all, that
    are added to dW0 one after the other: each add rounds once, at most u (|dW0| + |ref|).  So
        |dW - ref| <= 4 T u (|dY|^T |X|) + (nk + 1) u (|dW0| + |ref|)         |db - ref| <= 4 T u sum_t |dY| + (nk + 1) u (|db0| + |ref|)
    A dropped or doubled K-tile, a row read past `tokens` or a padding column that reaches an output misses these by orders of
    magnitude.

Which case catches which mistake.  Each line is a one-line change of the library, built separately and run on the named cases of
this file (with `-x`: the case is the first that failed) and, for the two planner changes, through the host program as well.
Every change only reads inside the three spare operand rows or writes inside the guarded buffers.
  * wgrad_group_kernel, stage guard `< tokens_left` -> `<=` (reads row `tokens`): test_bf16_one_product[t5_8x8_dense_db_nan],
    all 64 elements NaN.
  * wgrad_group_kernel, `do_rs` without `tn == 0` (every column tile adds the bias gradient): NOT caught by db on (264, 520) or by
    any list of one whose tiles are whole -- the column tiles run side by side, read the same db0 and store the same sum.  Caught
    where the adds cannot collide: test_bf16_one_264x264_whole_and_cut[961-*, 1087-*, 1600-*] (atomic pieces: db0 + 2 sums) and
    test_bf16_db_comes_from_the_first_column_tile_only (tiles (0, 1), (0, 2) in a second round), which was added for it.
  * wgrad_group_kernel, element-wise epilogue `col + e < P.n_in` -> `<=`: test_bf16_one_product[t5_9x15_dense_db_inf], one guard
    element behind the last row changed (inside the matrix the extra add lands on the next row's first element, also an error).
  * layout_rounds, tail cut keeps `t.atomic` instead of 1: the host program ("several pieces => atomic", on tail_round and on the
    third random list) and test_bf16_tail_round (item 256: 8 where 595 is due, the four pieces overwrite each other).
  * plan_f32, cut pieces pushed with atomic = 0: the host program (cut_f32 512, the 16th random list) and
    test_f32_tail_round_cut[512] (item 512: -40 for -329).
  * wgrad_f32_kernel, fetch guard `k < P.tokens` -> `<=`: test_f32_one_product[t7_1x1_dense_db_nan], NaN.
  * s2t_wgrad_group, cache key compared without its last 24 bytes: test_bf16_lists_that_differ_in_one_field at "64 of 128
    tokens" (the cached 128-token table ran: 69,183 of 69,696 elements wrong).
"""
import contextlib
import ctypes
import math

import numpy as np
import pytest
import torch

import wgrad_lists

pytestmark = pytest.mark.gpu

K = None
L = None
DEV = "cuda"
U32 = 2.0 ** -24                 # unit roundoff of f32
BF, F32 = torch.bfloat16, torch.float32
GUARD = 77.0
EINVAL = -22
FAMILY = {BF: "wgrad_group", F32: "wgrad_group_f32"}
KTILE = {BF: 64, F32: 32}        # tokens per K-tile (bf16) / stage (f32)
CHUNK = {BF: 8, F32: 4}          # elements of a 16-byte operand chunk
PLACEMENTS = ("dense", "odd", "padded")


@pytest.fixture(scope="module", autouse=True)
def _k():
    global K, L
    from fbk_fairseq_st_amd import kernels, lib
    K, L = kernels, lib
    K._lib()
    yield
    K.prof_enable(0)


# ------------------------------------------------------------------ shared tools
@contextlib.contextmanager
def set_option(key, value):
    """s2t_set_option for the duration of a `with` block; the previous value is restored even when the block fails"""
    old = K.set_option(key, value)
    try:
        yield old
    finally:
        K.set_option(key, old)


@contextlib.contextmanager
def launches():
    """launch counts of the two families for everything run inside the block (the library's event-bracketed profiler)"""
    counts = {}
    torch.cuda.synchronize()
    K.prof_reset()
    K.prof_enable(1)
    try:
        yield counts
    finally:
        torch.cuda.synchronize()
        for f in FAMILY.values():
            counts[f] = K.prof_read(f)["launches"]
        K.prof_enable(0)
        K.prof_reset()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def round_up(v, m):
    return (v + m - 1) // m * m


def assert_close(out, ref, bound, what):
    """|out - ref| <= bound element by element (ref, bound float64); on failure: the worst element, its value, ref and bound"""
    o = out.detach().cpu().double()
    err = (o - ref).abs()
    bad = ~(err <= bound)                  # NaN counts as bad
    if bool(bad.any()):
        ratio = torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, math.inf), ratio)
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape)))
        raise AssertionError("%s: %d of %d elements out of bound; worst at %s: out %.9g ref %.9g |err| %.3g bound %.3g"
                             % (what, int(bad.sum()), bad.numel(), idx, float(o[idx]), float(ref[idx]), float(err[idx]), float(bound[idx])))


class Arena:
    """f32 outputs as views inside one buffer filled with GUARD: every element outside the views must keep its bits"""

    def __init__(self):
        self.cursor, self.specs, self.buf = 0, [], None

    def matrix(self, n_out, n_in, placement):
        """dense: ldw = n_in, 16-byte aligned base; odd: ldw = n_in + 5, base one float in (the scalar and element-wise epilogues);
        padded: ldw = round_up(n_in, 4) + 4, base four floats in (aligned rows, ldw > n_in: the interior form is eligible).
        At least one guard row above; finish() adds the one below."""
        ldw, shift = {"dense": (n_in, 0), "odd": (n_in + 5, 1), "padded": (round_up(n_in, 4) + 4, 4)}[placement]
        return self.at(round_up(self.cursor + ldw, 4) + shift, n_out, n_in, ldw)

    def at(self, start, n_out, n_in, ldw):
        self.specs.append((start, n_out, n_in, ldw))
        self.cursor = max(self.cursor, start + (n_out - 1) * ldw + n_in)
        return len(self.specs) - 1

    def vector(self, n):
        """a db: one float into its guard band (4-byte aligned only)"""
        return self.at(round_up(self.cursor + 1, 4) + 1, 1, n, n)

    def finish(self):
        self.size = self.cursor + max(s[3] for s in self.specs) + 8
        self.buf = torch.full((self.size,), GUARD, dtype=F32, device=DEV)
        return self

    def view(self, i, buf=None):
        start, n_out, n_in, ldw = self.specs[i]
        return (self.buf if buf is None else buf).as_strided((n_out, n_in), (ldw, 1), start)

    def guards_intact(self, what, only=None):
        """`only`: the views that count as outputs (default: all); everything else is guard"""
        host = self.buf.cpu()
        keep = torch.ones(self.size, dtype=torch.bool)
        for i in (range(len(self.specs)) if only is None else only):
            self.view(i, keep).fill_(False)
        want = bits(torch.full((1,), GUARD))[0]
        wrong = np.flatnonzero(bits(host)[keep.numpy()] != want)
        assert wrong.size == 0, "%s: %d guard elements changed, first at guard index %d (of %d)" % (what, wrong.size, int(wrong[0]), int(keep.sum()))
        return host


def values(gen, kind, dt, *shape):
    """host f32 tensor of values that `dt` holds exactly"""
    if kind == "int":
        return torch.randint(-4, 5, shape, generator=gen).float()
    v = torch.randn(*shape, generator=gen) * 0.5
    return v.to(dt).float() if dt == BF else v


def operand(host, dt, poison):
    """the [T][cols] values as the top-left view of a device buffer of T + 3 rows whose row stride leaves at least one whole
    16-byte chunk of padding; every element outside the view is `poison` (NaN or +Inf)"""
    T, cols = host.shape
    c = CHUNK[dt]
    buf = torch.full((T + 3, round_up(cols, c) + c), poison, dtype=dt, device=DEV)
    v = buf[:T, :cols]
    v.copy_(host.to(DEV))
    assert v.data_ptr() % 16 == 0 and v.stride(0) % c == 0
    return v


class Batch:
    """one list of products: operands, guarded outputs and the fp64 reference.
    shapes: [(n_out, n_in, tokens)]; placements, has_db: per product; kind: "int" | "normal"."""

    def __init__(self, dt, shapes, placements, has_db, poison, kind, seed):
        gen = torch.Generator().manual_seed(seed)
        self.dt, self.shapes, self.kind = dt, shapes, kind
        self.wa, self.ba = Arena(), Arena()
        self.hy, self.hx, self.w0, self.b0, self.wi, self.bi = [], [], [], [], [], []
        for (n_out, n_in, T), pl, b in zip(shapes, placements, has_db):
            self.hy.append(values(gen, kind, dt, T, n_out))
            self.hx.append(values(gen, kind, dt, T, n_in))
            self.w0.append(values(gen, kind, F32, n_out, n_in))
            self.b0.append(values(gen, kind, F32, 1, n_out) if b else None)
            self.wi.append(self.wa.matrix(n_out, n_in, pl))
            self.bi.append(self.ba.vector(n_out) if b else None)
            if kind == "int":
                assert 16 * T + 4 < 2 ** 24
        if not any(has_db):
            self.ba.vector(1)                                     # an arena needs a view
        self.wa.finish(), self.ba.finish()
        self.dy = [operand(h, dt, poison) for h in self.hy]
        self.x = [operand(h, dt, poison) for h in self.hx]
        self.dw = [self.wa.view(i) for i in self.wi]
        self.db = [None if i is None else self.ba.view(i)[0] for i in self.bi]
        for pl, w in zip(placements, self.dw):
            assert w.data_ptr() % 16 == (4 if pl == "odd" else 0)
        self.reset()
        self.wa0, self.ba0 = self.wa.buf.clone(), self.ba.buf.clone()

    def reset(self):
        for w, w0, b, b0 in zip(self.dw, self.w0, self.db, self.b0):
            w.copy_(w0.to(DEV))
            if b is not None:
                b.copy_(b0[0].to(DEV))

    def items(self):
        return list(zip(self.dy, self.x, self.dw, self.db))

    def launch(self, n_launches=1):
        with launches() as c:
            K.wgrad_group(self.items())
        other = FAMILY[F32 if self.dt == BF else BF]
        assert c[FAMILY[self.dt]] == n_launches and c[other] == 0, c

    def check(self, what, times=1):
        """every element of every dW and db after `times` launches on top of dW0 / db0; every guard element"""
        hw = self.wa.guards_intact(what + " dW")
        hb = self.ba.guards_intact(what + " db", only=[i for i in self.bi if i is not None])
        for k, (n_out, n_in, T) in enumerate(self.shapes):
            nk = (T + KTILE[self.dt] - 1) // KTILE[self.dt]
            y, x, w0 = self.hy[k].double(), self.hx[k].double(), self.w0[k].double()
            outs = [(self.wa.view(self.wi[k], hw), w0 + times * (y.t() @ x), w0, times * 4 * T * U32 * (y.abs().t() @ x.abs()), "dW")]
            if self.bi[k] is not None:
                b0 = self.b0[k].double()
                outs.append((self.ba.view(self.bi[k], hb), b0 + times * y.sum(0, keepdim=True), b0, times * 4 * T * U32 * y.abs().sum(0, keepdim=True), "db"))
            for out, ref, init, accb, name in outs:
                tag = "%s item %d %s (%d x %d, %d tokens)" % (what, k, name, n_out, n_in, T)
                if self.kind == "int":
                    assert_close(out, ref, torch.zeros_like(ref), tag)
                    assert np.array_equal(bits(out), bits(ref.float())), tag + ": not the reference's bits"
                else:
                    assert_close(out, ref, accb + times * (nk + 1) * U32 * (init.abs() + ref.abs()), tag)

    def run(self, what):
        self.launch()
        self.check(what)
        if self.kind == "int":                                    # a second run repeats the first bit for bit
            first = (self.wa.buf.clone(), self.ba.buf.clone())
            self.reset()
            K.wgrad_group(self.items())
            assert torch.equal(bits_dev(self.wa.buf), bits_dev(first[0])) and torch.equal(bits_dev(self.ba.buf), bits_dev(first[1])), what + ": rerun differs"


def bits_dev(t):
    return t.view(torch.int32)


def one(dt, n_out, n_in, T, placement, has_db, poison, kind, seed):
    return Batch(dt, [(n_out, n_in, T)], [placement], [has_db], poison, kind, seed)


# ------------------------------------------------------------------ the shape grids, each case a list of one
def grid(tokens, shapes, every_shape_at, every_tokens_at, all_placements_at):
    """(tokens, shape) pairs: every shape at two token counts, every token count at three shapes.  The shapes with interior tiles
    and the smallest ragged one take all three dW placements, the others rotate through them.  db is present in every other
    case; the padding is NaN in half of the cases and +Inf in the other half (independent of db)."""
    pairs = [(t, s) for s in shapes for t in every_shape_at]
    pairs += [(t, s) for s in every_tokens_at for t in tokens if (t, s) not in pairs]
    cases = []
    for i, (t, s) in enumerate(pairs):
        for pl in (PLACEMENTS if s in all_placements_at else (PLACEMENTS[i % 3],)):
            k = len(cases)
            cases.append(pytest.param(t, s, pl, k % 2 == 0, math.nan if (k // 2) % 2 == 0 else math.inf,
                                      id="t%d_%dx%d_%s_%s_%s" % (t, s[0], s[1], pl, "db" if k % 2 == 0 else "nodb", "nan" if (k // 2) % 2 == 0 else "inf")))
    return cases


# bf16: K-tiles of 64 tokens, a prologue that stages K-tiles 0 and 1, loop restages of t + 1 / t + 2 clamped at nk - 1: 1 to 3
# K-tiles, whole and ragged.  Outputs: 8-column chunks with the min(.., n_out8 - 8) clamp, 128-column half tiles, 64-row wave slabs, the
# 256 tile on both sides, interior tiles next to ragged ones.
BF_TOKENS = [1, 3, 4, 5, 63, 64, 65, 128, 129, 193]
BF_SHAPES = [(8, 8), (9, 15), (16, 24), (63, 65), (127, 129), (128, 128), (136, 264), (255, 257), (256, 256), (257, 255), (264, 520), (513, 8)]
BF_CASES = grid(BF_TOKENS, BF_SHAPES, (5, 129), ((9, 15), (257, 255), (264, 520)), ((256, 256), (264, 520), (9, 15)))
# f32: stages of 32 tokens (1 to 4 stages, whole and ragged), 4-column pieces, 64 x 64 wave tiles, the 128 tile on both sides
F32_TOKENS = [1, 7, 8, 9, 31, 32, 33, 64, 65, 97]
F32_SHAPES = [(1, 1), (3, 5), (4, 4), (5, 3), (63, 65), (64, 64), (65, 63), (127, 129), (128, 128), (129, 127), (131, 260), (257, 4)]
F32_CASES = grid(F32_TOKENS, F32_SHAPES, (7, 65), ((3, 5), (129, 127), (131, 260)), ((128, 128), (131, 260), (3, 5)))


def run_grid_case(dt, tokens, shape, placement, has_db, poison):
    seed = 1000 * tokens + 7 * shape[0] + shape[1]
    for kind in ("int", "normal"):
        one(dt, shape[0], shape[1], tokens, placement, has_db, poison, kind, seed).run("%s %s" % (FAMILY[dt], kind))


@pytest.mark.parametrize("tokens,shape,placement,has_db,poison", BF_CASES)
def test_bf16_one_product(tokens, shape, placement, has_db, poison):
    run_grid_case(BF, tokens, shape, placement, has_db, poison)


@pytest.mark.parametrize("tokens,shape,placement,has_db,poison", F32_CASES)
def test_f32_one_product(tokens, shape, placement, has_db, poison):
    run_grid_case(F32, tokens, shape, placement, has_db, poison)


# ------------------------------------------------------------------ the planners' list shapes (tests/wgrad_lists.py: integer-exact, nonzero dW0)
def named(dt, shapes, placement="dense", db=lambda k: False, seed=5, poison=math.nan):
    return Batch(dt, shapes, [placement] * len(shapes), [db(k) for k in range(len(shapes))], poison, "int", seed)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("tokens", [960, 961, 1087, 1600])
def test_bf16_one_264x264_whole_and_cut(tokens, placement):
    """2 x 2 tiles with ragged edges: whole at 960 tokens, cut in two from 961, in three at 1,600 (wgrad_lists.PLANS): the atomic
    epilogue with its row and column guards and the atomic db, with poisoned padding"""
    with set_option("reserve_cus", 0):
        named(BF, wgrad_lists.one_264x264(tokens), placement, db=lambda k: True, seed=tokens, poison=math.inf if tokens & 1 else math.nan).run("one_264x264 %d" % tokens)


def test_bf16_ctc_head_at_the_config_shape():
    """encoder.ctc_fc of the m preset at the ragged Cfg3 batch (tests/test_configs_gpu.py: 5,001 units x 512, 3 x 375 = 1,125 tokens,
    dense in the arena, with its bias): 5,001 rows are a multiple of no tile (137 past 19 x 256, 9 past 39 x 128), 18 K-tiles, the
    last a ragged one; element by element against fp64.  The block-wise parity criterion of the config tests gives this tensor's
    class a wider margin and rests that on this product being right.  This is the ragged case's token count alone: the same tensor
    at the 16 x 1500 route (6,000 tokens) is not run here."""
    for kind in ("int", "normal"):
        one(BF, 5001, 512, 1125, "dense", True, math.nan, kind, 5001).run("ctc head %s" % kind)


def test_bf16_db_comes_from_the_first_column_tile_only():
    """db of a product of several column tiles is summed by tile (.., 0) alone.  In a list of one the column tiles run side by side
    and their plain read-modify-writes of db would collide into the right value; here tiles (0, 1) and (0, 2) of the last product
    run in the second round, after tile (0, 0) (wgrad_lists.second_round), so a sum added twice stays added"""
    with set_option("reserve_cus", 0):
        named(BF, wgrad_lists.second_round(), "odd", db=lambda k: True, seed=7).run("second_round")


def test_bf16_whole_round_is_placement_independent():
    """256 one-tile products on 256 workgroups: no cuts, no atomics (wgrad_lists.PLANS "whole_round 128").  The element-wise epilogue
    (dW one float in) and the 16-byte one (dense dW) do the same f32 add: the same bits, and the reference's"""
    with set_option("reserve_cus", 0):
        a = named(BF, wgrad_lists.whole_round(128), "dense")
        b = named(BF, wgrad_lists.whole_round(128), "odd")
        a.run("whole_round dense")
        b.run("whole_round odd")
        for k, (wa, wb) in enumerate(zip(a.dw, b.dw)):
            assert torch.equal(bits_dev(wa.contiguous()), bits_dev(wb.contiguous())), k


def test_bf16_whole_round_on_240_workgroups_is_cut():
    """the same 256 products at 2,048 tokens with 16 CUs reserved: a tail round of 16 tiles cut in four (PLANS "whole_round 2048 G240")"""
    with set_option("reserve_cus", 16):
        named(BF, wgrad_lists.whole_round(2048), "odd").run("whole_round 2048 reserve 16")


def test_bf16_tail_round():
    """260 products: a whole round and a tail round of 4 tiles cut in four, atomic (PLANS "tail_round")"""
    with set_option("reserve_cus", 0):
        named(BF, wgrad_lists.tail_round(), "padded").run("tail_round")


@pytest.mark.parametrize("reserve", [0, 16])
def test_bf16_fill_layout(reserve):
    """two long reductions poured over eight slots each next to 600 short ones (PLANS "fill", "fill G240"); db on every second product"""
    with set_option("reserve_cus", reserve):
        named(BF, wgrad_lists.fill(), "dense", db=lambda k: k % 2 == 0).run("fill reserve %d" % reserve)


@pytest.mark.parametrize("tokens", [480, 512])
def test_f32_tail_round_cut(tokens):
    """528 products on the f32 planner's 512 workgroups: whole at 15 stages, the tail round's 16 tiles cut in eight at 16 stages
    (PLANS "cut_f32 480", "cut_f32 512"); db on every third product"""
    named(F32, wgrad_lists.cut_f32(tokens), "odd", db=lambda k: k % 3 == 0).run("cut_f32 %d" % tokens)


# ------------------------------------------------------------------ the list cache of s2t_wgrad_group (4 slots, keyed on the problem array's bytes, per stream)
def test_bf16_cached_list_follows_new_operand_contents():
    """the second launch of a byte-identical list takes the cached table: it must read the operands as they are NOW"""
    b = Batch(BF, [(264, 264, 128), (16, 16, 64)], ["dense", "odd"], [True, False], math.nan, "int", 11)
    b.run("first contents")
    gen = torch.Generator().manual_seed(12)
    for k, (n_out, n_in, T) in enumerate(b.shapes):
        b.hy[k], b.hx[k] = values(gen, "int", BF, T, n_out), values(gen, "int", BF, T, n_in)
        b.dy[k].copy_(b.hy[k].to(DEV)), b.x[k].copy_(b.hx[k].to(DEV))
    b.reset()
    b.run("rewritten contents")


def test_bf16_six_lists_round_robin_evict_and_regrow():
    """six distinct lists twice round-robin through four slots: every launch of the second pass finds its list evicted; the list of
    1,400 products needs a table above a slot's first 64 KiB, so the slot it lands in is freed and regrown"""
    lists = [[(264, 264, 128)], [(16, 16, 64)] * 3, [(16, 16, 64)] * 1400, [(16, 24, 100), (264, 16, 64)], [(24, 16, 65)] * 5, [(8, 8, 1), (9, 15, 128)]]
    batches = [Batch(BF, s, ["dense" if k % 2 else "odd" for k in range(len(s))], [k % 2 == 0 for k in range(len(s))], math.inf, "int", 20 + i)
               for i, s in enumerate(lists)]
    for rep in range(2):
        with launches() as c:
            for b in batches:
                b.reset()
                K.wgrad_group(b.items())
        assert c["wgrad_group"] == len(batches), c
        for i, b in enumerate(batches):
            b.check("pass %d list %d" % (rep, i))


def test_bf16_lists_that_differ_in_one_field():
    """the key is every byte of the problem array: with all operand pointers equal, a list that differs from a cached one only in
    db, only in tokens or only in ldw is another list"""
    T, n = 128, 264
    gen = torch.Generator().manual_seed(31)
    hy, hx = values(gen, "int", BF, T, n), values(gen, "int", BF, T, n)
    w0, b0 = values(gen, "int", F32, n, n), values(gen, "int", F32, n)
    dy, x = operand(hy, BF, math.nan), operand(hx, BF, math.nan)
    wa = Arena()
    dense = wa.at(round_up(n, 4) + 4, n, n, n)
    wide = wa.at(round_up(n, 4) + 4, n, n, n + 4)                  # the same base pointer, another ldw
    wa.finish()
    ba = Arena()
    bi = ba.vector(n)
    ba.finish()
    assert wa.view(dense).data_ptr() == wa.view(wide).data_ptr()

    def run(what, tokens, view, with_db):
        wa.buf.fill_(GUARD), ba.buf.fill_(GUARD)
        dw, db = wa.view(view), ba.view(bi)[0]
        dw.copy_(w0.to(DEV)), db.copy_(b0.to(DEV))
        with launches() as c:
            K.wgrad_group([(dy[:tokens], x[:tokens], dw, db if with_db else None)])
        assert c["wgrad_group"] == 1, c
        y64, x64 = hy[:tokens].double(), hx[:tokens].double()
        hw, hb = wa.guards_intact(what, only=[view]), ba.guards_intact(what)
        ref = w0.double() + y64.t() @ x64
        assert_close(wa.view(view, hw), ref, torch.zeros_like(ref), what + " dW")
        refb = b0.double() + (y64.sum(0) if with_db else 0.0)
        assert_close(ba.view(bi, hb)[0], refb, torch.zeros_like(refb), what + " db")
    for rep in range(2):                                           # second pass: every variant is now in a slot of its own
        run("base", T, dense, True)
        run("no db", T, dense, False)
        run("base again", T, dense, True)
        run("64 of 128 tokens", 64, dense, True)
        run("base after tokens", T, dense, True)
        run("ldw + 4", T, wide, True)
        run("base after ldw", T, dense, True)


def test_bf16_same_list_on_a_second_stream():
    """a cached table serves only the stream it was uploaded on: the same list on a second stream uploads its own.  The second
    stream waits for the first (both add to the same dW); the result is dW0 plus twice the product"""
    b = Batch(BF, [(264, 264, 128), (16, 16, 64)], ["padded", "odd"], [True, True], math.inf, "int", 41)
    s2 = torch.cuda.Stream()
    torch.cuda.synchronize()
    K.wgrad_group(b.items())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        K.wgrad_group(b.items())
    s2.synchronize()
    torch.cuda.synchronize()
    b.check("two streams", times=2)
    b.reset()
    b.run("first stream again")


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_two_lists_back_to_back(dt):
    """two different lists on one stream with nothing between them: the f32 table lives in ONE per-stream scratch buffer that the
    second upload overwrites, the bf16 table in a slot the second upload may reuse -- stream order must keep the first launch's table
    intact until it has run"""
    a = Batch(dt, [(264, 264, 128), (16, 16, 64)], ["dense", "odd"], [True, False], math.nan, "int", 51)
    b = Batch(dt, [(24, 16, 65)] * 40 + [(136, 264, 33)], ["odd"] * 41, [k % 2 == 1 for k in range(41)], math.nan, "int", 52)
    for rep in range(2):
        a.reset(), b.reset()
        with launches() as c:
            K.wgrad_group(a.items())
            K.wgrad_group(b.items())
        assert c[FAMILY[dt]] == 2, c
        a.check("first list, pass %d" % rep)
        b.check("second list, pass %d" % rep)


# ------------------------------------------------------------------ refusals: S2T_EINVAL, no launch, no output touched
def _set(field, fn):
    def change(p):
        setattr(p, field, fn(getattr(p, field)))
    change.__name__ = field
    return change


REFUSED = {
    BF: [("n_out 7", _set("n_out", lambda v: 7)), ("n_in 7", _set("n_in", lambda v: 7)), ("n_out 0", _set("n_out", lambda v: 0)),
         ("ldy % 8", _set("ldy", lambda v: v - 4)), ("ldx % 8", _set("ldx", lambda v: v - 4)),
         ("dY + 2 bytes", _set("dY", lambda v: v + 2)), ("X + 2 bytes", _set("X", lambda v: v + 2)),
         ("ldy < n_out", _set("ldy", lambda v: 8)), ("ldx < n_in", _set("ldx", lambda v: 8)),
         ("tokens 0", _set("tokens", lambda v: 0)), ("dY null", _set("dY", lambda v: None))],
    F32: [("n_out 0", _set("n_out", lambda v: 0)), ("n_in 0", _set("n_in", lambda v: 0)),
          ("ldy % 4", _set("ldy", lambda v: v - 2)), ("ldx % 4", _set("ldx", lambda v: v - 2)),
          ("dY + 4 bytes", _set("dY", lambda v: v + 4)), ("X + 4 bytes", _set("X", lambda v: v + 4)),
          ("ldy < n_out", _set("ldy", lambda v: 12)), ("ldx < n_in", _set("ldx", lambda v: 12)),
          ("tokens 0", _set("tokens", lambda v: 0)), ("dY null", _set("dY", lambda v: None))],
}


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
def test_refusals_launch_nothing_and_touch_nothing(dt):
    """one bad problem between two good ones: S2T_EINVAL, no launch, and the dW / db of ALL three keep their bits (the checks run
    before anything is uploaded).  Every bad argument is one with which a launch would still have stayed inside the buffers: smaller
    sizes, smaller strides, a base a few bytes in (three spare rows follow each operand).  n = 0 is S2T_OK, a negative n S2T_EINVAL"""
    fn = K._lib().s2t_wgrad_group if dt == BF else K._lib().s2t_wgrad_group_f32
    b = Batch(dt, [(16, 24, 64), (16, 16, 64), (24, 16, 64)], ["dense", "odd", "padded"], [True, True, True], math.nan, "int", 61)

    def problems():
        arr = (L.WgradProblem * 3)()
        for p, (dy, x, dw, db) in zip(arr, b.items()):
            p.dY, p.X, p.dW, p.db = dy.data_ptr(), x.data_ptr(), dw.data_ptr(), db.data_ptr()
            p.n_out, p.n_in, p.tokens, p.ldy, p.ldx, p.ldw = dy.shape[1], x.shape[1], dy.shape[0], dy.stride(0), x.stride(0), dw.stride(0)
        return arr
    for what, change in REFUSED[dt]:
        arr = problems()
        change(arr[1])
        with launches() as c:
            rc = fn(3, ctypes.addressof(arr), L.stream())
        assert rc == EINVAL, (what, rc)
        assert c[FAMILY[dt]] == 0, (what, c)
        assert torch.equal(bits_dev(b.wa.buf), bits_dev(b.wa0)) and torch.equal(bits_dev(b.ba.buf), bits_dev(b.ba0)), what + ": an output changed"
    arr = problems()
    with launches() as c:
        assert fn(0, ctypes.addressof(arr), L.stream()) == 0 and fn(0, 0, L.stream()) == 0
        assert fn(-1, ctypes.addressof(arr), L.stream()) == EINVAL and fn(3, 0, L.stream()) == EINVAL
    assert c[FAMILY[dt]] == 0, c
    assert torch.equal(bits_dev(b.wa.buf), bits_dev(b.wa0)) and torch.equal(bits_dev(b.ba.buf), bits_dev(b.ba0))
    with launches() as c:                                          # and the list as it stands is taken
        assert fn(3, ctypes.addressof(arr), L.stream()) == 0
    assert c[FAMILY[dt]] == 1, c
    b.check("the unchanged list")
