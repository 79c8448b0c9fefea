"""The device-resident beam search (csrc/decode.hip through fbk_fairseq_st_amd.decode.BeamDecodeSession) step by step against float64.

Every case drives one session the way tools/decode_debug.py does -- s2t_decode_begin, then one s2t_decode_step at a time, synchronised
-- and after every step checks, each conditioned on the device's own history (tests/decode_ref.py):
  1. the logits (and the final LayerNorm output `xn`, and this step's K/V cache rows of every layer) against a float64 decoder step
     that starts from the device's step input x0 and its cached K/V rows along the ancestry rebuilt from `par_hist`, rounded where
     the kernels round, within measured allowances (decode_ref docstring); the step input x0 against embed_scale E[token] +
     position, within its f32 rounding;
  2. every row's 2 beam candidates against dec_row_kernel's arithmetic in float64 on the device's f32 logits;
  3. the sentence bookkeeping (tok_hist, par_hist, cum_hist, anc, blacklist, nfin, fin_*, steps, finished) bit for bit against the
     restated dec_sent_kernel fed the device's candidates of that step.
The weights come from oracle/s2t_ref.make_weights; the encoder output is a random [Ts, B, D] tensor handed to the session (its
encoder-side K/V product is computed here in float64 and rounded to the compute dtype, so the reference reads the same values).

Each case names the branch of decode.hip it is there for.  CH0 = positions whose cached K/V the self-attention kernel loads up front:
bf16 128 (beam <= 5), 64 (beam 6-8), 32 (beam > 8); f32 64, 32, 16.  The long cases set min_len = max_len, so every hypothesis runs to
max_len and takes the forced-EOS step there.  The worst error / allowance ratio of every check and dtype is printed at the end (-s).

One-line, value-only mutations of decode.hip, each built separately, and the first case and check that fail on them (MI355X):
  1. score chunk loop `pos0 += 2 * CH0`                  bf16-D256-b2-ancestors_300, step 257, xn
  2. P.V chunk loads `min(.., t - 2)`                    f32-D256-b5-CH0_64, step 65, xn
  3. bf16 pair path `pb = pa + NSLOT + 1`                bf16-D256-b5-CH0_128, step 32, xn
  4. ancestor rewrite of dec_sent_kernel stops at 256    bf16-D256-b2-ancestors_300, step 260, anc
  5. 64 < cnt <= 120 branch without column tie-break     f32-D256-b5-ties100, step 0, candidates (a lower tied column passed over)
  6. cross-attention key mask `pos <= klen`              f32-D256-b5-CH0_64, step 0, xn
  7. min-len rule `t <= min_len`                         f32-D256-b16-B8, step 1, candidates (EOS missing from the set)
  8. unk penalty added                                   f32-D256-b4-rules-gelu, step 1, candidate values
  9. prologue leaves out the last share                  f32-D256-b5-CH0_64, step 0, xn
The search tests that predate this file (test_model_gpu.py beam search, test_configs_gpu.py device search) pass with 1 and 2.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from oracle import s2t_ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
PAD, EOS, UNK, BOS = 1, 2, 3, 2
TIE0 = 60
ENOTSUP = -95
BF, F32 = torch.bfloat16, torch.float32
WORST = {}


def _mods():
    import decode_ref
    from fbk_fairseq_st_amd import decode, engine, lib
    return decode_ref, decode, engine, lib


def _note(check, dtype, ratio):
    k = (check, "bf16" if dtype == BF else "f32")
    WORST[k] = max(WORST.get(k, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (check, dt), r in sorted(WORST.items()):
        print("decode worst error/allowance: %-7s %-5s %.3g" % (check, dt, r))


class DecEngine:
    """What BeamDecodeSession reads of an S2TEngine, over s2t_ref.make_weights tensors: compute-dtype weights (W), f32 parameters (P),
    the sinusoid table and the encoder-side K/V product (float64, rounded to the compute dtype; recorded for the reference)."""

    def __init__(self, D, ffn, layers, V, dtype, seed, act="relu", eos_scale=1.0, unk_scale=1.0, tie=0):
        cfg = s2t_ref.default_cfg(D=D, heads=D // 64, ffn=ffn, enc_layers=0, dec_layers=layers, act=act)
        W = s2t_ref.make_weights({k: v for k, v in s2t_ref.param_shapes(cfg, 8, V).items() if k.startswith("decoder.")}, seed)
        wo = W["decoder.output_projection.weight"]
        wo[EOS] *= eos_scale
        wo[UNK] *= unk_scale
        if tie:
            # `tie` identical columns from TIE0 on, every row's best: the final LayerNorm's bias gets a component u of norm 4 and the
            # tied rows are 4 u / |u|, so their logit is about 16 where the others stay within a few units.  With TIE0 = 60 the list
            # of dec_row_kernel holds wave 1's 64 columns 64..127 and wave 0's 60..63 (and more): whenever wave 0 appends last, a lane's
            # second entry (60..63) has a lower column than its first, which only the column tie-break orders right.
            u = torch.from_numpy(np.random.RandomState(seed + 1).randn(D).astype(np.float32))
            u *= 4.0 / float(u.norm())
            W["decoder.layer_norm.bias"] += u
            wo[TIE0:TIE0 + tie] = u
        for l in range(layers):
            p = "decoder.layers.%d." % l
            for kind, parts, fused in (("self_attn.", ("q", "k", "v"), "qkv"), ("encoder_attn.", ("k", "v"), "kv")):
                for f in ("weight", "bias"):
                    W[p + kind + fused + "." + f] = torch.cat([W[p + kind + c + "_proj." + f] for c in parts], 0)
        self.cfg, self.dtype, self.dev = cfg, dtype, torch.device(DEV)
        self.hp = types.SimpleNamespace(D=D, heads=D // 64, ffn=ffn, dec_layers=layers, act=act, ln_eps=1e-5, no_scale_embedding=False)
        self.f32 = {k: v.to(DEV) for k, v in W.items()}
        self.w = {k: v.to(DEV, dtype) for k, v in W.items() if v.dim() == 2}
        self.kv = []
        self._table = None

    def W(self, n):
        return self.w[n]

    def P(self, n):
        return self.f32[n]

    def out_proj(self, pfx):
        return pfx + "output_projection"

    def table(self, n, pad):
        if self._table is None or self._table.shape[0] < n:
            self._table = _mods()[2].sinusoid_table(max(n, 1024), self.hp.D, pad, self.dev)
        return self._table

    def linear(self, x2d, name):
        y = (x2d.double() @ self.w[name + ".weight"].double().t() + self.f32[name + ".bias"].double()).to(self.dtype)
        self.kv.append(y)
        return y

    def ref_weights(self):
        """float64 copies: matrices as the compute dtype holds them, LayerNorm parameters and biases as f32"""
        return {k: (self.w[k] if k in self.w else self.f32[k]).double() for k in self.f32}


def _session(c, monkeypatch):
    _, DEC, _, _ = _mods()
    torch.manual_seed(c.get("seed", 0))
    eng = DecEngine(c["D"], c.get("ffn", 2 * c["D"]), c.get("layers", 1), c["V"], c["dtype"], c.get("seed", 0), c.get("act", "relu"),
                    c.get("eos_scale", 1.0), c.get("unk_scale", 1.0), c.get("tie", 0))
    B, beam, Ts = c["B"], c["beam"], c.get("Ts", 100)
    if c.get("hs"):
        monkeypatch.setenv("S2T_DECODE_HS", str(c["hs"]))
    enc = torch.randn(Ts, B, c["D"], device=DEV)
    klen = torch.tensor(c["klen"], dtype=torch.int32, device=DEV) if c.get("klen") else None
    init = torch.randn(B * beam, device=DEV) * 0.5 - 1.0 if c.get("init") else None
    ses = DEC.BeamDecodeSession(eng, "decoder.", enc, klen, beam, c["max_len"], c.get("min_len", 1), PAD, UNK, EOS, c["V"],
                                c.get("unk_penalty", 0.0), c.get("temperature", 1.0), init_scores=init, step0_all_slots=c.get("init", False))
    assert ses.ok, "the session refused a shape the case is meant to run"
    if c.get("hs"):
        assert ses.desc.ffn // ses.desc.ffn_slices == c["hs"], "S2T_DECODE_HS was not taken"
    return eng, ses, init


def _host(ses, name, shape=None):
    v = (ses.view_i(name) if name in ses.ioff else ses.view_f(name)).cpu().numpy()
    return v.reshape(shape) if shape is not None else v


def _check_close(out, ref, bound, check, dtype, what):
    """|out - ref| <= bound element by element; records the worst ratio; on failure names the worst element"""
    o = out.double()
    b = bound
    err = (o - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    worst = float(ratio.max())
    _note(check, dtype, worst)
    if not worst <= 1.0:
        i = int(ratio.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
        raise AssertionError("%s: %d elements out of bound; worst at %s: out %.9g ref %.9g bound %.3g (%.3gx)" % (
            what, int((ratio > 1).sum()), idx, float(o[idx]), float(ref[idx]), float(b[idx]), worst))


def run_search(c, monkeypatch):
    """the whole search, one checked step at a time; returns the session and how often a row's best candidate was a tied column"""
    R, DEC, E, L = _mods()
    eng, ses, init = _session(c, monkeypatch)
    dtype, B, beam, V, max_len = c["dtype"], c["B"], c["beam"], c["V"], c["max_len"]
    N, K2, M2, Ts = B * beam, 2 * beam, max_len + 2, c.get("Ts", 100)
    d = ses.desc
    lib, st = L.load(), L.stream()
    Wr = eng.ref_weights()
    ref = R.StepRef(Wr, eng.cfg, dtype, [k.view(Ts, B, -1) for k in eng.kv], c.get("klen"), beam, d.ffn_slices, float(np.float32(1e-5)))
    caches = [ses.bufs["cache%d" % l] for l in range(eng.cfg["dec_layers"])]
    pos_table = eng.table(PAD + 3 + max_len, PAD)
    # the scalars as the case states them, rounded to the f32 the C ABI carries (not read back from the session's descriptor)
    f32 = lambda v: float(np.float32(v))
    embed_scale, inv_temp = f32(c["D"] ** 0.5), f32(1.0 / c.get("temperature", 1.0))
    unk_pen, min_len, step0_all = f32(c.get("unk_penalty", 0.0)), c.get("min_len", 1), bool(c.get("init", False))
    L.check(lib.s2t_decode_begin(ses.addr, BOS, st), "s2t_decode_begin")
    host = R.new_state(B, beam, max_len, BOS)
    anc = torch.zeros((N, max_len + 1), dtype=torch.long, device=DEV)
    tokens = torch.full((N,), BOS, dtype=torch.long, device=DEV)
    fin_seen, tied_best = {}, 0
    for t in range(max_len + 1):
        what = "%s step %d" % (c["id"], t)
        x0 = ses.bufs["x0"].clone()
        xr, xb = R.next_input(Wr, PAD, tokens, PAD + 1 + t, pos_table, embed_scale)
        _check_close(x0, xr, R.SAFETY * xb, "x0", dtype, what + ": x0")
        L.check(lib.s2t_decode_step(ses.addr, st), "s2t_decode_step")
        torch.cuda.synchronize()
        # 1. the decoder step
        r = ref.step(x0, t, anc, caches)
        for l, (kv, ekv) in enumerate(r["kv"]):
            _check_close(caches[l][t], kv, ekv, "kv", dtype, what + ": K/V cache row of layer %d" % l)
        _check_close(ses.bufs["xn"], *r["xn"], "xn", dtype, what + ": xn")
        _check_close(ses.bufs["logits"], *r["logits"], "logits", dtype, what + ": logits")
        # 2. the rows' candidates, on the device's own logits
        base = torch.from_numpy(host["cum_hist"][t].astype(np.float64)).to(DEV) if t > 0 else \
            (init.double() if init is not None else torch.zeros(N, dtype=torch.float64, device=DEV))
        rv, rb = R.row_reference(ses.bufs["logits"], t, beam, PAD, UNK, EOS, max_len, min_len, inv_temp, unk_pen, base, step0_all)
        cv, ci = ses.view_f("cand_val").view(N, K2), ses.view_i("cand_idx").view(N, K2)
        _note("rows", dtype, R.check_row_candidates(cv, ci, rv, rb, what + ": candidates"))
        if c.get("tie"):
            tied_best += int(((ci[:, 0] == TIE0) & (ci[:, 1] == TIE0 + 1)).sum())
        # 3. the bookkeeping, bit for bit
        R.sent_step(host, cv.cpu().numpy(), ci.cpu().numpy(), beam, V, EOS, max_len, step0_all)
        for k in ("blacklist", "nfin", "finished", "steps"):
            v = _host(ses, k)
            assert np.array_equal(v, host[k]), "%s: %s %s != %s" % (what, k, v.tolist(), host[k].tolist())
        th, ph, ch = _host(ses, "tok_hist", (M2, N)), _host(ses, "par_hist", (M2, N)), _host(ses, "cum_hist", (M2, N))
        assert np.array_equal(th[:t + 2], host["tok_hist"][:t + 2]), what + ": tok_hist"
        assert np.array_equal(ph[1:t + 2], host["par_hist"][1:t + 2]), what + ": par_hist"
        assert np.array_equal(ch[1:t + 2].view(np.int32), host["cum_hist"][1:t + 2].view(np.int32)), what + ": cum_hist"
        na = t + 1 if t < max_len else t
        assert np.array_equal(_host(ses, "anc", (N, max_len + 1))[:, :na], host["anc"][:, :na]), what + ": anc"
        fs, fr, fsc = _host(ses, "fin_step", (B, beam)), _host(ses, "fin_row", (B, beam)), _host(ses, "fin_score", (B, beam))
        for s in range(B):
            k = int(host["nfin"][s])
            got = (fs[s, :k].tolist(), fr[s, :k].tolist(), fsc[s, :k].view(np.int32).tolist())
            assert got == (host["fin_step"][s, :k].tolist(), host["fin_row"][s, :k].tolist(),
                           host["fin_score"][s, :k].view(np.int32).tolist()), "%s: finalisation records of sentence %d" % (what, s)
            if host["finished"][s]:
                assert fin_seen.setdefault(s, got) == got, "%s: sentence %d changed its records after it finished" % (what, s)
        par = torch.from_numpy(host["par_hist"][t + 1].astype(np.int64)).to(DEV)
        tokens = torch.from_numpy(host["tok_hist"][t + 1].astype(np.int64)).to(DEV)
        if t < max_len:
            nxt = anc.clone()
            nxt[:, :t] = anc[par, :t]
            nxt[:, t] = par
            anc = nxt
    return ses, tied_best


def C(id_, dtype, D, beam, B, max_len, V=96, **kw):
    c = dict(id=id_, dtype=dtype, D=D, beam=beam, B=B, max_len=max_len, V=V)
    c.update(kw)
    return pytest.param(c, id=id_)


CASES = [
    # self-attention chunks past CH0 (min_len = max_len: every step runs, the last one forced to EOS)
    C("f32-D256-b5-CH0_64", F32, 256, 5, 2, 66, min_len=66),
    C("bf16-D256-b5-CH0_128", BF, 256, 5, 2, 131, min_len=131),
    C("bf16-D512-b8-CH0_64", BF, 512, 8, 2, 67, min_len=67),
    C("f32-D512-b6-CH0_32", F32, 512, 6, 2, 35, min_len=35),
    C("bf16-D256-b12-RT16-CH0_32", BF, 256, 12, 2, 34, min_len=34),
    C("f32-D256-b9-RT16-CH0_16", F32, 256, 9, 1, 18, min_len=18),
    C("bf16-D256-b2-ancestors_300", BF, 256, 2, 1, 300, min_len=300),
    C("f32-D256-b2-max_len_1023", F32, 256, 2, 1, 1023, min_len=1023),
    # D and the weight forms: registers (bf16, D <= 512) against run time (bf16 D 1024, f32); two layers; beam 1; B x beam = 128
    C("bf16-D1024-b4-2layers", BF, 1024, 4, 2, 10, layers=2),
    C("f32-D1024-b2", F32, 1024, 2, 1, 8),
    C("bf16-D512-b1-B3-2layers", BF, 512, 1, 3, 10, layers=2),
    C("f32-D256-b16-B8", F32, 256, 16, 8, 6),
    C("bf16-D256-b16-B8", BF, 256, 16, 8, 6),
    # EOS-rich searches with ragged encoder lengths (klen 1 included): finalisation at different steps, black-listing
    C("bf16-D256-b4-eos_rich", BF, 256, 4, 4, 24, eos_scale=4.0, klen=[100, 37, 1, 64]),
    C("f32-D512-b5-eos_rich", F32, 512, 5, 3, 24, eos_scale=5.0, klen=[80, 100, 1]),
    # encoder side: Tsp 256 in registers, 384 / 768 streamed
    C("bf16-D256-b5-Tsp256", BF, 256, 5, 2, 8, Ts=200, klen=[200, 150]),
    C("f32-D256-b5-Tsp256", F32, 256, 5, 2, 8, Ts=256),
    C("f32-D256-b4-Ts325", F32, 256, 4, 2, 8, Ts=325, klen=[325, 17]),
    C("bf16-D512-b5-Ts700", BF, 512, 5, 2, 8, Ts=700, klen=[700, 1]),
    # feed-forward slice widths
    C("bf16-D256-hs64", BF, 256, 5, 2, 6, ffn=512, hs=64),
    C("bf16-D256-hs128", BF, 256, 5, 2, 6, ffn=512, hs=128),
    C("bf16-D512-hs256", BF, 512, 4, 2, 6, ffn=1024, hs=256),
    C("f32-D256-hs256", F32, 256, 3, 2, 6, ffn=512, hs=256),
    # the row kernel: V at its minimum, on both sides of VPT switches, at its maximum; tied columns
    C("f32-D256-b4-V9", F32, 256, 4, 2, 8, V=9),
    C("bf16-D256-b5-V2048", BF, 256, 5, 2, 5, V=2048),
    C("bf16-D256-b5-V2049", BF, 256, 5, 2, 5, V=2049),
    C("f32-D256-b2-V8192", F32, 256, 2, 2, 5, V=8192),
    C("f32-D256-b2-V8193", F32, 256, 2, 2, 5, V=8193),
    C("bf16-D256-b4-V32768", BF, 256, 4, 1, 4, V=32768),
    C("f32-D256-b5-ties100", F32, 256, 5, 2, 6, V=512, tie=100),
    C("bf16-D256-b5-ties200", BF, 256, 5, 2, 6, V=512, tie=200),
    # the rules: unk penalty, temperature, min_len, step0_all_slots with init scores, GELU
    C("f32-D256-b4-rules-gelu", F32, 256, 4, 2, 12, min_len=5, unk_penalty=0.7, temperature=1.3, init=True, act="gelu",
      eos_scale=3.0, unk_scale=3.0),
    C("bf16-D512-b5-rules-gelu", BF, 512, 5, 2, 12, min_len=3, unk_penalty=-0.5, temperature=0.8, init=True, act="gelu",
      eos_scale=3.0, unk_scale=3.0),
]


@pytest.mark.parametrize("c", CASES)
def test_device_search_step_by_step(c, monkeypatch):
    _, tied_best = run_search(c, monkeypatch)
    if c.get("tie"):
        # every live row of steps 0 .. max_len - 1 (step 0: one per sentence; step max_len: EOS only)
        assert tied_best == c["B"] + c["B"] * c["beam"] * (c["max_len"] - 1), "the tied columns were not every row's best"


def _records(ses):
    """what a search leaves for the host: the hypotheses walk_records rebuilds, and the flags"""
    hyps = ses.hypotheses(True, 1.0)
    flat = [(b, h["tokens"].tolist(), h["positional_scores"].tolist(), h["_score"], h["origin"]) for b, hs in enumerate(hyps) for h in hs]
    return flat, _host(ses, "nfin").tolist(), _host(ses, "finished").tolist()


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_graph_replay_equals_step_launches(dtype, monkeypatch):
    """run(graph=True) (8 steps per replayed hipGraph) leaves the records of run(graph=False) bit for bit; replaying more graphs
    once every sentence has finished changes none of them"""
    _, DEC, _, L = _mods()
    c = dict(id="graph", dtype=dtype, D=256, beam=5, B=3, max_len=40, V=96, eos_scale=4.0, klen=[100, 9, 1])
    out = []
    for graph in (False, True):
        _, ses, _ = _session(c, monkeypatch)
        steps = ses.run(BOS, graph=graph)
        torch.cuda.synchronize()
        out.append((steps, _records(ses)))
    assert out[0] == out[1]
    assert all(out[1][1][2]), "every sentence finishes by max_len"
    lib = L.load()
    ex = ctypes.c_void_p(0)
    L.check(lib.s2t_decode_graph_create(ses.addr, DEC.POLL_STEPS, ctypes.addressof(ex)), "s2t_decode_graph_create")
    try:
        for _ in range(2):
            L.check(lib.s2t_decode_graph_launch(ex.value, L.stream()), "s2t_decode_graph_launch")
        torch.cuda.synchronize()
    finally:
        lib.s2t_decode_graph_destroy(ex.value)
    assert _records(ses) == out[1][1]


# ------------------------------------------------------------------ layout helpers
def _frag(dtype):
    per = 8 if dtype == BF else 4
    return per, 4 * per, (torch.int16 if dtype == BF else torch.int32)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_pack_weight_layout(dtype):
    """s2t_decode_pack_weight with N not a multiple of 16 and a row stride past K: fragment-major [ceil(N/16)][K/KS][64][PER], lane l of
    (tile, step) = W[16 tile + (l & 15)][KS step + PER (l >> 4) ..], rows past N zero (include/s2t_hip.h)"""
    L = _mods()[3]
    lib = L.load()
    N, K, ldw = 37, 128, 160
    PER, KS, it = _frag(dtype)
    Wfull = torch.randn(N, ldw).to(dtype)
    Wd = Wfull.to(DEV)
    tiles = (N + 15) // 16
    Wp = torch.full((tiles * 16, K), 7.0, dtype=dtype, device=DEV)
    L.check(lib.s2t_decode_pack_weight(L.dt(Wd), Wd.data_ptr(), ldw, N, K, Wp.data_ptr(), L.stream()), "s2t_decode_pack_weight")
    torch.cuda.synchronize()
    Wz = torch.zeros(tiles * 16, K, dtype=dtype)
    Wz[:N] = Wfull[:, :K]
    exp = Wz.view(tiles, 16, K // KS, 4, PER).permute(0, 2, 3, 1, 4).reshape(-1)          # [tile][step][l >> 4][l & 15][j]
    assert torch.equal(Wp.cpu().reshape(-1).view(it), exp.view(it))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_prepare_enc_layout(dtype):
    """s2t_decode_prepare_enc with Ts < Tsp: keys [B][H][Tsp/16][64/KS][64][PER] (lane l: K[16 pt + (l & 15)][KS step + PER (l >> 4) ..]),
    values transposed [B][H][4][Tsp/KS][64][PER] (lane l: V[KS step + PER (l >> 4) ..][16 ct + (l & 15)]), zero beyond Ts"""
    L = _mods()[3]
    lib = L.load()
    Ts, Tsp, B, D = 100, 128, 2, 256
    H = D // 64
    PER, KS, it = _frag(dtype)
    kv = torch.randn(Ts, B, 2 * D).to(dtype)
    kvd = kv.to(DEV)
    kp = torch.full((B, H, Tsp, 64), 7.0, dtype=dtype, device=DEV)
    vp = torch.full((B, H, 64, Tsp), 7.0, dtype=dtype, device=DEV)
    L.check(lib.s2t_decode_prepare_enc(L.dt(kvd), kvd.data_ptr(), kp.data_ptr(), vp.data_ptr(), Ts, Tsp, B, D, H, L.stream()),
            "s2t_decode_prepare_enc")
    torch.cuda.synchronize()
    Kf = torch.zeros(B, H, Tsp, 64, dtype=dtype)
    Kf[:, :, :Ts] = kv[:, :, :D].reshape(Ts, B, H, 64).permute(1, 2, 0, 3)
    Vf = torch.zeros(B, H, Tsp, 64, dtype=dtype)
    Vf[:, :, :Ts] = kv[:, :, D:].reshape(Ts, B, H, 64).permute(1, 2, 0, 3)
    ek = Kf.view(B, H, Tsp // 16, 16, 64 // KS, 4, PER).permute(0, 1, 2, 4, 5, 3, 6).reshape(-1)
    ev = Vf.view(B, H, Tsp // KS, 4, PER, 4, 16).permute(0, 1, 5, 2, 3, 6, 4).reshape(-1)
    assert torch.equal(kp.cpu().reshape(-1).view(it), ek.view(it))
    assert torch.equal(vp.cpu().reshape(-1).view(it), ev.view(it))


# ------------------------------------------------------------------ refusals
def test_refused_shapes(monkeypatch):
    """s2t_decode_lds_bytes returns 0 and s2t_decode_step S2T_ENOTSUP (before it launches anything) outside the limits of
    include/s2t_hip.h; max_len 1023 is the last one accepted"""
    _, DEC, _, L = _mods()
    lib = L.load()
    _, ses, _ = _session(dict(id="refuse", dtype=F32, D=256, beam=2, B=1, max_len=1023, V=96), monkeypatch)
    d = ses.desc
    assert 0 < lib.s2t_decode_lds_bytes(ses.addr) <= DEC.LDS_CAP

    def refused(**fields):
        old = {k: getattr(d, k) for k in fields}
        for k, v in fields.items():
            setattr(d, k, v)
        try:
            assert lib.s2t_decode_lds_bytes(ses.addr) == 0, fields
            assert lib.s2t_decode_step(ses.addr, L.stream()) == ENOTSUP, fields
        finally:
            for k, v in old.items():
                setattr(d, k, v)
    refused(max_len=1024)
    refused(beam=17)
    refused(B=43, beam=3)                   # B x beam = 129
    refused(V=32769, ldv=32769)
    refused(V=4)                            # below 2 beam + 1
    refused(Tsp=200)
    refused(ffn_slices=d.ffn // 32)         # 32 hidden units per slice
    refused(ffn_slices=1)                   # 512
    assert lib.s2t_decode_lds_bytes(ses.addr) > 0
