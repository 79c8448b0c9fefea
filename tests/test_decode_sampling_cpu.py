"""CPU checks of the sampling search (`Sampling`, fairseq/search.py:164-278): the host class against step outputs captured from the
reference with forced draws (tests/golden/sampling.npz, made by tests/golden/make_sampling_fixture.py), the package's hash against the
restatement of tests/decode_sampling_ref.py, the ABI of the new entry points, and the host generator loop with draws forced to EOS."""
import ctypes
import types

import numpy as np
import pytest
import torch

import decode_sampling_ref as SR
from helpers import load_golden
from fbk_fairseq_st_amd import lib as L
from fbk_fairseq_st_amd import sampling as SMP

EINVAL, ENOTSUP = -22, -95
PAD, EOS, UNK = 1, 2, 3


class _Dict:
    def __init__(self, V):
        self.V = V

    def pad(self):
        return PAD

    def eos(self):
        return EOS

    def unk(self):
        return UNK

    def __len__(self):
        return self.V


def _cases():
    g = load_golden("sampling")
    out = []
    for i in range(int(g["n_step"])):
        step, topk, topp = g["s%d_par" % i]
        out.append(dict(i=i, lprobs=g["s%d_lprobs" % i], cum=g["s%d_cum" % i], step=int(step), topk=int(topk), topp=float(topp),
                        support=g["s%d_support" % i], scores=g["s%d_out_scores" % i], tokens=g["s%d_out_tokens" % i],
                        beams=g["s%d_out_beams" % i]))
    return out


def _rows(c):
    B, beam, V = c["lprobs"].shape
    return c["lprobs"][:, 0, :] if c["step"] == 0 else c["lprobs"].reshape(B * beam, V)


def test_fixture_covers_the_edges():
    cs = _cases()
    assert len(cs) >= 12
    for mode in (lambda c: c["topp"] <= 0 and c["topk"] <= 0, lambda c: c["topp"] <= 0 and c["topk"] > 0, lambda c: c["topp"] > 0):
        assert any(mode(c) and c["step"] == 0 for c in cs) and any(mode(c) and c["step"] > 0 for c in cs)
    finite = lambda c: np.isfinite(_rows(c)).sum(1)
    assert any(c["topk"] == 1 and c["topp"] <= 0 for c in cs)
    assert any(c["topp"] <= 0 and c["topk"] >= finite(c).max() and c["topk"] > 1 for c in cs), "k >= the number of finite columns"
    assert any(c["topp"] > 0 and (c["support"].sum(1) == 1).all() for c in cs), "P so small that one column is kept"
    mass = lambda c: np.exp(_rows(c).astype(np.float64)).sum(1)
    assert any(c["topp"] > 0 and (c["topp"] >= mass(c)).all() and (c["support"].sum(1) == finite(c)).all() for c in cs), "P >= the total mass"
    assert any(c["topp"] > 0 and c["topk"] > 0 for c in cs), "top-p takes precedence over top-k"
    assert all((~np.isfinite(_rows(c))).any(1).all() for c in cs), "every row has -inf columns"
    for c in cs:                                                   # no kept set of the fixture hangs on a rounding
        if c["topp"] > 0:
            for r in _rows(c):
                m = np.cumsum(np.sort(np.exp(r.astype(np.float64)))[::-1])
                assert np.abs(m - c["topp"]).min() >= 1e-4


def test_kept_sets_equal_the_reference_support():
    for c in _cases():
        for r, sup in zip(_rows(c), c["support"]):
            assert np.array_equal(SMP.kept_set(r, max(c["topk"], 0), c["topp"]), sup), c["i"]
            assert np.array_equal(SR.kept_set(r, max(c["topk"], 0), c["topp"])[0], sup), c["i"]


def _forced(tokens):
    """a Sampling whose draws are the given tokens (slot order), each checked to lie in the kept set"""
    from fbk_fairseq_st_amd.sequence_generator import Sampling

    class Forced(Sampling):
        def _choose(self, step, lp, keep, slot):
            t = int(tokens[slot])
            assert keep[t], "the reference drew a token outside the kept set"
            return t
    return Forced


def test_forced_draws_reproduce_the_reference_step():
    """scores 1e-6, tokens and beams exact: the step-0 first-row rule, beams 0 at step 0 and arange later, cumulative scores"""
    from fbk_fairseq_st_amd.sequence_generator import Sampling
    for c in _cases():
        B, beam, V = c["lprobs"].shape
        sc = torch.zeros(B, beam, max(c["step"], 1))
        sc[:, :, c["step"] - 1] = torch.from_numpy(c["cum"])
        strat = _forced(c["tokens"].reshape(-1))(_Dict(V), c["topk"], c["topp"])
        s, t, b = strat.step(c["step"], torch.from_numpy(c["lprobs"]).clone(), sc)
        assert t.tolist() == c["tokens"].tolist() and b.tolist() == c["beams"].tolist(), c["i"]
        assert b.tolist() == ([[0] * beam] * B if c["step"] == 0 else [list(range(beam))] * B)
        np.testing.assert_allclose(s.numpy(), c["scores"], rtol=0, atol=1e-6)
        # the class's own draw: a token of the kept set, the same for the same (seed, call), another for another call
        own = Sampling(_Dict(V), c["topk"], c["topp"], seed=5)
        own.new_call()
        s1, t1, b1 = own.step(c["step"], torch.from_numpy(c["lprobs"]).clone(), sc)
        s2, t2, _ = own.step(c["step"], torch.from_numpy(c["lprobs"]).clone(), sc)
        assert t1.tolist() == t2.tolist() and torch.equal(s1, s2) and b1.tolist() == c["beams"].tolist()
        rows = t1.reshape(-1, beam if c["step"] == 0 else 1)
        for r in range(rows.shape[0]):
            assert all(c["support"][r][int(v)] for v in rows[r]), c["i"]


def test_the_call_counter_changes_the_draws_and_the_seed_repeats_them():
    from fbk_fairseq_st_amd.sequence_generator import Sampling
    lp = torch.log_softmax(torch.from_numpy(np.random.RandomState(3).randn(4, 3, 50).astype(np.float32)), -1)
    sc = torch.zeros(4, 3, 1)

    def calls(seed):
        s = Sampling(_Dict(50), seed=seed)
        out = []
        for _ in range(3):
            s.new_call()
            out.append(s.step(1, lp.clone(), sc)[1].tolist())
        return out
    a, b = calls(7), calls(7)
    assert a == b and a[0] != a[1] and a[1] != a[2] and calls(8) != a
    assert Sampling(_Dict(50), seed=7).key != Sampling(_Dict(50), seed=8).key
    # a hierarchical start: every slot draws from its own row at step 0, from its own start score, and continues itself
    s = Sampling(_Dict(50), 1, seed=7)
    prev = torch.arange(12, dtype=torch.float32).view(4, 3, 1)
    sc0, t0, b0 = s.step(0, lp.clone(), sc, prev)
    assert t0.tolist() == lp.argmax(-1).tolist() and b0.tolist() == [[0, 1, 2]] * 4
    assert torch.allclose(sc0, lp.max(-1)[0] + prev[:, :, 0])


def test_package_hash_equals_the_restatement():
    rs = np.random.RandomState(11)
    n = 100000
    cols = rs.randint(0, 32768, n)
    for key, step, slot in ((0, 0, 0), (SMP.make_key(1, 1), 3, 5), (2 ** 64 - 1, 1023, 127), (SMP.make_key(123456789, 4000000000), 17, 64)):
        h = SMP.hash32(key, step, slot, cols)
        assert h.dtype == np.uint32 and np.array_equal(h, SR.hash32(key, step, slot, cols))
        for i in range(0, n, 9973):
            assert int(h[i]) == SR.hash32_scalar(key, step, slot, int(cols[i]))
    steps, slots = rs.randint(0, 1024, 200), rs.randint(0, 128, 200)
    for i in range(200):
        assert int(SMP.hash32(5, steps[i], slots[i], [cols[i]])[0]) == SR.hash32_scalar(5, int(steps[i]), int(slots[i]), int(cols[i]))
    u = SMP.uniform(SMP.hash32(9, 1, 2, np.arange(n)))
    assert u.dtype == np.float32 and u.min() > 0 and u.max() < 1
    assert np.array_equal(u.astype(np.float64), SR.uniform(SR.hash32(9, 1, 2, np.arange(n)))), "the uniform is exact in f32"
    assert abs(float(u.mean()) - 0.5) < 0.005


# ------------------------------------------------------------------ ABI
def _bindings():
    L.build_fastcall()
    fast = L._load_fastcall(None)
    assert fast is not None, "the generated binding did not load"
    L.load()
    return [("ctypes", L.load_ctypes()), ("fastcall", fast)]


def test_abi_version_and_struct_sizes_are_unchanged():
    assert L.load().s2t_abi_version() == 9 and L.ABI_VERSION == 9
    assert ctypes.sizeof(L.DecodeDesc) == L.DecodeDesc.diverse_groups.offset + 8
    assert ctypes.sizeof(L.DecodeRules) == 16
    assert ctypes.sizeof(L.DecodeSample) == 16 and L.DecodeSample.key.offset == 8
    for name in ("s2t_sample_rows", "s2t_decode_step_sample", "s2t_decode_graph_create_sample"):
        assert name in L.SIGNATURES


def test_new_calls_refuse_in_the_documented_order():
    ex = ctypes.c_void_p(0)
    exa = ctypes.addressof(ex)
    for what, b in _bindings():
        d = L.DecodeDesc()                                          # zeroed: outside the limits (S2T_ENOTSUP), looked at last
        arr = (ctypes.c_void_p * 1)(ctypes.addressof(d))
        aa = ctypes.addressof(arr)
        ok, bad_k, bad_p = L.DecodeSample(), L.DecodeSample(), L.DecodeSample()
        ok.topk, ok.topp = 5, 0.5
        bad_k.topk = -1
        bad_p.topp = float("nan")
        r1, rneg = L.DecodeRules(), L.DecodeRules()
        r1.no_repeat_ngram, rneg.no_repeat_ngram = 1, -1
        A = ctypes.addressof

        def both(dv, n, r, s):
            got = (b.s2t_decode_step_sample(dv, n, r, s, None), b.s2t_decode_graph_create_sample(dv, n, r, s, 8, exa))
            assert ex.value is None and got[0] == got[1], (what, got)
            return got[0]
        # 1. the sample struct, before anything else
        assert both(None, 1, None, None) == EINVAL and both(aa, 1, None, None) == EINVAL
        assert both(aa, 1, A(r1), A(bad_k)) == EINVAL and both(aa, 1, A(r1), A(bad_p)) == EINVAL
        # 2. what s2t_decode_step_ensemble checks, in its order
        assert both(None, 1, None, A(ok)) == EINVAL and both(aa, 0, None, A(ok)) == EINVAL and both(aa, 9, A(r1), A(ok)) == EINVAL
        assert both(aa, 1, A(rneg), A(ok)) == EINVAL and both(aa, 1, A(r1), A(ok)) == ENOTSUP
        pair = [L.DecodeDesc(), L.DecodeDesc()]
        pair[1].beam = 3
        parr = (ctypes.c_void_p * 2)(*[A(p) for p in pair])
        assert both(A(parr), 2, None, A(ok)) == EINVAL
        dneg = L.DecodeDesc()
        dneg.diverse_groups = -1
        assert both(A((ctypes.c_void_p * 1)(A(dneg))), 1, None, A(ok)) == EINVAL
        assert both(aa, 1, None, A(ok)) == ENOTSUP
        # graph_exec and n_steps first
        assert b.s2t_decode_graph_create_sample(aa, 1, None, None, 8, None) == EINVAL
        assert b.s2t_decode_graph_create_sample(aa, 1, None, A(ok), 0, exa) == EINVAL
        assert b.s2t_decode_graph_create_sample(aa, 1, None, A(ok), 65, exa) == EINVAL
        # s2t_sample_rows: nothing is dereferenced before the checks (the pointers are never read here)
        buf = (ctypes.c_float * 64)()
        p = A(buf)
        args = lambda **kw: [kw.get(k, v) for k, v in (("x", p), ("rows", 1), ("V", 8), ("ld", 8), ("draws", 1), ("topk", 0), ("topp", 0.0),
                                                       ("key", 2 ** 63 + 1), ("step", 0), ("tok", p), ("lp", p), ("nk", p), ("st", None))]
        for kw in (dict(x=None), dict(tok=None), dict(lp=None), dict(nk=None), dict(rows=0), dict(draws=0), dict(topk=-1),
                   dict(topp=float("nan")), dict(ld=7), dict(V=0), dict(step=-1)):
            assert b.s2t_sample_rows(*args(**kw)) == EINVAL, (what, kw)
        assert b.s2t_sample_rows(*args(V=32769, ld=32769)) == ENOTSUP
        assert b.s2t_sample_rows(*args(V=32769, ld=32769, topk=-1)) == EINVAL


def test_build_generator_keeps_refusing_the_flag():
    import test_decode_diverse_cpu as TD
    with pytest.raises(NotImplementedError):
        TD._build(sampling=True)


# ------------------------------------------------------------------ the host loop
class _ToyDecoder:
    """what SequenceGenerator._beam_search reads of an incremental decoder: logits that depend on the last token only"""

    def __init__(self, V, seed):
        self.table = torch.from_numpy(np.random.RandomState(seed).randn(V, V).astype(np.float32) * 2)
        self.table[:, EOS] = 3.0                                     # EOS among the best of every row: inside every kept set
        enc = types.SimpleNamespace(reorder_encoder_out=lambda e, order: e)
        self.owner = types.SimpleNamespace(training=False, encoder=enc, hp=types.SimpleNamespace(dec_layers=1))
        self.engine = types.SimpleNamespace(hp=types.SimpleNamespace(layernorm_embedding=False), dtype=torch.float32)
        self.pfx = "decoder."

    def begin_incremental(self, enc, n):
        return {"attn": None}

    def reorder_incremental(self, st, order):
        pass

    def step_incremental(self, st, last):
        return self.table[last].clone()


@pytest.mark.parametrize("topk,topp", [(-1, -1.0), (6, -1.0), (-1, 0.7)], ids=["plain", "topk6", "topp0.7"])
def test_host_loop_with_eos_draws(topk, topp, monkeypatch):
    """draws forced to EOS at steps 1 and 3 for some slots: the finalised slots are black-listed and the loop goes on with k = beam
    candidates; every sentence returns `beam` hypotheses ending in EOS whose scores are the sums of their positional scores"""
    from cpu_stubs import cpu_kernels
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    V, B, beam, max_len = 40, 3, 4, 9
    forced = []

    class Forced(Sampling):
        def _choose(self, step, lp, keep, slot):
            if step in (1, 3) and slot % 3 != 1 and keep[EOS]:
                forced.append((step, slot))
                return EOS
            return super()._choose(step, lp, keep, slot)
    model = types.SimpleNamespace(training=False, eval=lambda: None, train=lambda t=True: None, max_decoder_positions=lambda: 1024)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen = SequenceGenerator([model], _Dict(V), beam_size=beam, max_len_b=max_len, min_len=1, normalize_scores=False,
                            search_strategy=Forced(_Dict(V), topk, topp, seed=3))
    gen.search.new_call()
    enc = types.SimpleNamespace(encoder_out=torch.zeros(5, B, 8), encoder_padding_mask=None, src_lengths=None)
    with cpu_kernels():
        hyps = gen._beam_search(_ToyDecoder(V, 1), enc, B, torch.device("cpu"), max_len, gen.search, None, PAD, UNK, EOS, V)
    assert forced and any(s == 1 for s, _ in forced), "no draw was forced to EOS"
    assert "launches_per_step" not in gen.last_stats
    assert len(hyps) == B
    lengths = set()
    for hs in hyps:
        assert len(hs) == beam
        sc = [float(h["score"]) for h in hs]
        assert sc == sorted(sc, reverse=True)
        for h in hs:
            toks = h["tokens"].tolist()
            lengths.add(len(toks))
            assert toks[-1] == EOS and EOS not in toks[:-1] and PAD not in toks and len(toks) <= max_len + 1
            assert abs(float(h["score"]) - float(h["positional_scores"].sum())) < 1e-4
    assert 2 in lengths, "a hypothesis finalised by the EOS forced at step 1"
