"""The sampling search (`Sampling`: unrestricted, top-k, nucleus) on the GPU: the stand-alone kernel behind the step-by-step route
(s2t_sample_rows, csrc/sample.hip), the SAMPLE forms of the device-resident search (csrc/decode.hip, s2t_decode_step_sample) and the
two routes of SequenceGenerator against each other.  The reference of every draw is tests/decode_sampling_ref.py: the hash and the
uniform bit for bit, the Gumbel keys, kept sets and arg-max in float64.

A draw whose two best float64 keys are closer than SR.NEAR_TIE (1e-4: keys lie in (-40, 40), the f32 errors of logf(logf) and of the
log-softmax are a few ulp of 64, about 1e-5 -- a tenfold margin) may come out as either of the two; a nucleus whose boundary mass lies
within SR.NEAR_P * P (1e-5 P) of P may differ in size by one.  How many such rows a test may hold is asserted from the reference alone,
before the device output is looked at.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import decode_ref as R
import decode_sampling_ref as SR
import test_decode_gpu as TG
from test_decode_gpu import BF, BOS, DEV, EOS, F32, PAD, UNK

pytestmark = pytest.mark.gpu

KEY = (20240611 << 32) | 1
MODES = [("plain", 0, 0.0)] + [("topk%d" % k, k, 0.0) for k in (1, 2, 64, -1)] + [("topp%g" % p, 0, p) for p in (1e-6, 0.5, 0.999999, 2.0)]


# ------------------------------------------------------------------ 1. s2t_sample_rows against the float64 restatement
def _rows_input(V, rows, seed):
    """log-probabilities with -inf columns and duplicated values in every row; from five rows on also: many -inf columns, equal values
    straddling the top-k boundaries (k = 1, 2 and 64), one finite column, a row of -inf"""
    rs = np.random.RandomState(seed)
    x = torch.log_softmax(torch.from_numpy(rs.randn(rows, V).astype(np.float32) * 2.0), -1).numpy().copy()
    for r in range(rows):
        x[r, rs.choice(V, max(V // 10, 1), replace=False)] = -np.inf
        fin = np.nonzero(np.isfinite(x[r]))[0]
        top = fin[np.argsort(-x[r, fin], kind="stable")]
        x[r, top[1]] = x[r, top[2]] = x[r, top[0]]                 # three equal maxima: top-1 and top-2 cut them by column
        a = rs.choice(fin, 6, replace=False)
        x[r, a[:3]] = x[r, a[3:]]                                   # and equal values elsewhere
    if rows >= 5:
        x[1, rs.choice(V, V - 7, replace=False)] = -np.inf
        fin = np.nonzero(np.isfinite(x[2]))[0]
        x[2, fin[:min(70, fin.size)]] = x[2, fin].max() + 0.5       # up to 70 equal values on top: k = 64 cuts them by column
        x[3, :] = -np.inf
        x[3, V // 2] = -0.25
        x[4, :] = -np.inf
    return x


@pytest.mark.parametrize("rows", [1, 5, 128])
@pytest.mark.parametrize("V", [33, 257, 1000, 32768])
def test_sample_rows_against_float64(V, rows):
    from fbk_fairseq_st_amd import kernels as K
    x = _rows_input(V, rows, 2000 + V + rows)
    ref = SR.Rows(x)
    xd = torch.from_numpy(x).to(DEV)
    step = 3
    cases, n_near = [], 0
    for draws in (1, 4):
        gs = [ref.gumbel(KEY, step, np.arange(rows) * draws + j) for j in range(draws)]
        for name, k, p in MODES:
            k = V if k < 0 else k
            keep, near_p, _ = ref.kept(k, p)
            dr = [ref.draw(keep, g) for g in gs]
            near_rows = near_p.copy()
            for tok, sec, gap in dr:
                near_rows |= gap < SR.NEAR_TIE
            n_near += int(near_rows.sum())
            cases.append((draws, name, k, p, keep, near_p, dr))
    total = rows * len(cases)
    assert n_near <= 0.01 * total, "%d of %d rows are near ties or near boundaries: choose other inputs" % (n_near, total)
    for draws, name, k, p, keep, near_p, dr in cases:
        what = "V %d rows %d draws %d %s" % (V, rows, draws, name)
        tok, lp, nk = K.sample_rows(xd, draws, k, p, KEY, step)
        tok, lp, nk = tok.cpu().numpy(), lp.cpu().numpy(), nk.cpu().numpy()
        assert ((tok >= 0) & (tok < V)).all(), what
        want = np.take_along_axis(x, tok.astype(np.int64), 1)
        assert np.array_equal(lp.view(np.int32), want.view(np.int32)), what + ": lp_out is not lprobs[row, tok]"
        n_ref = keep.sum(1)
        bad = (nk != n_ref) & ~(near_p & (np.abs(nk - n_ref) <= 1))
        assert not bad.any(), "%s: n_kept %s != %s in rows %s" % (what, nk[bad][:4], n_ref[bad][:4], np.nonzero(bad)[0][:4])
        for j, (rt, rsec, gap) in enumerate(dr):
            ok = (tok[:, j] == rt) | ((gap < SR.NEAR_TIE) & (tok[:, j] == rsec))
            if near_p.any():                                       # a nucleus one column larger or smaller: only that the token is legal
                ok |= near_p
            assert ok.all(), "%s: draw %d of rows %s: %s != %s" % (what, j, np.nonzero(~ok)[0][:4], tok[~ok, j][:4], rt[~ok][:4])
            empty = n_ref == 0
            assert (tok[empty, j] == 0).all() and np.isneginf(lp[empty, j]).all(), what + ": a row of -inf gives token 0 with -inf"


# ------------------------------------------------------------------ 2. the distribution
def _chi2_quantile(df, z=3.719016):
    """Wilson-Hilferty: the 1 - 1e-4 quantile of chi-square(df) (z = the normal quantile of 1 - 1e-4)"""
    return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def _counts(xd, topk, key, V):
    from fbk_fairseq_st_amd import kernels as K
    toks = torch.stack([K.sample_rows(xd, 1, topk, 0.0, key, step)[0].view(-1) for step in range(64)])
    return toks, np.bincount(toks.cpu().numpy().reshape(-1), minlength=V)


@pytest.mark.parametrize("key", [KEY, (7 << 32) | 3, (123456789 << 32) | 4000000000])
def test_draws_follow_the_softmax(key):
    V, rows = 16, 128
    logits = np.linspace(-2.0, 2.0, V).astype(np.float32)[np.random.RandomState(5).permutation(V)]
    lp = torch.log_softmax(torch.from_numpy(logits), -1)
    xd = lp[None, :].repeat(rows, 1).to(DEV)
    p = np.exp(lp.double().numpy())
    toks, n = _counts(xd, 0, key, V)
    N = rows * 64
    assert n.sum() == N == 8192
    chi2 = float(((n - N * p) ** 2 / (N * p)).sum())
    print("key %x: chi2 %.2f (bound %.2f)" % (key, chi2, _chi2_quantile(V - 1)))
    assert chi2 < _chi2_quantile(V - 1)
    top4 = np.argsort(-logits, kind="stable")[:4]
    toks4, n4 = _counts(xd, 4, key, V)
    assert n4.sum() == N and n4[top4].sum() == N, "a draw fell outside the top 4"
    q = p[top4] / p[top4].sum()
    chi2 = float(((n4[top4] - N * q) ** 2 / (N * q)).sum())
    print("key %x top-4: chi2 %.2f (bound %.2f)" % (key, chi2, _chi2_quantile(3)))
    assert chi2 < _chi2_quantile(3)
    again, _ = _counts(xd, 0, key, V)
    assert torch.equal(again, toks), "the same key gave other draws"
    other, _ = _counts(xd, 0, key + 1, V)                           # the next call of the same seed
    assert not torch.equal(other, toks), "another call counter gave the same draws"


# ------------------------------------------------------------------ 3. the session, step by step
def _check_state(ses, host, t, B, beam, max_len, what):
    N, M2 = B * beam, max_len + 2
    for k in ("blacklist", "nfin", "finished", "steps"):
        v = TG._host(ses, k)
        assert np.array_equal(v, host[k]), "%s: %s %s != %s" % (what, k, v.tolist(), host[k].tolist())
    th, ph, ch = TG._host(ses, "tok_hist", (M2, N)), TG._host(ses, "par_hist", (M2, N)), TG._host(ses, "cum_hist", (M2, N))
    assert np.array_equal(th[:t + 2], host["tok_hist"][:t + 2]), "%s: tok_hist %s != %s" % (what, th[t + 1].tolist(), host["tok_hist"][t + 1].tolist())
    assert np.array_equal(ph[1:t + 2], host["par_hist"][1:t + 2]), "%s: par_hist %s != %s" % (what, ph[t + 1].tolist(), host["par_hist"][t + 1].tolist())
    a, b = ch[1:t + 2], host["cum_hist"][1:t + 2]
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and np.abs(np.where(np.isneginf(a), 0, a - b)).max() <= 1e-5, what + ": cum_hist"
    na = t + 1 if t < max_len else t
    assert np.array_equal(TG._host(ses, "anc", (N, max_len + 1))[:, :na], host["anc"][:, :na]), what + ": anc"
    fs, fr, fsc = TG._host(ses, "fin_step", (B, beam)), TG._host(ses, "fin_row", (B, beam)), TG._host(ses, "fin_score", (B, beam))
    for s in range(B):
        k = int(host["nfin"][s])
        assert fs[s, :k].tolist() == host["fin_step"][s, :k].tolist() and fr[s, :k].tolist() == host["fin_row"][s, :k].tolist(), what
        assert np.abs(fsc[s, :k] - host["fin_score"][s, :k]).max(initial=0.0) <= 1e-5, what


@pytest.mark.parametrize("name,topk,topp", [("plain", 0, 0.0), ("topk5", 5, 0.0), ("topp0.8", 0, 0.8)])
def test_session_step_by_step(name, topk, topp):
    """one s2t_decode_step_sample at a time; after every step the session's own logits go through the float64 row rules and the
    restatement's draw, and the records must be those of the reference loop"""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd import lib as L
    B, beam, V, max_len, min_len, seed = 2, 3, 96, 9, 1, 4
    N = B * beam
    torch.manual_seed(seed)
    eng = TG.DecEngine(256, 256, 1, V, F32, seed, "relu", 4.0)
    enc = torch.randn(20, B, 256, device=DEV)
    klen = torch.tensor([20, 13], dtype=torch.int32, device=DEV)
    ses = DEC.BeamDecodeSession(eng, "decoder.", enc, klen, beam, max_len, min_len, PAD, UNK, EOS, V, sampling=dict(topk=topk, topp=topp, key=KEY))
    assert ses.ok and ses.launches_per_step == 3 * 1 + 4, "sampling adds no launch"
    lib, st = L.load(), L.stream()
    L.check(lib.s2t_decode_begin(ses.addr, BOS, st), "s2t_decode_begin")
    host = R.new_state(B, beam, max_len, BOS)
    early = 0
    for t in range(max_len + 1):
        what = "%s step %d" % (name, t)
        L.check(lib.s2t_decode_step_sample(ses.descs_addr, 1, None, ses.sample_addr, st), "s2t_decode_step_sample")
        torch.cuda.synchronize()
        logits = ses.bufs["logits"].clone()
        zero = torch.zeros(N, dtype=torch.float64, device=DEV)
        lp = R.row_reference(logits, t, beam, PAD, UNK, EOS, max_len, min_len, 1.0, 0.0, zero, True)[0].cpu().numpy()
        if t == 0:
            lp = lp[(np.arange(N) // beam) * beam]                  # every slot draws from the sentence's first row
        ref = SR.Rows(lp)
        keep, near_p, _ = ref.kept(topk, topp)
        tok, sec, gap = ref.draw(keep, ref.gumbel(KEY, t, np.arange(N)))
        live = np.repeat(host["steps"] <= max_len, beam)
        assert not (near_p & live).any() and (gap[live] >= SR.NEAR_TIE).all(), what + ": a near tie -- choose another seed"
        base = host["cum_hist"][t].astype(np.float64) if t > 0 else np.zeros(N)
        val = (lp[np.arange(N), tok] + base).astype(np.float32)
        nf0 = int(host["nfin"].sum())
        SR.sent_step_sample(host, val, tok, beam, EOS, max_len)
        if t < max_len:
            early += int(host["nfin"].sum()) - nf0
        _check_state(ses, host, t, B, beam, max_len, what)
    assert TG._host(ses, "finished").all() and early > 0, "no slot drew EOS before the forced step"


# ------------------------------------------------------------------ 4. - 7. whole searches
def _dc(dtype, temperature=0.5):
    import test_decode_diverse_gpu as TD
    task, model, net, opts, _, _, _ = TD._fixture("dc", dtype)
    return task, model, net, dict(opts, beam_size=4, max_len_b=10, temperature=temperature)


def _margins(captured, topk, topp, key, beam):
    """from the step route's own log-probabilities: the smallest top-two key gap and the smallest distance of a cumulative mass from P"""
    gap_min, p_min, wide = np.inf, np.inf, 0
    for step, lp in captured:
        B = lp.shape[0]
        rows = lp[:, 0, :] if step == 0 else lp.reshape(B * beam, -1)
        draws = beam if step == 0 else 1
        ref = SR.Rows(rows)
        keep, _, margin = ref.kept(topk, topp)
        p_min = min(p_min, float(margin.min()))
        wide += int((keep.sum(1) > 1).sum())
        for j in range(draws):
            gap_min = min(gap_min, float(ref.draw(keep, ref.gumbel(key, step, np.arange(rows.shape[0]) * draws + j))[2].min()))
    return gap_min, p_min, wide


def _step_route(models, task, net, opts, topk, topp, monkeypatch, **gen_kw):
    """the step-by-step route with the first seed whose every draw keeps its top-two key gap >= 1e-3 and every nucleus boundary >= 1e-3
    from P (judged by the restatement on the route's own log-probabilities: a choice of inputs, made before the device route runs)"""
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    for seed in range(1, 60):
        captured = []

        class Capture(Sampling):
            def step(self, step, lprobs, scores):
                captured.append((step, lprobs.detach().cpu().numpy().copy()))
                return super().step(step, lprobs, scores)
        strat = Capture(task.target_dictionary, topk, topp, seed=seed)
        gen = SequenceGenerator(models, task.target_dictionary, search_strategy=strat, **opts)
        hyps = gen.generate(models, net, **gen_kw)
        assert "launches_per_step" not in gen.last_stats, "the step route was not taken"
        gap, pm, wide = _margins(captured, strat.topk, strat.topp, strat.key, opts["beam_size"])
        print("seed %d: smallest key gap %.3g, P clear of every cumulative mass by %.3g, %d rows keep more than one column" % (seed, gap, pm, wide))
        if gap >= 1e-3 and pm >= 1e-3:
            assert topk == 1 or wide > 0, "every kept set is a single column: the search is the greedy one"
            return seed, hyps
    raise AssertionError("no seed below 60 keeps every draw clear of a tie")


def _same(dev_h, step_h, beam):
    assert len(dev_h) == len(step_h)
    for hs, ss in zip(dev_h, step_h):
        assert len(hs) == len(ss) == beam
        for h, s_ in zip(hs, ss):
            assert h["tokens"].tolist() == s_["tokens"].tolist()
            assert abs(float(h["score"]) - float(s_["score"])) < 1e-4
            np.testing.assert_allclose(h["positional_scores"].cpu().numpy(), s_["positional_scores"].cpu().numpy(), atol=1e-4)


@pytest.mark.parametrize("name,topk,topp", [("plain", -1, -1.0), ("topk5", 5, -1.0), ("topp0.8", -1, 0.8)])
def test_device_route_equals_step_route(name, topk, topp, monkeypatch):
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    # (the nucleus case runs colder: rows peaked enough that a seed exists whose every boundary is 1e-3 clear of P)
    task, model, net, opts = _dc(F32, 0.2 if topp > 0 else 0.5)
    seed, step_h = _step_route([model], task, net, opts, topk, topp, monkeypatch)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "1")
    plain = SequenceGenerator([model], task.target_dictionary, **opts)
    plain.generate([model], net)
    for graph in (True, False):
        gen = SequenceGenerator([model], task.target_dictionary, search_strategy=Sampling(task.target_dictionary, topk, topp, seed=seed), **opts)
        gen.device_graph = graph
        dev_h = gen.generate([model], net)
        assert gen.last_stats.get("launches_per_step") == plain.last_stats["launches_per_step"], "the device route was not taken"
        _same(dev_h, step_h, opts["beam_size"])
    assert len({tuple(h["tokens"].tolist()) for hs in step_h for h in hs}) > len(step_h), "the slots of a sentence all drew the same"


def test_ensemble_with_ngram_blocking_and_prefix_device_route_equals_step_route(monkeypatch):
    import test_decode_ensemble_gpu as TE
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    built = TE._models(F32)
    task, models = built[0][0], [b[1] for b in built]
    _, _, net = TE._net()
    opts = dict(TE.OPTS, beam_size=4, max_len_b=10, no_repeat_ngram_size=3, temperature=0.5)
    P2 = [[17, 45], [33, PAD], [PAD, PAD]]
    prefix = torch.tensor(P2, dtype=torch.int64, device=DEV)
    seed, step_h = _step_route(models, task, net, opts, 5, -1.0, monkeypatch, prefix_tokens=prefix)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "1")
    for graph in (True, False):
        gen = SequenceGenerator(models, task.target_dictionary, search_strategy=Sampling(task.target_dictionary, 5, seed=seed), **opts)
        gen.device_graph = graph
        dev_h = gen.generate(models, net, prefix_tokens=prefix)
        assert gen.last_stats.get("launches_per_step") == TE._formula(models), "the device route was not taken"
        _same(dev_h, step_h, 4)
    for b, hs in enumerate(step_h):
        for h in hs:
            toks = h["tokens"].tolist()
            forced = [v for v in P2[b] if v != PAD]
            assert toks[:len(forced)] == forced and not TE._repeats(toks, 3)


@pytest.mark.parametrize("route", ["device", "steps"])
def test_top1_is_the_greedy_search(route, monkeypatch):
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    task, model, net, opts = _dc(F32)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "1" if route == "device" else "0")
    greedy = SequenceGenerator([model], task.target_dictionary, **dict(opts, beam_size=1)).generate([model], net)
    gen = SequenceGenerator([model], task.target_dictionary, search_strategy=Sampling(task.target_dictionary, 1, seed=9), **opts)
    hyps = gen.generate([model], net)
    assert ("launches_per_step" in gen.last_stats) == (route == "device")
    for hs, gs in zip(hyps, greedy):
        assert len(hs) == opts["beam_size"] and len(gs) == 1
        for h in hs:
            assert h["tokens"].tolist() == gs[0]["tokens"].tolist()
            assert abs(float(h["score"]) - float(gs[0]["score"])) < 1e-4


def _score_is_the_sum(h, opts):
    n = h["tokens"].shape[0]
    want = float(h["positional_scores"].sum()) / n ** opts["len_penalty"]
    assert abs(float(h["score"]) - want) < 1e-4 * max(1.0, abs(want))


@pytest.mark.parametrize("topk,topp", [(-1, -1.0), (5, -1.0), (-1, 0.8)], ids=["plain", "topk5", "topp0.8"])
def test_bf16_device_route_is_well_formed(topk, topp, monkeypatch):
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    task, model, net, opts = _dc(BF)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "1")
    gen = SequenceGenerator([model], task.target_dictionary, search_strategy=Sampling(task.target_dictionary, topk, topp, seed=2), **opts)
    hyps = gen.generate([model], net)
    assert "launches_per_step" in gen.last_stats
    again = gen.generate([model], net)                               # the next call: other draws
    assert [[h["tokens"].tolist() for h in hs] for hs in hyps] != [[h["tokens"].tolist() for h in hs] for hs in again]
    for hs in hyps:
        assert len(hs) == opts["beam_size"]
        for h in hs:
            toks = h["tokens"].tolist()
            assert toks[-1] == EOS and EOS not in toks[:-1] and len(toks) <= opts["max_len_b"] + 1
            _score_is_the_sum(h, opts)


def test_searches_the_device_route_leaves_to_the_step_route(monkeypatch):
    """n-gram size 1, a prefix holding EOS and hierarchical start scores build no session (the session classes raise here) and the
    step-by-step route answers; a session asked for sampling with groups, or with every slot live at step 0, refuses before it
    allocates anything (a Sampling strategy cannot carry groups: the two are different search_strategy objects)"""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd.sequence_generator import Sampling, SequenceGenerator
    task, model, net, opts = _dc(F32)
    eng = TG.DecEngine(256, 256, 1, 200, F32, 0)
    enc = torch.randn(20, 2, 256, device=DEV)
    mk = lambda **kw: DEC.BeamDecodeSession(eng, "decoder.", enc, None, 4, 8, 1, PAD, UNK, EOS, 200, sampling=dict(topk=0, topp=0.0, key=1), **kw)
    assert mk().ok
    for kw in (dict(diverse_groups=2), dict(step0_all_slots=True, init_scores=torch.zeros(8))):
        ses = mk(**kw)
        assert not ses.ok and ses.members == [], "refused before a member is built"
    assert not DEC.BeamDecodeSession(eng, "decoder.", enc, None, 4, 8, 1, PAD, UNK, EOS, 200, sampling=dict(topk=-1, topp=0.0, key=1)).ok

    def no_session(*a, **k):
        raise RuntimeError("a session was built for a search the device route does not handle")
    monkeypatch.setattr(DEC, "BeamDecodeSession", no_session)
    monkeypatch.setattr(DEC, "EnsembleDecodeSession", no_session)
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "1")
    B = net["net_input"]["src_tokens"].shape[0]
    pre = torch.full((B, 2), PAD, dtype=torch.int64, device=DEV)
    pre[0, 1] = EOS
    pre[0, 0] = 17
    mkgen = lambda **kw: SequenceGenerator([model], task.target_dictionary, search_strategy=Sampling(task.target_dictionary, 5, seed=3), **dict(opts, **kw))
    gen = mkgen(no_repeat_ngram_size=1)
    with pytest.raises(AssertionError):                             # as with the beam search: EOS is banned through the <bos> column
        gen.generate([model], net)
    assert gen.last_stats == {"steps": opts["max_len_b"] + 1}
    gen = mkgen()
    hyps = gen.generate([model], net, prefix_tokens=pre)
    assert "launches_per_step" not in gen.last_stats and len(hyps) == B
    assert all(h["tokens"].tolist() == [17, EOS] for h in hyps[0])
    for hs in hyps:
        assert len(hs) == opts["beam_size"] and all(int(h["tokens"][-1]) == EOS for h in hs)
    # hierarchical start scores: _device_search declines before it looks at anything else
    gen = SequenceGenerator([model], task.target_dictionary, search_strategy=Sampling(task.target_dictionary, 5, seed=3), **opts)
    assert gen._device_search([model.decoder], [None], B, 10, gen.search, None, PAD, UNK, EOS, 96, torch.zeros(B, 4, 1, device=DEV)) is None
