"""The device-resident beam search over an ensemble (s2t_decode_*_ensemble: csrc/decode.hip through decode.EnsembleDecodeSession).

Step by step, in the manner of test_decode_gpu.test_device_search_step_by_step: one s2t_decode_step_ensemble at a time over
test_decode_gpu.DecEngine members that differ in width, depth and encoder length; after every step
  1. every member's logits, final LayerNorm output and K/V cache rows against ITS OWN float64 decoder step (decode_ref.StepRef, within
     that reference's allowances) -- the members share one ancestor table and one step counter, so this shows that both drive every
     member's cache -- and every member's step input x0 against decode_ref.next_input with that member's weights;
  2. every row's 2 beam candidates against the float64 restatement of the ensemble row on the members' own f32 logits
     (decode_ensemble_ref.row_reference_ensemble, bound derived there);
  3. the sentence bookkeeping bit for bit against decode_ref.sent_step.
The candidate check is shown to reject three wrong combinations.  n = 1 through the ensemble calls and a recorded graph leave the
records of the calls they must equal.  Whole searches through SequenceGenerator on two s2t_transformer_s models take the device
route and agree with the step-by-step route and with oracle/s2t_ref.beam_search; the ensembles that must stay on the step route do.
"""

import numpy as np
import pytest
import torch

import decode_ensemble_ref as ER
import decode_ref as R
import test_decode_gpu as TG
from test_decode_gpu import BF, BOS, DEV, EOS, F32, PAD, UNK

pytestmark = pytest.mark.gpu

P3 = [[17, 45, 9], [33, PAD, PAD], [PAD, PAD, PAD]]


def M(D, layers=1, Ts=100, klen=None, eos_scale=2.0):
    return dict(D=D, layers=layers, Ts=Ts, klen=klen, eos_scale=eos_scale)


PAIR = [M(256, 1, 100), M(512, 2, 300, klen=[300, 37, 1])]              # heterogeneous: width, depth, encoder length, ragged klen


def _session(c):
    from fbk_fairseq_st_amd import decode as DEC
    torch.manual_seed(c.get("seed", 0))
    B, beam, dtype = c["B"], c["beam"], c["dtype"]
    engs, members = [], []
    for j, m in enumerate(c["members"]):
        eng = TG.DecEngine(m["D"], 2 * m["D"], m["layers"], c["V"], dtype, 10 * j + c.get("seed", 0), "relu", m["eos_scale"], 1.0, 0)
        enc = torch.randn(m["Ts"], B, m["D"], device=DEV)
        klen = torch.tensor(m["klen"][:B], dtype=torch.int32, device=DEV) if m["klen"] else None
        engs.append(eng)
        members.append((eng, "decoder.", enc, klen))
    init = torch.randn(B * beam, device=DEV) * 0.5 - 1.0 if c.get("init") else None
    prefix = torch.tensor(c["prefix"], dtype=torch.int64) if c.get("prefix") is not None else None
    ses = DEC.EnsembleDecodeSession(members, beam, c["max_len"], c.get("min_len", 1), PAD, UNK, EOS, c["V"], init_scores=init,
                                    step0_all_slots=c.get("init", False), no_repeat_ngram_size=c.get("n", 0), prefix_tokens=prefix)
    assert ses.ok, "the session refused a shape the case is meant to run"
    assert ses.launches_per_step == sum(3 * m["layers"] + 2 for m in c["members"]) + 2
    assert len(ses.bufs_of) == len(members) and len({b["logits"].data_ptr() for b in ses.bufs_of}) == len(members)
    return engs, ses, init


def _check_bookkeeping(ses, host, t, B, beam, max_len, what):
    N, M2 = B * beam, max_len + 2
    for k in ("blacklist", "nfin", "finished", "steps"):
        v = TG._host(ses, k)
        assert np.array_equal(v, host[k]), "%s: %s %s != %s" % (what, k, v.tolist(), host[k].tolist())
    th, ph, ch = TG._host(ses, "tok_hist", (M2, N)), TG._host(ses, "par_hist", (M2, N)), TG._host(ses, "cum_hist", (M2, N))
    assert np.array_equal(th[:t + 2], host["tok_hist"][:t + 2]), what + ": tok_hist"
    assert np.array_equal(ph[1:t + 2], host["par_hist"][1:t + 2]), what + ": par_hist"
    assert np.array_equal(ch[1:t + 2].view(np.int32), host["cum_hist"][1:t + 2].view(np.int32)), what + ": cum_hist"
    na = t + 1 if t < max_len else t
    assert np.array_equal(TG._host(ses, "anc", (N, max_len + 1))[:, :na], host["anc"][:, :na]), what + ": anc"
    fs, fr, fsc = TG._host(ses, "fin_step", (B, beam)), TG._host(ses, "fin_row", (B, beam)), TG._host(ses, "fin_score", (B, beam))
    for s in range(B):
        k = int(host["nfin"][s])
        got = (fs[s, :k].tolist(), fr[s, :k].tolist(), fsc[s, :k].view(np.int32).tolist())
        assert got == (host["fin_step"][s, :k].tolist(), host["fin_row"][s, :k].tolist(),
                       host["fin_score"][s, :k].view(np.int32).tolist()), "%s: finalisation records of sentence %d" % (what, s)


def run_ensemble_search(c, wrong=()):
    """the whole search, one checked step at a time.  Returns (bans, forced rows, {wrong mode: steps at which the candidate check
    rejected that wrong reference})"""
    from fbk_fairseq_st_amd import lib as L
    engs, ses, init = _session(c)
    dtype, B, beam, V, max_len, min_len = c["dtype"], c["B"], c["beam"], c["V"], c["max_len"], c.get("min_len", 1)
    ngram, step0_all = c.get("n", 0), bool(c.get("init", False))
    prefix = np.asarray(c["prefix"], dtype=np.int64) if c.get("prefix") is not None else None
    n, N, K2 = len(engs), B * beam, 2 * beam
    lib, st = L.load(), L.stream()
    Wr = [e.ref_weights() for e in engs]
    refs, caches, tables, scales = [], [], [], []
    for j, (e, m) in enumerate(zip(engs, c["members"])):
        d = ses.members[j].desc
        refs.append(R.StepRef(Wr[j], e.cfg, dtype, [k.view(m["Ts"], B, -1) for k in e.kv], m["klen"][:B] if m["klen"] else None, beam,
                              d.ffn_slices, float(np.float32(1e-5))))
        caches.append([ses.bufs_of[j]["cache%d" % l] for l in range(m["layers"])])
        tables.append(e.table(PAD + 3 + max_len, PAD))
        scales.append(float(np.float32(m["D"] ** 0.5)))
    rules_addr = ses.rules_addr
    assert bool(rules_addr) == bool(ngram or prefix is not None)
    L.check(lib.s2t_decode_begin_ensemble(ses.descs_addr, n, BOS, st), "s2t_decode_begin_ensemble")
    host = R.new_state(B, beam, max_len, BOS)
    anc = torch.zeros((N, max_len + 1), dtype=torch.long, device=DEV)
    tokens = torch.full((N,), BOS, dtype=torch.long, device=DEV)
    bans = forced = 0
    rejected = {m: 0 for m in wrong}
    for t in range(max_len + 1):
        what = "%s step %d" % (c["id"], t)
        x0s = [ses.bufs_of[j]["x0"].clone() for j in range(n)]
        for j in range(n):
            xr, xb = R.next_input(Wr[j], PAD, tokens, PAD + 1 + t, tables[j], scales[j])
            TG._check_close(x0s[j], xr, R.SAFETY * xb, "x0", dtype, what + ": x0 of member %d" % j)
        L.check(lib.s2t_decode_step_ensemble(ses.descs_addr, n, rules_addr, st), "s2t_decode_step_ensemble")
        torch.cuda.synchronize()
        # 1. every member's decoder step, from its own x0 and its own cache along the SHARED ancestry
        for j in range(n):
            r = refs[j].step(x0s[j], t, anc, caches[j])
            for l, (kv, ekv) in enumerate(r["kv"]):
                TG._check_close(caches[j][l][t], kv, ekv, "kv", dtype, what + ": member %d K/V cache row of layer %d" % (j, l))
            TG._check_close(ses.bufs_of[j]["xn"], *r["xn"], "xn", dtype, what + ": member %d xn" % j)
            TG._check_close(ses.bufs_of[j]["logits"], *r["logits"], "logits", dtype, what + ": member %d logits" % j)
        # 2. the rows' candidates, on the members' own logits
        base = torch.from_numpy(host["cum_hist"][t].astype(np.float64)).to(DEV) if t > 0 else \
            (init.double() if init is not None else torch.zeros(N, dtype=torch.float64, device=DEV))
        logits = [ses.bufs_of[j]["logits"] for j in range(n)]
        args = (t, beam, PAD, UNK, EOS, max_len, min_len, 1.0, 0.0, base, step0_all, host["tok_hist"], host["par_hist"])
        rv, rb = ER.row_reference_ensemble(logits, *args, ngram=ngram, prefix=prefix)
        cv, ci = ses.view_f("cand_val").view(N, K2), ses.view_i("cand_idx").view(N, K2)
        TG._note("ens_rows", dtype, R.check_row_candidates(cv, ci, rv, rb, what + ": candidates"))
        if ngram or prefix is not None:
            plain, _ = ER.row_reference_ensemble(logits, *args)
            live = torch.isfinite(plain).any(1)
            if prefix is None or t >= prefix.shape[1]:
                bans += int((torch.isfinite(plain) & torch.isneginf(rv)).sum())
            else:
                forced += sum(int(prefix[r_ // beam][t] != PAD) for r_ in range(N) if bool(live[r_]))
        for mode in wrong:
            wv, wb = ER.row_reference_ensemble(logits, *args, ngram=ngram, prefix=prefix, mode=mode)
            try:
                R.check_row_candidates(cv, ci, wv, wb, what)
            except AssertionError:
                rejected[mode] += 1
        # 3. the bookkeeping, bit for bit
        R.sent_step(host, cv.cpu().numpy(), ci.cpu().numpy(), beam, V, EOS, max_len, step0_all)
        _check_bookkeeping(ses, host, t, B, beam, max_len, what)
        par = torch.from_numpy(host["par_hist"][t + 1].astype(np.int64)).to(DEV)
        tokens = torch.from_numpy(host["tok_hist"][t + 1].astype(np.int64)).to(DEV)
        if t < max_len:
            nxt = anc.clone()
            nxt[:, :t] = anc[par, :t]
            nxt[:, t] = par
            anc = nxt
    return bans, forced, rejected


def C(id_, dtype, members, B, beam, V, max_len, min_len=1, **kw):
    c = dict(id=id_, dtype=dtype, members=members, B=B, beam=beam, V=V, max_len=max_len, min_len=min_len)
    c.update(kw)
    return c


HETERO_F32 = C("f32-pair-b4-V200", F32, PAIR, 3, 4, 200, 16, 4)
CASES = [
    HETERO_F32,
    C("bf16-pair-b5-V5000", BF, PAIR, 3, 5, 5000, 16, 4),                                     # 20 columns per thread; bf16 members
    C("f32-three-b16", F32, [M(256), M(512, 1, 200), M(256, 2, 130, klen=[130, 5])], 2, 16, 200, 8, 2),      # 16-row tiles, three members
    C("f32-eight-b2-V96", F32, [M(256, 1, 100 + 28 * (j % 2)) for j in range(8)], 1, 2, 96, 6),             # the limit of eight
    C("f32-pair-n2-prefix3", F32, PAIR, 3, 4, 200, 16, 4, n=2, prefix=P3),                    # the rules on the combined row
    C("f32-pair-hierarchical", F32, PAIR, 3, 4, 200, 10, 3, init=True),                       # step0_all_slots + init_scores
]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_ensemble_step_by_step(c):
    bans, forced, _ = run_ensemble_search(c)
    if c.get("n"):
        assert bans > 0, "no step of the case banned a column that was open"
    if c.get("prefix") is not None:
        assert forced > 0, "no live row was forced"


def test_candidate_check_rejects_wrong_combinations():
    """the check of step 2 can fail: a reference without member 1, one without the - log n term and one that averages the members'
    log-probabilities are each rejected (the search itself still passes against the right reference)"""
    _, _, rejected = run_ensemble_search(dict(HETERO_F32, id="f32-pair-wrong-refs"), wrong=("drop1", "nolog", "meanlog"))
    for mode, steps in rejected.items():
        assert steps > 0, "the candidate check accepted the wrong reference %r at every step" % mode


def _written(ses, steps):
    """what `steps` steps of a search wrote, as bytes: the hypotheses walk_records rebuilds and the flags (test_decode_gpu._records), and
    the selection records of arrangements 0 .. steps (the rest of the state's buffers was never written: torch.empty)"""
    N, M2 = ses.N, ses.max_len + 2
    rows = min(steps, ses.max_len + 1) + 1
    hist = [TG._host(ses, k, (M2, N))[lo:rows].view(np.int32).tobytes() for k, lo in (("tok_hist", 0), ("par_hist", 1), ("cum_hist", 1))]
    return TG._records(ses), hist, TG._host(ses, "steps").tolist(), TG._host(ses, "blacklist").tolist()


def test_one_member_through_the_ensemble_calls_equals_step_rules():
    """n == 1: s2t_decode_begin_ensemble / s2t_decode_step_ensemble leave the records of s2t_decode_begin / s2t_decode_step_rules bit for bit
    (they launch the same kernels), with and without rules"""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd import lib as L
    lib = L.load()
    for ngram, prefix in ((0, None), (2, [[17, 45], [33, PAD], [PAD, PAD]])):
        out = []
        for ens in (False, True):
            torch.manual_seed(3)
            eng = TG.DecEngine(256, 512, 1, 200, F32, 3, "relu", 3.0, 1.0, 0)
            enc = torch.randn(100, 3, 256, device=DEV)
            pt = None if prefix is None else torch.tensor(prefix, dtype=torch.int64)
            ses = DEC.EnsembleDecodeSession([(eng, "decoder.", enc, None)], 4, 20, 3, PAD, UNK, EOS, 200, no_repeat_ngram_size=ngram,
                                            prefix_tokens=pt)
            assert ses.ok and ses.launches_per_step == 3 + 4
            st = L.stream()
            one = ses.members[0].addr
            if ens:
                L.check(lib.s2t_decode_begin_ensemble(ses.descs_addr, 1, BOS, st), "s2t_decode_begin_ensemble")
            else:
                L.check(lib.s2t_decode_begin(one, BOS, st), "s2t_decode_begin")
            for _ in range(21):
                if ens:
                    L.check(lib.s2t_decode_step_ensemble(ses.descs_addr, 1, ses.rules_addr, st), "s2t_decode_step_ensemble")
                else:
                    L.check(lib.s2t_decode_step_rules(one, ses.rules_addr, st), "s2t_decode_step_rules")
            torch.cuda.synchronize()
            out.append(_written(ses, 21))
        assert out[0] == out[1]
        assert all(out[0][0][2]), "every sentence finishes by max_len"


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_ensemble_graph_replay_equals_step_launches(dtype):
    """the heterogeneous pair: run(graph=True) (one recorded 8-step hipGraph, replayed) leaves the records of run(graph=False) bit for bit"""
    from fbk_fairseq_st_amd import decode as DEC
    assert DEC.POLL_STEPS == 8
    c = C("graph", dtype, PAIR, 3, 4, 200, 16, 4)
    out = []
    for graph in (False, True):
        _, ses, _ = _session(c)
        steps = ses.run(BOS, graph=graph)
        torch.cuda.synchronize()
        out.append((steps, _written(ses, steps)))
    assert out[0] == out[1]
    assert all(out[1][1][0][2]), "every sentence finishes by max_len"


# ------------------------------------------------------------------ whole searches
LENGTHS = [400, 250, 90]
OPTS = dict(beam_size=5, max_len_a=0.0, max_len_b=14, min_len=4, len_penalty=1.0, unk_penalty=0.0, temperature=1.0)
_CACHE = {}


def _models(dtype, seeds=(11, 12), **over):
    """s2t_transformer_s as test_configs_gpu builds it, once per (dtype, seeds): models that share the dictionaries, with different weights"""
    import test_configs_gpu as TC
    key = (dtype, seeds, tuple(sorted(over.items())))
    if key not in _CACHE:
        out = []
        for seed in seeds:
            a, task, model, crit, cfg, W = TC.build("s2t_transformer_s", dtype, criterion="label_smoothed_cross_entropy", seed=seed, **over)
            model.eval()
            out.append((task, model, cfg, W))
        _CACHE[key] = out
    return _CACHE[key]


def _net():
    import test_configs_gpu as TC
    if "net" not in _CACHE:
        task = _models(F32)[0][0]
        sample = TC.batch(task, len(LENGTHS), max(LENGTHS), 8, 8, 9, lengths=LENGTHS)
        _CACHE["net"] = (sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"])
    src, lens = _CACHE["net"]
    return src, lens, dict(net_input=dict(src_tokens=src.to(DEV), src_lengths=lens.to(DEV)))


def _formula(models):
    return sum(3 * m.hp.dec_layers + 2 for m in models) + 2


def test_ensemble_search_fp32_device_route_equals_step_route_and_oracle(monkeypatch):
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    from oracle import s2t_ref
    built = _models(F32)
    task, models = built[0][0], [b[1] for b in built]
    src, lens, net = _net()
    gen = SequenceGenerator(models, task.target_dictionary, **OPTS)
    dev_h = gen.generate(models, net)
    assert "launches_per_step" in gen.last_stats, "the device route was not taken"
    assert gen.last_stats["launches_per_step"] == _formula(models) == 42
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen2 = SequenceGenerator(models, task.target_dictionary, **OPTS)
    step_h = gen2.generate(models, net)
    assert "launches_per_step" not in gen2.last_stats, "the step route was not taken"
    orc = s2t_ref.beam_search([b[3] for b in built], built[0][2], src, lens, 5, 0.0, 14, 4, 1.0, 0.0, 1.0)
    assert len(dev_h) == len(step_h) == len(orc) == len(LENGTHS)
    for hs, ss, os_ in zip(dev_h, step_h, orc):
        assert len(hs) == len(ss) == len(os_) == 5
        for h, s_, (ot, osc, ops) in zip(hs, ss, os_):
            assert h["tokens"].tolist() == s_["tokens"].tolist() == ot.tolist()
            assert abs(float(h["score"]) - float(s_["score"])) < 1e-4 and abs(float(h["score"]) - osc) < 1e-4
            np.testing.assert_allclose(h["positional_scores"].cpu().numpy(), s_["positional_scores"].cpu().numpy(), atol=1e-4)
            np.testing.assert_allclose(h["positional_scores"].cpu().numpy(), ops, atol=1e-4)


def _repeats(tokens, n):
    g = [EOS] + list(tokens)                                   # <bos> = EOS heads the history
    grams = [tuple(g[i:i + n]) for i in range(len(g) - n + 1)]
    return len(grams) != len(set(grams))


@pytest.mark.parametrize("rules", [False, True], ids=["plain", "ngram3-prefix2"])
def test_ensemble_search_bf16(rules, monkeypatch):
    """bf16 (the two routes round differently): well-formed hypotheses whose best scores agree to BF16_GEN_ATOL; with n-gram size 3 and a
    two-token prefix every hypothesis starts with its sentence's forced tokens and repeats no trigram"""
    import test_configs_gpu as TC
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    built = _models(BF)
    task, models = built[0][0], [b[1] for b in built]
    _, _, net = _net()
    P2 = [[17, 45], [33, PAD], [PAD, PAD]]
    kw = dict(no_repeat_ngram_size=3) if rules else {}
    prefix = torch.tensor(P2, dtype=torch.int64, device=DEV) if rules else None
    gen = SequenceGenerator(models, task.target_dictionary, **OPTS, **kw)
    dev_h = gen.generate(models, net, prefix_tokens=prefix)
    assert gen.last_stats.get("launches_per_step") == _formula(models), "the device route was not taken"
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen2 = SequenceGenerator(models, task.target_dictionary, **OPTS, **kw)
    step_h = gen2.generate(models, net, prefix_tokens=prefix)
    assert "launches_per_step" not in gen2.last_stats
    assert len(dev_h) == len(step_h) == len(LENGTHS)
    for b, (hs, ss) in enumerate(zip(dev_h, step_h)):
        assert len(hs) == len(ss) == 5
        sc = [float(h["score"]) for h in hs]
        assert sc == sorted(sc, reverse=True)
        for h in hs:
            toks = h["tokens"].tolist()
            assert toks[-1] == EOS and EOS not in toks[:-1]
            if rules:
                forced = [v for v in P2[b] if v != PAD]
                assert toks[:len(forced)] == forced, "sentence %d: %s does not start with its forced tokens" % (b, toks)
                assert not _repeats(toks, 3), "sentence %d: a repeated trigram in %s" % (b, toks)
        assert abs(sc[0] - float(ss[0]["score"])) < TC.BF16_GEN_ATOL


@pytest.mark.parametrize("what", ["heads32_member", "print_alignment", "mixed_dtypes"])
def test_ensembles_the_device_route_leaves_to_the_step_route(what, monkeypatch):
    """an ensemble with one member of 32-wide heads, one that returns alignments and one whose members differ in compute dtype take the
    step route -- no session runs -- and give the step route's hypotheses"""
    from fbk_fairseq_st_amd import decode as DEC
    from fbk_fairseq_st_amd.sequence_generator import SequenceGenerator
    a_, b_ = _models(F32)
    task = a_[0]
    if what == "heads32_member":
        other = _models(F32, seeds=(12,), encoder_attention_heads=8, decoder_attention_heads=8)[0][1]
        assert other.hp.D // other.hp.heads == 32
    elif what == "mixed_dtypes":
        other = _models(BF)[1][1]
    else:
        other = b_[1]
    models = [a_[1], other]
    _, _, net = _net()
    opts = dict(OPTS, max_len_b=8, print_alignment=(what == "print_alignment"))

    def no_run(self, *a, **k):
        raise RuntimeError("a device session ran for a search the device route does not handle")
    monkeypatch.setattr(DEC.EnsembleDecodeSession, "run", no_run)
    gen = SequenceGenerator(models, task.target_dictionary, **opts)
    hyps = gen.generate(models, net)
    assert "launches_per_step" not in gen.last_stats
    monkeypatch.setenv("S2T_DEVICE_SEARCH", "0")
    gen2 = SequenceGenerator(models, task.target_dictionary, **opts)
    step_h = gen2.generate(models, net)
    assert len(hyps) == len(step_h) == len(LENGTHS)
    for hs, ss in zip(hyps, step_h):
        assert len(hs) == len(ss) == 5
        for h, s_ in zip(hs, ss):
            assert h["tokens"].tolist() == s_["tokens"].tolist() and float(h["score"]) == float(s_["score"])
            assert (h["alignment"] is not None) == (what == "print_alignment")
