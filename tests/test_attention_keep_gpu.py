"""The dropout keep-bit record of the second-generation attention kernels (include/s2t_hip.h: s2t_attn_keep_bytes, s2t_attn_fwd_keep,
s2t_attn_bwd_keep; csrc/attention.hip: the KEEP instantiations of attn_fwd2_kernel, attn_bwd_dq2_kernel, attn_bwd_dkv2_kernel).

The forward writes the keep decision of every (query, key) pair its hash produced, the two backward kernels test those bits where
s2t_attn_bwd hashes again.  The decisions are the same, so everything is held to EQUALITY with the hashing entry points:
  1. s2t_attn_fwd_keep: O and LSE torch.equal to s2t_attn_fwd;
  2. s2t_attn_bwd_keep, fed that record: dQ, dK, dV torch.equal to s2t_attn_bwd;
  3. the record, decoded by `decode` below (the header's layout restated once), equals on the valid positions (query < Tq,
     key < klen) the mask tests/test_dropout_parity_gpu.py rebuilds for an attention site (s2t_dropout on the padded index space);
  4. the backward reads the record and does not hash: an all-ones record gives the gradients of "nothing dropped, probabilities
     scaled by 1 / (1 - p)" (float64 autograd; bound 3e-2 of max(1, max |ref|), the bf16 backward bound of
     tests/test_kernels_gpu.py::test_attention_fwd_bwd), which are not the hashing backward's; an all-zeros record gives dV = 0 exactly
     where the second-generation dK/dV kernel runs (Tk >= 128);
  5. s2t_attn_keep_bytes is 0 for causal, distance-penalty, d = 32, p = 0, p < 2^-16 and short-query calls; the _keep entry points
     with a NULL record are the old entry points; with a record they refuse (S2T_ENOTSUP) a call that would not write it;
  6. one encoder-shaped layer call (T 130, B 2, D 512, training) against the per-kernel schedule with the assertions of
     tests/test_engine_gpu.py, and s2t_layer_ws_bytes grows by exactly the record.

Shapes (d = 64, bf16, a seed of its own per case): the smallest at which the indexing can go wrong.
  B 1, H 3, 130 x 130   B H & 7 != 0: no XCD remap; partial last query block and key tile; the second dK/dV workgroup's second key tile
                        does not exist (clamped)
  B 2, H 4, 200 x 70    B H = 8: the remap; Tk just over one tile; below 128 keys dK/dV runs the first generation, which hashes, next
                        to a dQ kernel that reads the record (check 4 can hold dQ alone to the all-ones record here, and at 128 x 64)
  B 2, H 8, 375 x 375   klen [375, 301]: the bench's tile counts; keys (and a whole key tile) past klen, which the forward never writes
  B 1, H 8, 64 x 64     one tile -- but 64 queries over 64 keys run the FIRST-generation kernels (the second generation takes
                        Tq >= 128, or Tq >= attn_v2_min_tq over Tk >= 128, and the short-query pair takes Tq <= 64 there), so
                        s2t_attn_keep_bytes is 0: the case holds the refusal and the NULL-record equality, and
  B 1, H 8, 128 x 64    is the one-tile case that does take the record: one query block, one key tile
The record buffers are filled with a bit pattern before every forward: what the forward leaves unwritten must not matter.
"""
import pytest
import torch

from fbk_fairseq_st_amd import kernels as K
from fbk_fairseq_st_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
D_HEAD = 64

#        id            B  H  Tq   Tk   klen          record expected
CASES = [("h3_130",    1, 3, 130, 130, None,         True),
         ("h4_200x70", 2, 4, 200, 70,  None,         True),
         ("h8_375",    2, 8, 375, 375, [375, 301],   True),
         ("h8_64",     1, 8, 64,  64,  None,         False),
         ("h8_128x64", 1, 8, 128, 64,  None,         True)]
RATES = [0.1, 0.5]
BWD_TOL = 3e-2                       # tests/test_kernels_gpu.py::test_attention_fwd_bwd, bf16


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1.0, float(b.abs().max())))


def decode(rec, B, H, Tq, Tk):
    """the record (int32 words) -> bool [B, H, 128 nq, 64 nk]; include/s2t_hip.h:
    word (((b H + h) nq + bx) nk + t) 256 + 64 w + 16 q + r16, bit 16 qb + 4 j + r = keep(query 128 bx + 32 w + 16 qb + r16, key 64 t + 16 j + 4 q + r)"""
    nq, nk = (Tq + 127) // 128, (Tk + 63) // 64
    w = rec.cpu().to(torch.int64).view(B * H, nq, nk, 4, 4, 16) & 0xFFFFFFFF               # [head, bx, t, w, q, r16]
    bits = ((w[..., None] >> torch.arange(32)) & 1).bool().view(B * H, nq, nk, 4, 4, 16, 2, 4, 4)   # ..., qb, j, r
    #  head bx w qb r16 | t j q r
    return bits.permute(0, 1, 3, 6, 5, 2, 7, 4, 8).reshape(B, H, nq * 128, nk * 64)


def hash_mask(p, seed, B, H, Tq, Tk):
    """the keep mask of an attention site as tests/test_dropout_parity_gpu.py rebuilds it from the engine's record"""
    from test_dropout_parity_gpu import site_mask
    return site_mask("x.self_attn.probs", p, seed, (B, H, Tq, Tk))


_cache = {}


def run_case(cid, p, seed_high=0):
    """inputs, both forwards and both backwards of a case, computed once and shared (nothing modifies them); `seed_high` goes into the
    upper word of the case's dropout seed"""
    key = (cid, p, seed_high)
    if key in _cache:
        return _cache[key]
    idx, (_, B, H, Tq, Tk, klen, has) = next((i, c) for i, c in enumerate(CASES) if c[0] == cid)
    seed = 1000 * (idx + 1) + int(100 * p)
    D = H * D_HEAD
    g = torch.Generator().manual_seed(seed)
    seed |= seed_high << 32
    qkv = torch.randn(max(Tq, Tk), B, 3 * D, generator=g).to(BF).to(DEV)
    q, k, v = qkv[:Tq, :, :D], qkv[:Tk, :, D:2 * D], qkv[:Tk, :, 2 * D:]
    do = torch.randn(Tq, B, D, generator=g).to(BF).to(DEV)
    kl = torch.tensor(klen, dtype=torch.int32, device=DEV) if klen else None
    nbytes = K.attn_keep_bytes(D_HEAD, B, H, Tq, Tk, p_drop=p)
    c = dict(B=B, H=H, Tq=Tq, Tk=Tk, D=D, klen=klen, kl=kl, p=p, seed=seed, q=q, k=k, v=v, do=do, nbytes=nbytes, has=has)
    c["o"], c["lse"] = K.attn_fwd(q, k, v, H, klen=kl, p_drop=p, seed=seed)

    def bwd(fn, o, *extra, **kw):
        dqkv = torch.zeros_like(qkv)
        fn(q, k, v, o, do, c["lse"], H, dqkv[:Tq, :, :D], dqkv[:Tk, :, D:2 * D], dqkv[:Tk, :, 2 * D:], *extra, klen=kl, p_drop=p, seed=seed, **kw)
        return dqkv[:Tq, :, :D], dqkv[:Tk, :, D:2 * D], dqkv[:Tk, :, 2 * D:]
    c["bwd"] = bwd
    c["grads"] = bwd(K.attn_bwd, c["o"])
    if nbytes:
        rec = torch.full((nbytes // 4,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        c["o_keep"], c["lse_keep"] = K.attn_fwd_keep(q, k, v, H, rec, klen=kl, p_drop=p, seed=seed)
        c["rec"] = rec
        c["grads_keep"] = bwd(K.attn_bwd_keep, c["o_keep"], rec)
    torch.cuda.synchronize()
    _cache[key] = c
    return c


IDS = [c[0] for c in CASES]
ON_ROUTE = [c[0] for c in CASES if c[6]]


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("cid", IDS)
def test_record_size_follows_the_route(cid, p):
    c = run_case(cid, p)
    nq, nk = (c["Tq"] + 127) // 128, (c["Tk"] + 63) // 64
    assert c["nbytes"] == (c["B"] * c["H"] * nq * nk * 256 * 4 if c["has"] else 0)


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("cid", ON_ROUTE)
def test_forward_with_a_record_equals_the_hashing_forward(cid, p):
    c = run_case(cid, p)
    assert torch.equal(c["o_keep"], c["o"]) and torch.equal(c["lse_keep"], c["lse"])
    o0, _ = K.attn_fwd(c["q"], c["k"], c["v"], c["H"], klen=c["kl"])
    assert rel_err(o0, c["o"]) > 1e-2, "the mask does nothing"


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("cid", ON_ROUTE)
def test_backward_from_the_record_equals_the_hashing_backward(cid, p):
    c = run_case(cid, p)
    for name, a, b in zip(("dQ", "dK", "dV"), c["grads_keep"], c["grads"]):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
        assert float(b.float().abs().max()) > 0, name


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("cid", ON_ROUTE)
def test_decoded_record_is_the_hash_mask(cid, p):
    c = run_case(cid, p)
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    got = decode(c["rec"], B, H, Tq, Tk)[:, :, :Tq, :Tk]
    want = hash_mask(p, c["seed"], B, H, Tq, Tk)
    valid = torch.zeros(B, 1, 1, Tk, dtype=torch.bool)
    for b in range(B):
        valid[b, :, :, :(c["klen"][b] if c["klen"] else Tk)] = True
    valid = valid.expand(B, H, Tq, Tk)
    n = int(valid.sum())
    frac = float(want[valid].float().mean())
    assert abs(frac - (1 - p)) < 6 * (p * (1 - p) / n) ** 0.5, frac           # a mask of that rate, not a constant
    bad = (got != want) & valid
    assert not bool(bad.any()), (int(bad.sum()), n, bad.nonzero()[:4].tolist())


def test_record_and_hashing_kernels_at_a_seed_above_32_bits():
    """case h8_128x64 with the upper word of the dropout seed set: the forward's record is still s2t_dropout's mask at that seed, and
    the hashing forward and backward (which take the upper word once per launch) still equal the record-reading ones bit for bit"""
    cid, p = "h8_128x64", 0.1
    c = run_case(cid, p, seed_high=5)
    assert c["seed"] >> 32 == 5 and c["nbytes"] > 0
    assert torch.equal(c["o_keep"], c["o"]) and torch.equal(c["lse_keep"], c["lse"])
    for name, a, b in zip(("dQ", "dK", "dV"), c["grads_keep"], c["grads"]):
        assert torch.equal(a, b), (name, float((a.float() - b.float()).abs().max()))
    B, H, Tq, Tk = c["B"], c["H"], c["Tq"], c["Tk"]
    got = decode(c["rec"], B, H, Tq, Tk)[:, :, :Tq, :Tk]
    want = hash_mask(p, c["seed"], B, H, Tq, Tk)
    assert not bool((got != want).any()), int((got != want).sum())
    assert bool((got != hash_mask(p, c["seed"] & 0xFFFFFFFF, B, H, Tq, Tk)).any()), "the seed's upper word does not reach the record"
    assert not torch.equal(c["o"], run_case(cid, p)["o"])


@pytest.mark.parametrize("p", RATES)
@pytest.mark.parametrize("cid", ON_ROUTE)
def test_backward_reads_the_record_and_does_not_hash(cid, p):
    c = run_case(cid, p)
    B, H, Tq, Tk, D = c["B"], c["H"], c["Tq"], c["Tk"], c["D"]
    # float64: O = softmax(S) V / (1 - p), nothing dropped
    q, k, v = [t.double().clone().requires_grad_(True) for t in (c["q"], c["k"], c["v"])]
    qh = q.view(Tq, B * H, D_HEAD).transpose(0, 1) * D_HEAD ** -0.5
    kh = k.reshape(Tk, B * H, D_HEAD).transpose(0, 1); vh = v.reshape(Tk, B * H, D_HEAD).transpose(0, 1)
    s = torch.bmm(qh, kh.transpose(1, 2)).view(B, H, Tq, Tk)
    if c["klen"]:
        m = torch.arange(Tk, device=DEV)[None, :] >= c["kl"][:, None]
        s = s.masked_fill(m[:, None, None, :], float("-inf"))
    o = (torch.bmm(torch.softmax(s, -1).view(B * H, Tq, Tk), vh) / (1 - p)).transpose(0, 1).reshape(Tq, B, D)
    o.backward(c["do"].double())
    # the kernels' Delta is rowsum(dO * O) of the O they are handed: the output of THAT forward
    ones = torch.full_like(c["rec"], -1)
    got = c["bwd"](K.attn_bwd_keep, o.detach().to(BF), ones)
    # below 128 keys dK / dV come from the first-generation kernel, which hashes whatever the record says (bwd_launch: dkv2 needs
    # Tk >= 128): there the record reaches dQ alone
    reads = ("dQ", "dK", "dV") if Tk >= 128 else ("dQ",)
    for name, a, ref in zip(reads, got, (q.grad, k.grad, v.grad)):
        e = rel_err(a, ref)
        print("%s p=%.1f %s all-ones record vs float64: %.3e (bound %.0e)" % (cid, p, name, e, BWD_TOL))
        assert e < BWD_TOL, (name, e)
    for name, a, b in zip(reads, got, c["grads"]):
        assert not torch.equal(a, b), name + ": the hashing backward's gradients from an all-ones record"
    if Tk >= 128:                                     # attn_bwd_dkv2_kernel: P * keep is all zeros
        zeros = torch.zeros_like(c["rec"])
        dv = c["bwd"](K.attn_bwd_keep, c["o"], zeros)[2]
        assert float(dv.float().abs().max()) == 0.0


def test_keep_bytes_is_zero_off_the_plain_path():
    ok = K.attn_keep_bytes(64, 2, 8, 375, 375, p_drop=0.1)
    assert ok == 2 * 8 * 3 * 6 * 256 * 4
    assert K.attn_keep_bytes(64, 2, 8, 375, 375, causal=True, p_drop=0.1) == 0
    assert K.attn_keep_bytes(64, 2, 8, 375, 375, dist_penalty=True, p_drop=0.1) == 0
    assert K.attn_keep_bytes(32, 2, 8, 375, 375, p_drop=0.1) == 0
    assert K.attn_keep_bytes(64, 2, 8, 375, 375, p_drop=0.0) == 0
    assert K.attn_keep_bytes(64, 2, 8, 375, 375, p_drop=2.0 ** -17) == 0          # a rate below 2^-16 drops nothing: no DROP tiles
    assert K.attn_keep_bytes(64, 2, 8, 375, 375, p_drop=2.0 ** -16) == ok
    assert K.attn_keep_bytes(64, 2, 8, 40, 368, p_drop=0.1) == 0                  # the short-query kernels (decoder encoder-attention)
    assert K.attn_keep_bytes(64, 2, 8, 64, 368, p_drop=0.1) == 0
    assert K.attn_keep_bytes(64, 2, 8, 65, 368, p_drop=0.1) == 2 * 8 * 1 * 6 * 256 * 4
    assert K.attn_keep_bytes(64, 2, 8, 100, 100, p_drop=0.1) == 0                 # first generation: below 128 queries and 128 keys
    old = K.set_option("attn_v1", 1)
    try:
        assert K.attn_keep_bytes(64, 2, 8, 375, 375, p_drop=0.1) == 0
    finally:
        K.set_option("attn_v1", old)


@pytest.mark.parametrize("cid", ["h3_130", "h8_64"])
def test_null_record_is_the_old_entry_point_and_a_useless_record_is_refused(cid):
    c = run_case(cid, 0.1)
    q, k, v, H, p, seed = c["q"], c["k"], c["v"], c["H"], c["p"], c["seed"]
    o, lse = K.attn_fwd_keep(q, k, v, H, None, klen=c["kl"], p_drop=p, seed=seed)
    assert torch.equal(o, c["o"]) and torch.equal(lse, c["lse"])
    for a, b in zip(c["bwd"](K.attn_bwd_keep, c["o"], None), c["grads"]):
        assert torch.equal(a, b)
    rec = torch.zeros(1 << 16, dtype=torch.int32, device=DEV)
    # h8_64 runs the first-generation kernels: no record at all; on the route, a causal call has none either
    with pytest.raises(L.S2THipError, match="not supported"):
        K.attn_fwd_keep(q, k, v, H, rec, klen=c["kl"], causal=c["has"], p_drop=p, seed=seed)
    with pytest.raises(L.S2THipError, match="not supported"):
        c["bwd"](K.attn_bwd_keep, c["o"], rec, causal=c["has"])
    if c["has"]:                                                           # a layout that leaves attn_fwd2_kernel: O 4 bytes off 8
        buf = torch.empty(c["Tq"] * c["B"] * c["D"] + 2, dtype=BF, device=DEV)
        o_off = buf[2:].view(c["Tq"], c["B"], c["D"])
        with pytest.raises(L.S2THipError, match="not supported"):
            K.attn_fwd_keep(q, k, v, H, rec, klen=c["kl"], p_drop=p, seed=seed, out=o_off)
        with pytest.raises(L.S2THipError, match="not supported"):
            K.attn_fwd_keep(q.float(), k.float(), v.float(), H, rec, klen=c["kl"], p_drop=p, seed=seed)


# ---- one encoder-shaped layer call
def build_engine():
    from fbk_fairseq_st_amd import conv_transformer, criterions, tasks  # noqa: F401
    from fbk_fairseq_st_amd.data import Dictionary
    from fbk_fairseq_st_amd.registry import apply_arch, namespace
    a = namespace(arch="conv_transformer", criterion="ctc_multi_loss", underlying_criterion="label_smoothed_cross_entropy", label_smoothing=0.1,
                  ctc_compress_out=True, ctc_encoder_layer=1, ctc_weight=1.0, encoder_embed_dim=512, encoder_ffn_embed_dim=1024,
                  encoder_attention_heads=8, encoder_layers=1, decoder_layers=1, decoder_embed_dim=512, decoder_ffn_embed_dim=1024,
                  decoder_attention_heads=8, no_attn_2d=True, input_feat_per_channel=80, dropout=0.1, attention_dropout=0.1, activation_dropout=0.1,
                  relu_dropout=0.1, activation_fn="relu", sentence_avg=False, seed=7)
    apply_arch(a)
    tgt, src = Dictionary.synthetic(300), Dictionary.synthetic(200)
    src.add_symbol("<ctc_blank>")
    task = tasks.SpeechTranslationCTCTask(a, tgt, src)
    torch.manual_seed(3)
    model, crit = task.build_model(a), task.build_criterion(a)
    model.materialize(DEV, BF, extra=crit.arena_params())
    model._ensure_engine(DEV)
    return model, model.engine


def test_layer_call_carries_the_record():
    """csrc/layer.hip with the record against the per-kernel schedule (which stays on the hashing entry points): forward bits,
    gradients to f32 rounding (tests/test_engine_gpu.py); the training workspace holds exactly the record more"""
    model, eng = build_engine()
    T, B, D, H = 130, 2, 512, 8
    assert eng.hp.D == D and eng.hp.heads == H and eng.composite
    pfx, s0 = "encoder.layers.0.", 11 * 1000 + 10
    g = torch.Generator().manual_seed(17)
    x = torch.randn(T, B, D, generator=g).to(BF).to(DEV)
    dy = torch.randn(T * B, D, generator=g).to(BF).to(DEV)
    klen = torch.tensor([T, 101], dtype=torch.int32, device=DEV)
    names = [n for n in model.arena.slices if n.startswith(pfx)]
    assert names

    def grads():
        eng.flush_wgrad()
        torch.cuda.synchronize()
        return {n: model.arena.g(n).clone() for n in names}
    # the per-kernel schedule
    model.arena.zero_grad()
    y1, ca = eng.self_attn_block_fwd(pfx, x, klen, False, True, s0, dist_penalty=False)
    y0, cf = eng.ffn_block_fwd(pfx, y1, True, s0)
    dx0 = eng.self_attn_block_bwd(pfx, ca, eng.ffn_block_bwd(pfx, cf, dy))
    g0 = grads()
    # one call per direction
    model.arena.zero_grad()
    y, cl = eng.layer_fwd(pfx, x, True, (s0 + 1, s0 + 2, 0, 0, s0 + 3, s0 + 4), self_klen=klen, dist_penalty=False)
    dx1, _ = eng.layer_bwd(cl, dy, None, None)
    g1 = grads()
    assert torch.equal(y, y0)

    def close(a, b, n):
        assert torch.allclose(a.float(), b.float(), rtol=2e-5, atol=2e-6 * max(float(b.float().abs().max()), 1e-30)), n
    close(dx1, dx0, "dx")
    for n in names:
        assert float(g0[n].abs().max()) > 0, n
        close(g1[n], g0[n], n)
    # the workspace: the record and nothing else
    nrec = K.attn_keep_bytes(D // H, B, H, T, T, p_drop=eng.hp.attention_dropout)
    assert nrec == B * H * 2 * 3 * 256 * 4
    desc = eng._layer_desc(pfx, False, T, B, 0, False, False)["desc"]
    train, ev = K.layer_ws_bytes(desc, True), K.layer_ws_bytes(desc, False)
    pa = desc.p_attn
    try:
        desc.p_attn = 0.0
        train0, ev0 = K.layer_ws_bytes(desc, True), K.layer_ws_bytes(desc, False)
    finally:
        desc.p_attn = pa
    assert ev == ev0 and train - train0 == nrec
    mask = (K.relu_mask_bytes(T * B, eng.hp.ffn, D) + 255) // 256 * 256
    assert train - ev == mask + nrec
    assert cl["ws"].numel() == train
