"""Float64 references of the device-resident beam search (fbk_fairseq_st_amd/decode.py, csrc/decode.hip), one decoding step at a time.

Three independent pieces, each conditioned on the device's own history so that no check depends on which of two near-tied candidates
won a selection:

* `StepRef`: the decoder step (self-attention over the cached positions, encoder attention, feed-forward, final LayerNorm, output
  projection) in float64 from the step's f32 input `x0`, the K/V rows the device cached at earlier positions (gathered along the
  ancestry the test derives from `par_hist`, not from the device's `anc`) and the same weights.  Every value the kernels round to the
  compute dtype T is rounded here too: LayerNorm outputs, the K/V rows, the attention outputs, the per-head / per-slice shares,
  `xn`, the encoder-attention probabilities, and in bf16 the packed query of the self-attention scores and the packed probabilities
  of its paired-position P.V (beam <= 8).
  The comparisons allow a fraction of the compared magnitudes, TOL[dtype] of |v| + mean |v| over the row for xn and the K/V rows,
  LOGIT_SHARE times that of |xn| . |W| for a logit.  These allowances are MEASURED, not derived: a worst-case running error bound
  grows by about sqrt(D) per product and exponentially through the attention softmax, and already past the first block it bounds
  nothing useful, in bf16 as soon as one value may round to the neighbouring bf16 number.  What is left in the device-reference
  difference is rounding of this kind (two bf16 steps at most where it shows, in the measurements; f32-level otherwise); the test
  prints the worst error / allowance ratio of every check, and tests/test_decode_gpu.py lists the decode.hip mutations these
  allowances were shown to catch.
* `row_reference`: dec_row_kernel's arithmetic (log-softmax with temperature, the pad / unk / min-len / max-len rules, + cumulative
  score or init score) in float64 on the device's f32 logits, with its f32 error bound (derived: see the function).
* `sent_step`: dec_sent_kernel's bookkeeping restated on host arrays (merge of the rows' candidate lists, EOS finalisation,
  black-listing, next beam, ancestors, `finished`), bit for bit; tests/test_decode_host_cpu.py pins it to oracle/s2t_ref.py's search.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
SAFETY = 2.0
TOL = {torch.bfloat16: 2.0 ** -6, torch.float32: 2.0 ** -18}
LOGIT_SHARE = 0.125                  # a logit sums D products: its allowance is an eighth of the sum of their magnitudes
DH = 64
NTHREADS = 256


def layer_norm(v, g, b, eps):
    """fairseq LayerNorm over the last axis (biased variance, eps inside the root)"""
    c = v - v.mean(-1, keepdim=True)
    return c * ((c * c).mean(-1, keepdim=True) + eps).rsqrt() * g + b


# ------------------------------------------------------------------ the decoder step
class StepRef:
    """One decoding step of the whole batch in float64, rounded where the kernels round (module docstring).

    W: float64 tensors on the device, every weight matrix already rounded to the compute dtype (what the session packs), LayerNorm
    parameters and biases as the f32 values the kernels read.  kv_enc[l]: [Ts, B, 2D] encoder keys | values of layer l as the
    session holds them (compute dtype); klen: int list or None; eps: the f32 LayerNorm epsilon the kernels read."""

    def __init__(self, W, cfg, dtype, kv_enc, klen, beam, ffn_slices, eps):
        self.W, self.cfg, self.dtype, self.beam, self.FS, self.eps = W, cfg, dtype, beam, ffn_slices, eps
        self.D, self.H, self.L = cfg["D"], cfg["heads"], cfg["dec_layers"]
        self.kv_enc = [k.double() for k in kv_enc]
        self.Ts, self.B = kv_enc[0].shape[0], kv_enc[0].shape[1]
        self.klen = klen
        self.gelu = cfg["act"] == "gelu"
        # the self-attention P.V of the bf16 kernels packs the probabilities to bf16 where it pairs positions (RT <= 8: PU even)
        self.pack_p = dtype == torch.bfloat16 and beam <= 8

    def rd(self, y):
        return y.to(self.dtype).double()

    def _mask_cross(self, dev):
        Ts = self.Ts
        lim = torch.tensor([min(int(k), Ts) for k in self.klen] if self.klen is not None else [Ts] * self.B, device=dev)
        lim = lim.repeat_interleave(self.beam)
        return (torch.arange(Ts, device=dev)[None, :] < lim[:, None])[:, None, :]          # [N, 1, Ts]

    def _shares(self, o, w, parts, width):
        """per head (slice) products o_j [N, width] @ w[:, j width:(j+1) width]^T, each rounded to T: [parts, N, D]"""
        return torch.stack([self.rd(o[:, j] @ w[:, j * width:(j + 1) * width].t()) for j in range(parts)])

    def step(self, x0, t, anc, caches):
        """x0 [N, D] (the device's f32 step input), t = step index, anc LongTensor [N, >= t] (cache row of each position < t),
        caches[l] = the device's [max_len + 1, N, 2D] K/V cache of layer l.  Returns a dict of (value, allowance) pairs: "kv" (one
        per layer), "xn", "logits"."""
        W, D, H, N, eps, rd = self.W, self.D, self.H, x0.shape[0], self.eps, self.rd
        dev = x0.device
        x = x0.double()
        kvs = []
        rows = torch.arange(N, device=dev)
        for l in range(self.L):
            p = "decoder.layers.%d." % l
            # ---- self-attention (dec_self_kernel)
            a = rd(layer_norm(x, W[p + "self_attn_layer_norm.weight"], W[p + "self_attn_layer_norm.bias"], eps))
            qkv = a @ W[p + "self_attn.qkv.weight"].t() + W[p + "self_attn.qkv.bias"]
            q = qkv[:, :D] * 0.125
            if self.dtype == torch.bfloat16:
                q = rd(q)                                               # the packed bf16 query of the v_dot2 score loop
            kt, vt = rd(qkv[:, D:2 * D]), rd(qkv[:, 2 * D:])
            kvs.append(torch.cat([kt, vt], 1))
            if t > 0:
                old = caches[l][torch.arange(t, device=dev)[None, :], anc[:, :t]].double()      # [N, t, 2D]
                K, V = torch.cat([old[:, :, :D], kt[:, None]], 1), torch.cat([old[:, :, D:], vt[:, None]], 1)
            else:
                K, V = kt[:, None], vt[:, None]
            n = t + 1
            s = torch.einsum("nhd,nphd->nhp", q.view(N, H, DH), K.reshape(N, n, H, DH))
            pr = torch.softmax(s, -1)
            if self.pack_p:
                pr = rd(pr)
            o = rd(torch.einsum("nhp,nphd->nhd", pr, V.reshape(N, n, H, DH)))
            x = x + W[p + "self_attn.out_proj.bias"] + self._shares(o, W[p + "self_attn.out_proj.weight"], H, DH).sum(0)
            # ---- encoder attention (dec_cross_kernel)
            a = rd(layer_norm(x, W[p + "encoder_attn_layer_norm.weight"], W[p + "encoder_attn_layer_norm.bias"], eps))
            q = rd((a @ W[p + "encoder_attn.q_proj.weight"].t() + W[p + "encoder_attn.q_proj.bias"]) * 0.125)
            kv = self.kv_enc[l]                                          # [Ts, B, 2D]
            sent = rows // self.beam
            Ke = kv[:, sent, :D].permute(1, 0, 2).reshape(N, self.Ts, H, DH)
            Ve = kv[:, sent, D:].permute(1, 0, 2).reshape(N, self.Ts, H, DH)
            s = torch.einsum("nhd,nphd->nhp", q.view(N, H, DH), Ke).masked_fill(~self._mask_cross(dev), -math.inf)
            pr = rd(torch.softmax(s, -1))
            o = rd(torch.einsum("nhp,nphd->nhd", pr, Ve))
            x = x + W[p + "encoder_attn.out_proj.bias"] + self._shares(o, W[p + "encoder_attn.out_proj.weight"], H, DH).sum(0)
            # ---- feed-forward (dec_ffn_kernel)
            a = rd(layer_norm(x, W[p + "final_layer_norm.weight"], W[p + "final_layer_norm.bias"], eps))
            h = a @ W[p + "fc1.weight"].t() + W[p + "fc1.bias"]
            h = rd(0.5 * h * (1.0 + torch.erf(h * 0.7071067811865476)) if self.gelu else h.clamp_min(0.0))
            hs = self.cfg["ffn"] // self.FS
            x = x + W[p + "fc2.bias"] + self._shares(h.view(N, self.FS, hs), W[p + "fc2.weight"], self.FS, hs).sum(0)
        # ---- final LayerNorm (dec_final_kernel) and the output projection (dec_logits_kernel)
        xn = rd(layer_norm(x, W["decoder.layer_norm.weight"], W["decoder.layer_norm.bias"], eps))
        w_out = W["decoder.output_projection.weight"]
        tol = TOL[self.dtype]
        row = lambda v: (v.abs() + v.abs().mean(-1, keepdim=True)) * tol
        return {"kv": [(v, row(v)) for v in kvs], "xn": (xn, row(xn)),
                "logits": (xn @ w_out.t(), tol * LOGIT_SHARE * (xn.abs() @ w_out.abs().t()))}


def next_input(W, pad, tokens, pos_row, pos_table, embed_scale):
    """a step's x0 = embed_scale * E[token] + position row `pos_row` (pad's own row for pad), float64, and its f32 bound"""
    e = W["decoder.embed_tokens.weight"][tokens]
    rows = torch.where(tokens == pad, torch.full_like(tokens, pad), torch.full_like(tokens, pos_row))
    pe = pos_table[rows].double()
    return embed_scale * e + pe, 2 * U * ((embed_scale * e).abs() + pe.abs())


# ------------------------------------------------------------------ dec_row_kernel
def row_reference(logits, t, beam, pad, unk, eos, max_len, min_len, it, unk_penalty, base, step0_all):
    """float64 [N, V] candidate values of every column (the kernel keeps the 2 beam best) and their f32 bound.
    logits: the device's f32 [N, V]; it, unk_penalty: the f32 values the kernel reads; base [N] float64 (cum score or init score).
    Bound: the product x it (u), the sum of V exponentials (depth ceil(V / 256) + 19, as in tests/test_loss_rows_gpu.py), logf
    (4 ulp) and the f32 additions / subtractions after it (u each), doubled."""
    x = logits.double()
    N, V = x.shape
    val = x * it
    lse = torch.logsumexp(val, -1, keepdim=True)
    lp = val - lse
    lp = torch.where(torch.isnan(lp), torch.full_like(lp, -math.inf), lp)
    cols = torch.arange(V, device=x.device)
    lp[:, pad] = -math.inf
    lp[:, unk] = lp[:, unk] - unk_penalty
    if t >= max_len:
        lp = lp.masked_fill((cols != eos)[None, :], -math.inf)
    elif t < min_len:
        lp[:, eos] = -math.inf
    live = torch.ones(N, dtype=torch.bool, device=x.device) if (t > 0 or step0_all) else \
        (torch.arange(N, device=x.device) % beam == 0)
    res = lp + base[:, None]
    res = torch.where(live[:, None], res, torch.full_like(res, -math.inf))
    depth = (V + NTHREADS - 1) // NTHREADS + 19
    z = lambda a: a.nan_to_num(0.0, posinf=0.0, neginf=0.0)
    mag = val.abs() + lse.abs() + 2 * z(lp.abs()) + base.abs()[:, None] + abs(unk_penalty) + z(res.abs())
    bound = SAFETY * U * (mag + depth + 4 * lse.abs().clamp_min(1.0))
    return res, torch.where(torch.isfinite(res), bound, torch.zeros_like(bound))


def check_row_candidates(cand_val, cand_idx, ref, bound, what):
    """the 2 beam device candidates of every row against the float64 values of all columns: values within the bound of their
    column's reference; values non-increasing with exact ties in column order (bit for bit, -inf included); the set is the top
    2 beam up to near-ties (no column outside it beats the last one by more than the two bounds); -inf exactly where the reference
    has -inf, in the reference's tie order; among exact ties the lowest columns.  Returns the worst |err| / bound ratio."""
    N, K2 = cand_val.shape
    cv, ci = cand_val.double(), cand_idx.long()
    assert bool((ci >= 0).all()) and bool((ci < ref.shape[1]).all()), "%s: column out of range" % what
    rv = ref.gather(1, ci)
    rb = bound.gather(1, ci)
    ninf_d, ninf_r = torch.isneginf(cv), torch.isneginf(rv)
    assert bool((ninf_d == ninf_r).all()), "%s: -inf candidates differ in rows %s" % (
        what, torch.nonzero((ninf_d != ninf_r).any(1)).view(-1).tolist()[:8])
    err = (cv - rv).abs().masked_fill(ninf_d, 0.0)
    ratio = (err / rb.clamp_min(1e-300)).masked_fill(ninf_d, 0.0)
    worst = float(ratio.max())
    assert worst <= 1.0, "%s: %d candidate values out of bound, worst %.3gx" % (what, int((ratio > 1).sum()), worst)
    a, b = cv[:, :-1], cv[:, 1:]
    order_ok = (a > b) | ((a == b) & (ci[:, :-1] < ci[:, 1:]))
    assert bool(order_ok.all()), "%s: candidates out of order in rows %s" % (what, torch.nonzero(~order_ok.all(1)).view(-1).tolist()[:8])
    outside = torch.ones_like(ref, dtype=torch.bool)
    outside.scatter_(1, ci, False)
    beats = outside & (ref > rv[:, -1:] + rb[:, -1:] + bound)
    assert not bool(beats.any()), "%s: a column outside the candidates beats them in rows %s" % (
        what, torch.nonzero(beats.any(1)).view(-1).tolist()[:8])
    # exact ties (identical columns give bit-identical logits): a lower column tied with the last candidate must have been taken first
    tied_lower = outside & (ref == rv[:, -1:]) & torch.isfinite(ref) & (torch.arange(ref.shape[1], device=ref.device)[None, :] < ci[:, -1:])
    assert not bool(tied_lower.any()), "%s: a lower column tied with the last candidate was passed over in rows %s" % (
        what, torch.nonzero(tied_lower.any(1)).view(-1).tolist()[:8])
    for n in torch.nonzero(ninf_d.any(1)).view(-1).tolist():
        k0 = int((~ninf_d[n]).sum())
        free = torch.isneginf(ref[n])
        free[ci[n, :k0]] = False
        rest = torch.nonzero(free).view(-1)[:K2 - k0].tolist()
        assert ci[n, k0:].tolist() == rest, "%s: row %d -inf tail %s != %s" % (what, n, ci[n, k0:].tolist(), rest)
    return worst


# ------------------------------------------------------------------ dec_sent_kernel
def new_state(B, beam, max_len, bos):
    """host state after s2t_decode_begin: the fields dec_begin_kernel sets (the others are never read before they are written)"""
    N, M2 = B * beam, max_len + 2
    st = dict(tok_hist=np.zeros((M2, N), np.int32), par_hist=np.zeros((M2, N), np.int32), cum_hist=np.zeros((M2, N), np.float32),
              anc=np.zeros((N, max_len + 1), np.int32), blacklist=np.zeros(N, np.int32), nfin=np.zeros(B, np.int32),
              finished=np.zeros(B, np.int32), steps=np.zeros(B, np.int32), fin_step=np.zeros((B, beam), np.int32),
              fin_row=np.zeros((B, beam), np.int32), fin_score=np.zeros((B, beam), np.float32))
    st["tok_hist"][0, :] = bos
    return st


def sent_step(st, cand_val, cand_idx, beam, V, eos, max_len, step0_all):
    """One launch of dec_sent_kernel on host state `st` (new_state's arrays, modified in place).  cand_val [N, 2 beam] float32 /
    cand_idx int32: every row's candidate list, ordered (value descending, column ascending).  Semantics of fairseq's
    BeamSearch.step (search.py:55-83: top 2 beam of beam x V, only row 0 at the first step) and SequenceGenerator (:383-446:
    EOS among the first beam candidates finalise while the sentence has room, unless their slot is black-listed; the next beam
    is the non-EOS candidates in rank order, then the EOS ones, which black-list their slot), as oracle/s2t_ref.py restates them."""
    B = st["steps"].shape[0]
    K2 = 2 * beam
    for s in range(B):
        n0 = s * beam
        t = int(st["steps"][s])
        if t > max_len:
            continue
        first = t == 0 and not step0_all
        k = min(K2, (V if first else beam * V) - 1)
        rows = 1 if first else beam
        ent = [(float(cand_val[n0 + j, i]), j * V + int(cand_idx[n0 + j, i])) for j in range(rows) for i in range(K2)]
        ent.sort(key=lambda e: (-e[0], e[1]))
        ent = ent[:k]
        val = [np.float32(e[0]) for e in ent]
        tok = [e[1] % V for e in ent]
        row = [n0 + e[1] // V for e in ent]
        bl = [bool(st["blacklist"][n0 + i]) for i in range(beam)]
        done = bool(st["finished"][s])
        nf = int(st["nfin"][s])
        nb = min(beam, k)
        eosm = [tok[i] == eos and val[i] != -np.inf for i in range(k)]
        for i in range(nb):
            eosm[i] = eosm[i] and not bl[i]
        nm = 0
        for i in range(nb):
            if eosm[i] and not done:
                slot = nf + nm
                nm += 1
                if slot < beam:
                    st["fin_step"][s, slot], st["fin_row"][s, slot], st["fin_score"][s, slot] = t, row[i], val[i]
        nf_new = min(beam, nf + nm)
        st["nfin"][s] = nf_new
        if nm and (nf_new == beam or t == max_len):
            st["finished"][s] = 1
        for i in range(nb):
            eosm[i] = eosm[i] or bl[i]
        pick = ([i for i in range(k) if not eosm[i]] + [i for i in range(k) if eosm[i]])[:beam]
        for place, i in enumerate(pick):
            st["tok_hist"][t + 1, n0 + place] = tok[i]
            st["par_hist"][t + 1, n0 + place] = row[i]
            st["cum_hist"][t + 1, n0 + place] = val[i]
            st["blacklist"][n0 + place] = 1 if eosm[i] else 0
        if t < max_len:
            old = st["anc"][n0:n0 + beam, :t].copy()
            for j, i in enumerate(pick):
                st["anc"][n0 + j, :t] = old[row[i] - n0]
                st["anc"][n0 + j, t] = row[i]
        st["steps"][s] = t + 1
