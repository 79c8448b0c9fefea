"""Float64 restatement of the ensemble row of the device search (csrc/decode.hip, dec_row_kernel<VPT, true, true>).

From every member's device f32 logits: each member's log-softmax with temperature, the log of the members' mean probability per
column (fairseq/sequence_generator.py:757-768: logsumexp over the members - log n), then the rules exactly as
decode_ref.row_reference applies them (NaN -> -inf, pad, unk penalty, max_len / min_len, the live slots of step 0, + the cumulative
or initial score) and the prefix / n-gram rules through decode_rules_ref.history and banned_columns, as
decode_rules_ref.row_reference_rules applies them.

The f32 bound is derived by counting the kernel's operations, in units of U = 2^-24 and doubled (SAFETY), as row_reference documents
for its own; it is not fitted to any output:
  member j's log-probability lp_j = x_j * it - lse_j: the product (|x_j it|), the sum of V exponentials (depth ceil(V / 256) + 19), logf
      (4 ulp of |lse_j|, at least 4), the addition m + log z (|lse_j|) and the subtraction (|lp_j|).  The combine is a smooth maximum: its
      derivatives with respect to the lp_j are the weights p_j / sum p, which sum to 1, so the members' errors enter with at most the
      largest of them;
  the combine m + logf(sum_j expf(lp_j - m)) - logf(n): per member the argument's subtraction, which reaches the sum with weight
      |d| e^-|d| <= 1, and expf (2 ulp) -- 3 per member; the n - 1 additions of the sum; all of these are relative errors of a sum
      S in [1, n], i.e. absolute errors of log S; logf (4 ulp of log S <= log n: at least 4); the two additions (|m + log S| and |lp|);
  the tail of row_reference: the unk subtraction (|lp| + |unk_penalty|) and the score addition (|base| + |result|).
"""
import math

import torch

import decode_ref
import decode_rules_ref

U, SAFETY, NTHREADS = decode_ref.U, decode_ref.SAFETY, decode_ref.NTHREADS


def row_reference_ensemble(logits, t, beam, pad, unk, eos, max_len, min_len, it, unk_penalty, base, step0_all, tok_hist=None, par_hist=None,
                           ngram=0, prefix=None, mode="lse"):
    """logits: list of the members' device f32 [N, V]; the other arguments as decode_rules_ref.row_reference_rules.  Returns (values
    [N, V] float64, bound).  mode: "lse" is the kernel's; the others are deliberately WRONG combinations the candidate check has to
    reject: "drop1" leaves member 1 out, "nolog" leaves the - log n term out, "meanlog" averages the log-probabilities."""
    xs = [x.double() for x in logits]
    n = len(xs)
    N, V = xs[0].shape
    dev = xs[0].device
    depth = (V + NTHREADS - 1) // NTHREADS + 19
    z = lambda a: a.nan_to_num(0.0, posinf=0.0, neginf=0.0)
    lps, member_err = [], None
    for x in xs:
        val = x * it
        lse = torch.logsumexp(val, -1, keepdim=True)
        lpj = val - lse
        lps.append(lpj)
        e = val.abs() + lse.abs() + z(lpj.abs()) + depth + 4 * lse.abs().clamp_min(1.0)
        member_err = e if member_err is None else torch.maximum(member_err, e)
    if mode == "drop1":
        lps = [lps[j] for j in range(n) if j != 1]
    st = torch.stack(lps)                                                # [n', N, V]
    if mode == "meanlog":
        lp = st.mean(0)
        m = lp
        log_s = torch.zeros_like(lp)
    else:
        m = st.max(0).values
        s = torch.exp(st - m.unsqueeze(0)).sum(0)
        log_s = torch.log(s)
        lp = m + log_s - (0.0 if mode == "nolog" else math.log(len(lps)))
        lp = torch.where(torch.isneginf(m), m, lp)
    comb_err = 3.0 * n + (n - 1) + 4 * log_s.abs().clamp_min(1.0) + z((m + log_s).abs()) + z(lp.abs())
    # ---- from here on as decode_ref.row_reference
    lp = torch.where(torch.isnan(lp), torch.full_like(lp, -math.inf), lp)
    cols = torch.arange(V, device=dev)
    lp[:, pad] = -math.inf
    lp[:, unk] = lp[:, unk] - unk_penalty
    in_prefix = prefix is not None and t < prefix.shape[1] and t < max_len
    if t >= max_len:
        lp = lp.masked_fill((cols != eos)[None, :], -math.inf)
    elif in_prefix:                                                      # the min-len rule is skipped for every sentence (the reference's `elif`)
        pass
    elif t < min_len:
        lp[:, eos] = -math.inf
    live = torch.ones(N, dtype=torch.bool, device=dev) if (t > 0 or step0_all) else (torch.arange(N, device=dev) % beam == 0)
    res = lp + base[:, None]
    res = torch.where(live[:, None], res, torch.full_like(res, -math.inf))
    # ---- the prefix and n-gram rules, as decode_rules_ref.row_reference_rules
    kill = torch.zeros((N, V), dtype=torch.bool)
    if in_prefix:
        for r in range(N):
            p = int(prefix[r // beam][t])
            if p != pad:
                kill[r] = True
                if 0 <= p < V:
                    kill[r, p] = False
    if ngram >= 2:
        for r in range(N):
            for c in decode_rules_ref.banned_columns(decode_rules_ref.history(tok_hist, par_hist, t, r), ngram):
                kill[r, c] = True
    res = res.masked_fill(kill.to(dev), -math.inf)
    tail = z(lp.abs()) + abs(unk_penalty) + base.abs()[:, None] + z(res.abs())
    bound = SAFETY * U * (member_err + comb_err + tail)
    return res, torch.where(torch.isfinite(res), bound, torch.zeros_like(bound))
