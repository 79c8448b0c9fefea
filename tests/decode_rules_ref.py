"""The two score rules of s2t_decode_step_rules (csrc/decode.hip, dec_row_kernel<VPT, true>) restated on top of decode_ref.row_reference.

Both rules only write -inf over values row_reference computes (fairseq/sequence_generator.py:270-280, 449-476 prefix tokens; :596-650
n-gram blocking), so they add no arithmetic and no allowance: a candidate value is compared within row_reference's own bound.

A row's history is rebuilt from the selection records (`tok_hist`, `par_hist`: arrangement i = the beam after i selections), NOT from
the ancestor table `anc` the kernel gathers through: a wrong gather shows up as a wrong ban.
"""
import math

import torch

import decode_ref


def history(tok_hist, par_hist, t, n):
    """g[0 .. t] of the hypothesis in slot n at step t (<bos> first): walk the parent links down from arrangement t"""
    g = [0] * (t + 1)
    r = int(n)
    for i in range(t, -1, -1):
        g[i] = int(tok_hist[i][r])
        if i > 0:
            r = int(par_hist[i][r])
    return g


def banned_columns(g, ngram):
    """every j with g[j .. j+n-2] == the last n - 1 tokens bans g[j+n-1] (sequence_generator.py:617-650); n >= 2"""
    assert ngram >= 2
    head = g[len(g) - (ngram - 1):]
    if len(head) < ngram - 1:
        return set()
    return {g[j + ngram - 1] for j in range(len(g) - ngram + 1) if g[j:j + ngram - 1] == head}


def row_reference_rules(logits, t, beam, pad, unk, eos, max_len, min_len, it, unk_penalty, base, step0_all, tok_hist, par_hist,
                        ngram=0, prefix=None):
    """decode_ref.row_reference with the rules.  tok_hist / par_hist: host arrays [max_len + 2][N] (the device's own records up to
    arrangement t); prefix: host integer array [B][P] or None (pad = free).  Returns (values [N, V] float64, bound)."""
    N, V = logits.shape
    in_prefix = prefix is not None and t < prefix.shape[1] and t < max_len
    # inside the prefix the min-len rule is skipped for every sentence (the reference's `elif`)
    res, bound = decode_ref.row_reference(logits, t, beam, pad, unk, eos, max_len, 0 if in_prefix else min_len, it, unk_penalty, base,
                                          step0_all)
    kill = torch.zeros((N, V), dtype=torch.bool)
    if in_prefix:
        for n in range(N):
            p = int(prefix[n // beam][t])
            if p != pad:
                kill[n] = True
                if 0 <= p < V:
                    kill[n, p] = False
    if ngram >= 2:
        for n in range(N):
            for c in banned_columns(history(tok_hist, par_hist, t, n), ngram):
                kill[n, c] = True
    kill = kill.to(res.device)
    res = res.masked_fill(kill, -math.inf)
    return res, torch.where(torch.isfinite(res), bound, torch.zeros_like(bound))
