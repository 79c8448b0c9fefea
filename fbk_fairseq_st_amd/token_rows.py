"""Token rows on their way to the scorers' kernels (bleu_scorer, chrf_scorer, error_rate, mbr): integer matrices with lengths of
their own dtype, lists of 1-D hypotheses padded into such matrices, and the tables of an n-best call.  Lengths and list shapes come
from tensor shapes: nothing here reads the device."""
import torch

INTS = (torch.int32, torch.int64)


def as_ints(tok, ln, dev):
    """tokens on dev as int32 (kept) or int64 (every other dtype), the lengths in the tokens' dtype"""
    tok = tok.to(dev)
    if tok.dtype not in INTS:
        tok = tok.long()
    return tok, ln.to(device=dev, dtype=tok.dtype)


def pad_rows(rows, dev):
    """1-D token tensors -> (matrix padded with zeros, lengths); int32 if every row is, int64 otherwise"""
    dtype = torch.int32 if rows and all(t.dtype == torch.int32 for t in rows) else torch.int64
    lens = [t.numel() for t in rows]
    width = max(lens + [0])
    mat = torch.zeros((len(rows), width), dtype=dtype, device=dev)
    if width:
        mat = torch.nn.utils.rnn.pad_sequence([t.to(dtype) for t in rows], batch_first=True)
    return mat, torch.tensor(lens, dtype=dtype, device=dev)


def best_rows(hypos, dev):
    """hypos: per sentence a list of dicts with `tokens`, best first -> the first hypothesis of every sentence as a 1-D tensor on
    dev, an empty row for a sentence without one"""
    return [h[0]["tokens"].to(dev).reshape(-1) if len(h) else torch.empty((0,), dtype=torch.int64, device=dev) for h in hypos]


def nbest_tables(hypos, B, dev, run, width, key, lowest=False):
    """Every hypothesis of B sentences through one call.  run(hyp, hyp_len, rows) scores the flat list (rows: int32, the sentence of
    every hypothesis) and returns a dict with `stats` [n, width], `status` [n] and the float64 score `key` [n].  Returns
    (stats [B, N, width], status [B, N], score [B, N], n_hyp [B], oracle [B], pick): N the longest list, at least 1; zeros, and -1 in
    the score, behind a list's end; oracle the first index of the row's highest score (0 for an empty list); pick(which) the int64
    sums [width] of the stats of hypothesis 0 ("best") or oracle[b] ("oracle") over the sentences.  lowest: the score is an error
    rate -- oracle is the first index of the row's lowest score among its finished entries (status 0; a refused entry's score of 0
    is no result), 0 for a list without one."""
    counts = [len(h) for h in hypos]
    N = max(counts + [1])
    flat = [h["tokens"].to(dev).reshape(-1) for hs in hypos for h in hs]
    sent = [b for b, n in enumerate(counts) for _ in range(n)]                 # lists' shapes: no host read
    slot = [k for n in counts for k in range(n)]
    hyp, hyp_len = pad_rows(flat, dev)
    rows = torch.tensor(sent, dtype=torch.int32, device=dev)
    got = run(hyp, hyp_len, rows)
    at = (rows.long(), torch.tensor(slot, dtype=torch.int64, device=dev))
    stats = torch.zeros((B, N, width), dtype=torch.int32, device=dev)
    status = torch.zeros((B, N), dtype=torch.int32, device=dev)
    score = torch.full((B, N), -1.0, dtype=torch.float64, device=dev)
    stats[at], status[at], score[at] = got["stats"], got["status"], got[key]
    cols = torch.arange(N, device=dev).expand(B, N)                            # the first index of the row's maximum
    rank = score
    if lowest:                                                                 # ... of the lowest score that is a result
        rank = torch.where((score >= 0) & (status == 0), -score, torch.full_like(score, float("-inf")))
    oracle = torch.where(rank == rank.max(1, keepdim=True).values, cols, torch.full_like(cols, N)).min(1).values if B else \
        torch.zeros((0,), dtype=torch.int64, device=dev)

    def pick(which):
        at = oracle if which == "oracle" else torch.zeros_like(oracle)
        return stats.gather(1, at[:, None, None].expand(B, 1, width)).sum((0, 1), dtype=torch.int64)
    return stats, status, score, torch.tensor(counts, dtype=torch.int64, device=dev), oracle, pick
