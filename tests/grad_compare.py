"""Per-element and per-block comparison of a tensor with its reference (CPU only: test infrastructure, no GPU import).

A whole-tensor norm or cosine averages a localized defect over the tensor: a lost 32-row tile of a [2048, 512] weight gradient
carries 1/64 of its energy and leaves the cosine at sqrt(1 - 1/64) = 0.9922.  The functions here look at the places instead.

  elementwise(mine, ref)     max|mine - ref| / max|ref| and where it is: the fp32 criterion (one wrong element shows)
  blocks(mine, ref, rows)    per block of `rows` leading indices: energy share, relative error, cosine: the bf16 criterion, where
                             honest rounding noise is percent-sized on every element and only its DISTRIBUTION over the tensor tells
                             noise from a defect
  spread(a, b)               the largest block error relative to the whole tensor's: how unevenly the difference of a pair of tensors
                             falls on the blocks.  Of a reference against a more precise reference it is the "null spread" of honest
                             rounding noise on that tensor
  worst_block(mine, ref, null_spread)
                             the figure the bf16 tests bound: block error / (whole-tensor error x null spread), low-energy blocks by
                             their absolute error
"""
import math

import numpy as np
import torch

RUN_1D = 512              # 1-D tensors (biases, LayerNorm / BatchNorm parameters) are cut into runs of this many elements
LOW_SHARE = 0.25          # a block below this fraction of the equal share 1 / n_blocks is "low-energy"


def _f64(t):
    return (t.detach() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).double().cpu()


def elementwise(mine, ref):
    """(max|mine - ref| / max|ref|, index of the worst element as a tuple); a dict of tensors gives a dict of such pairs, over the
    names of `ref`.  An all-zero reference gives inf as soon as one element differs."""
    if isinstance(ref, dict):
        return {k: elementwise(mine[k], g) for k, g in ref.items()}
    a, b = _f64(mine), _f64(ref)
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    if b.numel() == 0:
        return 0.0, ()
    d = (a - b).abs().reshape(-1)
    i = int(d.argmax())
    top, scale = float(d[i]), float(b.abs().max())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(b.shape))) if b.dim() else ()
    return (top / scale if scale > 0 else (0.0 if top == 0 else math.inf)), idx


def blocks(mine, ref, rows=64):
    """The tensor viewed as [dim0, rest] and cut along dim0 into blocks of `rows` (a 1-D tensor: runs of RUN_1D elements); the last
    block may be shorter.  Returns a dict of
      n        number of blocks                       rows     rows (elements, 1-D) per block
      r        |mine - ref| / |ref|, whole tensor      err      |mine - ref|, whole tensor
      share    s_i = |ref_i|^2 / |ref|^2
      rel      r_i = |mine_i - ref_i| / |ref_i|   (nan where the block's reference is zero)
      cos      cosine of the block                (nan where either side is zero)
      abs      |mine_i - ref_i|
      low      s_i < LOW_SHARE / n: the block's reference is (nearly) nothing -- an embedding row that never occurs has a zero
               reference gradient -- so a relative error means nothing there; compare `abs` with the whole tensor's error level
    as float64 numpy arrays of length n (low: bool)."""
    a, b = _f64(mine), _f64(ref)
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    if b.dim() <= 1:
        a, b, rows = a.reshape(-1, 1), b.reshape(-1, 1), RUN_1D
    else:
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    n = max(1, -(-b.shape[0] // rows))
    start = np.arange(n) * rows
    d2 = np.add.reduceat(((a - b) ** 2).sum(1).numpy(), start)
    a2 = np.add.reduceat((a * a).sum(1).numpy(), start)
    b2 = np.add.reduceat((b * b).sum(1).numpy(), start)
    ab = np.add.reduceat((a * b).sum(1).numpy(), start)
    tot = float(b2.sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        share = b2 / tot if tot > 0 else np.zeros(n)
        rel = np.where(b2 > 0, np.sqrt(d2 / b2), np.nan)
        cos = np.where((a2 > 0) & (b2 > 0), ab / np.sqrt(a2 * b2), np.nan)
    err = math.sqrt(float(d2.sum()))
    return dict(n=n, rows=rows, r=(err / math.sqrt(tot) if tot > 0 else (0.0 if err == 0 else math.inf)), err=err, share=share,
                rel=rel, cos=cos, abs=np.sqrt(d2), low=share < LOW_SHARE / n)


def spread(a, b, rows=64):
    """largest r_i / r over the blocks of `b` that carry at least a quarter of the equal share; 1.0 for identical tensors (there
    is no noise to be uneven) and for a tensor of one block"""
    k = blocks(a, b, rows)
    hi = ~k["low"]
    if k["r"] == 0 or not hi.any():
        return 1.0
    return float(np.nanmax(k["rel"][hi]) / k["r"])


def worst_block(mine, ref, null_spread=1.0, rows=64):
    """The block-wise figure of one tensor: max over its blocks of
         r_i / (r x null_spread)                              blocks with at least a quarter share
         |mine_i - ref_i| / (|mine - ref| / sqrt(n) x null_spread)   low-energy blocks: their error against the error an equal share
                                                              of the whole tensor's would be
    so 1.0 means "this block is as wrong as the reference's own rounding noise is uneven", and a bound on the figure is the margin
    allowed on top of that.  Returns (figure, block index, the blocks() dict); (0.0, -1, ...) for identical tensors."""
    k = blocks(mine, ref, rows)
    if k["err"] == 0:
        return 0.0, -1, k
    if not math.isfinite(k["r"]):
        return math.inf, 0, k
    level = k["err"] / math.sqrt(k["n"])
    fig = np.where(k["low"], k["abs"] / level, np.nan_to_num(k["rel"], nan=0.0) / k["r"]) / null_spread
    i = int(np.argmax(fig))
    return float(fig[i]), i, k
