"""BLEU of token sequences against references, on the device: the n-gram statistics of every sentence (the ten numbers of the
reference's `bleu_add`), the smoothed sentence score, and the corpus score of `fairseq/bleu.py:Scorer` from their sums.

`BleuScorer(pad, eos, unk)` takes the three ids of the target dictionary (`BleuScorer.for_dictionary(tgt_dict)`); `score` takes two
padded matrices, `score_hypotheses` the best hypothesis of every sentence of what `SequenceGenerator.generate` returns,
`score_nbest` every hypothesis of every sentence (the n-best list shares its reference through a row map, nothing is copied) with
the index of the best-scoring one.  Every call returns per-sentence device tensors and adds its sums to a device accumulator;
`result()` makes the object's one device-to-host copy, `result_string()` prints what `generate.py` prints.

The hot path is csrc/bleu_stats.hip (kernels.bleu_stats; include/s2t_hip.h states the rule): one launch per call, no host read.
Padded widths of at most MAX_LEN tokens on either side.
"""
import math

import torch

from . import kernels as K
from .token_rows import as_ints, best_rows, nbest_tables, pad_rows

MAX_LEN = K.BLEU_MAX_LEN                # S2T_BLEU_MAX_LEN
STATUS = {0: "done", 2: "refused: a length outside the padded width, or a reference row outside the references"}
_SUMS = ("ref_len", "sys_len", "match1", "count1", "match2", "count2", "match3", "count3", "match4", "count4")


class BleuScorer:
    """pad, eos, unk: the ids the reference's Scorer is built with.  Leading pads and trailing eos / pad are trimmed from both sides
    (never the first remaining token); a reference token equal to unk matches nothing (unk < 0 switches that off)."""

    def __init__(self, pad, eos, unk=-1):
        self.pad, self.eos, self.unk = int(pad), int(eos), int(unk)
        if self.pad == self.eos or (self.unk >= 0 and self.unk in (self.pad, self.eos)):
            raise ValueError("BleuScorer: pad, eos and unk must be three different ids, got %d, %d and %d" % (self.pad, self.eos, self.unk))
        self._acc = None

    @classmethod
    def for_dictionary(cls, tgt_dict):
        return cls(tgt_dict.pad(), tgt_dict.eos(), tgt_dict.unk())

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def score(self, hyp, hyp_len, ref, ref_len):
        """hyp [B, Hmax] and ref [B, Rmax] integer token matrices (device), hyp_len / ref_len [B] their lengths.  Returns a dict of
        per-sentence device tensors: `stats` (int32 [B, 10]: reflen, predlen, match1, count1, ... match4, count4 -- the reference's
        BleuStat), `match` and `count` (int32 [B, 4], views of it), `sys_len`, `ref_len` (the trimmed lengths), `status` (see STATUS;
        the numbers of a refused sentence are 0 and it adds nothing to the accumulator) and `sentence_bleu` (float64, in percent:
        the reference's score after reset(one_init=True) and this one sentence; 0 for a refused sentence or an empty hypothesis)."""
        out = self._run(hyp, hyp_len, ref, ref_len, None)
        self._add(out["stats"].sum(0, dtype=torch.int64))
        return out

    @torch.no_grad()
    def score_hypotheses(self, hypos, ref, ref_len):
        """hypos: per sentence a list of dicts with `tokens` (1-D device tensors), best first, what SequenceGenerator.generate
        returns; the best hypothesis of every sentence is scored (a sentence without one counts as empty).  Returns what `score`
        returns."""
        dev = ref.device
        best = best_rows(hypos, dev)
        if len(best) != ref.shape[0]:
            raise ValueError("BleuScorer.score_hypotheses: %d sentences of hypotheses, %d references" % (len(best), ref.shape[0]))
        hyp, hyp_len = pad_rows(best, dev)
        return self.score(hyp, hyp_len, ref, ref_len)

    @torch.no_grad()
    def score_nbest(self, hypos, ref, ref_len, accumulate=None):
        """every hypothesis of every sentence against the sentence's reference, in one call.  Returns a dict of device tensors shaped
        [B, N] (N the longest list, at least 1) -- `stats` [B, N, 10], `match` and `count` [B, N, 4], `sys_len`, `ref_len`, `status`,
        `sentence_bleu` -- with zeros, and -1 in `sentence_bleu`, behind `n_hyp` [B] (int64, the lists' lengths), and `oracle` [B]
        (int64), the first index of the highest sentence BLEU (0 for a sentence without hypotheses).  accumulate: None adds nothing to
        the accumulator, "best" the stats of hypothesis 0 of every sentence, "oracle" those of hypothesis oracle[b]; a sentence
        without hypotheses adds nothing."""
        if accumulate not in (None, "best", "oracle"):
            raise ValueError("BleuScorer.score_nbest: accumulate is None, 'best' or 'oracle', got %r" % (accumulate,))
        dev = ref.device
        B = len(hypos)
        if B != ref.shape[0]:
            raise ValueError("BleuScorer.score_nbest: %d sentences of hypotheses, %d references" % (B, ref.shape[0]))
        stats, status, bleu, n_hyp, oracle, pick = nbest_tables(
            hypos, B, dev, lambda hyp, hyp_len, rows: self._run(hyp, hyp_len, ref, ref_len, rows), 10, "sentence_bleu")
        out = _fields(stats, status, bleu)
        out["n_hyp"], out["oracle"] = n_hyp, oracle
        if accumulate is not None and B:
            self._add(pick(accumulate))
        return out

    def _run(self, hyp, hyp_len, ref, ref_len, rows):
        if hyp.dim() != 2 or ref.dim() != 2 or (rows is None and hyp.shape[0] != ref.shape[0]):
            raise ValueError("BleuScorer: hypotheses and references must be [B, width] matrices with one B, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        if hyp.shape[1] > MAX_LEN or ref.shape[1] > MAX_LEN:
            raise ValueError("BleuScorer: padded widths of at most %d tokens (S2T_BLEU_MAX_LEN), got %d and %d"
                             % (MAX_LEN, hyp.shape[1], ref.shape[1]))
        dev = hyp.device
        hyp, hyp_len = as_ints(hyp, hyp_len, dev)
        ref, ref_len = as_ints(ref, ref_len, dev)
        stats, status = K.bleu_stats(hyp, hyp_len, ref, ref_len, self.pad, self.eos, self.unk, ref_row=rows)
        return _fields(stats, status, sentence_bleu(stats))

    # ------------------------------------------------------------------ accumulation
    def _add(self, sums):
        self._acc = sums if self._acc is None else self._acc + sums.to(self._acc.device)

    def result(self):
        """the ten sums over every call since the last reset() -- ref_len, sys_len, match1, count1, ... match4, count4 (refused
        sentences left out) -- with `precisions` (four ratios, 0 where the count is 0), `brevity`, `ratio` (sys_len / ref_len) and
        `bleu` in percent, by the arithmetic of the reference's Scorer (bleu.py:100-118); `bleu` is 0.0 when a precision is 0.  With
        sys_len == 0 nothing is divided: zeros (the reference raises there); ratio is inf for ref_len == 0 < sys_len.  The object's
        one device-to-host copy."""
        vals = [0] * len(_SUMS) if self._acc is None else self._acc.tolist()
        out = dict(zip(_SUMS, vals))
        out.update(_corpus(vals, 4))
        return out

    def result_string(self, order=4):
        """the line the reference prints (bleu.py:120-129), character for character"""
        if not 1 <= order <= 4:
            raise ValueError("BLEU scores for order > 4 aren't supported")
        vals = [0] * len(_SUMS) if self._acc is None else self._acc.tolist()
        c = _corpus(vals, order)
        fmt = "BLEU{} = {:2.2f}, {:2.1f}"
        for _ in range(1, order):
            fmt += "/{:2.1f}"
        fmt += " (BP={:.3f}, ratio={:.3f}, syslen={}, reflen={})"
        return fmt.format(order, c["bleu"], *[p * 100 for p in c["precisions"][:order]], c["brevity"], c["ratio"], vals[1], vals[0])

    def reset(self):
        self._acc = None


def _corpus(vals, order):
    """bleu.py:100-118 on ten sums"""
    prec = [vals[2 + 2 * k] / vals[3 + 2 * k] if vals[3 + 2 * k] > 0 else 0 for k in range(4)]
    if vals[1] == 0:
        return {"bleu": 0.0, "precisions": [0.0] * 4, "brevity": 0.0, "ratio": 0.0}
    brevity = min(1, math.exp(1 - vals[0] / vals[1]))
    psum = sum(math.log(p) if p > 0 else float("-Inf") for p in prec[:order])
    return {"bleu": brevity * math.exp(psum / order) * 100, "precisions": prec, "brevity": brevity,
            "ratio": vals[1] / vals[0] if vals[0] > 0 else float("inf")}


def sentence_bleu(stats):
    """stats [..., 10] integers -> float64 [...]: brevity * exp(mean of the four log precisions) * 100 with match and count of the
    orders 2 to 4 raised by one; 0 where the hypothesis is empty (a refused sentence has zeros) or nothing matches at order 1"""
    s = stats.double()
    match, count = s[..., 2::2].clone(), s[..., 3::2].clone()
    match[..., 1:] += 1
    count[..., 1:] += 1
    some = s[..., 1] > 0
    prec = torch.where(count > 0, match / count.clamp(min=1), torch.zeros_like(match))
    sys_len = torch.where(some, s[..., 1], torch.ones_like(s[..., 1]))
    brevity = torch.exp(1 - s[..., 0] / sys_len).clamp(max=1)
    bleu = brevity * torch.exp(torch.log(prec).sum(-1) / 4) * 100          # log 0 = -inf, exp -inf = 0
    return torch.where(some, bleu, torch.zeros_like(bleu))


def _fields(stats, status, bleu):
    return {"stats": stats, "match": stats[..., 2::2], "count": stats[..., 3::2], "sys_len": stats[..., 1], "ref_len": stats[..., 0],
            "status": status, "sentence_bleu": bleu}
