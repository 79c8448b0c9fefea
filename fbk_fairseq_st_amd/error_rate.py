"""Error rates of token sequences against references, on the device: substitutions, insertions and deletions from the edit-distance
alignment of every sentence, with the alignment itself on request.

`ErrorRate(costs=(1, 1, 1))` is the plain Levenshtein alignment, what WER and CER mean everywhere; `ErrorRate.reference_uer(src_dict)`
is the (4, 3, 3) alignment of the reference's `compute_ctc_uer` with the dictionary's `<ctc_blank>`, so that `ctc_acc` numbers can be
reproduced from device transcripts.  Under weighted costs the counts are those of the path the reference's tie rule picks, which is
not always the path with the fewest errors.  `score` aligns two padded matrices, `score_frames` takes the frame arg-maxes of the CTC
head (`kernels.ctc_argmax`) with the criterion's operands, `score_hypotheses` takes what `CTCDecoder.generate` or
`SequenceGenerator.generate` returns.  Every call returns per-sentence device tensors and adds its sums to a device accumulator;
`result()` makes the object's one device-to-host copy.

The hot path is csrc/edit_align.hip (kernels.edit_align; include/s2t_hip.h states the rule): one launch per call, no host read.
Hypotheses of at most MAX_HYP tokens (or frames), references of at most MAX_REF.
"""
import torch

from . import kernels as K
from .token_rows import as_ints, best_rows, pad_rows

MAX_HYP = K.EDIT_MAX_A                  # S2T_EDIT_MAX_A
MAX_REF = K.EDIT_MAX_B                  # S2T_EDIT_MAX_B
OPS = {0: "match", 1: "substitution", 2: "deletion (a reference token left alone)", 3: "insertion (a hypothesis token left alone)"}
STATUS = {0: "done", 2: "refused: a length outside the padded width"}
WORKSPACE_LIMIT = 1 << 30               # bytes of step storage one call with ops=True may ask for
_SUMS = ("errors", "substitutions", "insertions", "deletions", "ref_tokens", "sentences")


class ErrorRate:
    """costs: (substitution, hypothesis token left alone, reference token left alone), integers in [1, 255].  blank: the label
    score_frames drops after collapsing repeats."""

    def __init__(self, costs=(1, 1, 1), blank=None):
        self.costs = tuple(int(c) for c in costs)
        if len(self.costs) != 3 or not all(1 <= c <= 255 for c in self.costs):
            raise ValueError("ErrorRate: costs must be three integers in [1, 255], got %r" % (tuple(costs),))
        self.blank = None if blank is None else int(blank)
        self._acc = None

    @classmethod
    def reference_uer(cls, src_dict):
        """the scorer of the reference's compute_ctc_uer: costs (4, 3, 3), the blank is the dictionary's `<ctc_blank>` entry"""
        blank = src_dict.index("<ctc_blank>")
        if blank == src_dict.unk():
            raise ValueError("the dictionary has no <ctc_blank> entry")
        return cls(costs=(4, 3, 3), blank=blank)

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def score(self, hyp, hyp_len, ref, ref_len, ops=False):
        """hyp [B, Hmax] and ref [B, Rmax] integer token matrices (device), hyp_len / ref_len [B] their lengths.  Returns a dict of
        per-sentence device tensors: `substitutions`, `insertions` (hypothesis tokens left alone), `deletions` (reference tokens
        left alone), `matches`, `errors` (their sum without the matches), `cost`, `ref_len` (int64), `status` (see STATUS; the
        numbers of a refused sentence are 0 and it adds nothing to the accumulator); with ops=True also `ops` (uint8
        [B, Hmax + Rmax], see OPS; entries behind `n_ops` are not written) and `n_ops`."""
        return self._run(hyp, hyp_len, ref, ref_len, None, ops)

    @torch.no_grad()
    def score_frames(self, pred, in_len, ref, ref_len):
        """pred [B, T] frame arg-maxes (kernels.ctc_argmax gives them), in_len [B] frames per sentence: repeats are collapsed and
        the blank dropped in the same call.  Returns the dict of `score` plus `hyp_len` (the collapsed lengths) and `hyp` (the
        collapsed tokens [B, T]; entries behind hyp_len are not written)."""
        if self.blank is None:
            raise ValueError("ErrorRate.score_frames needs the blank: ErrorRate(costs, blank=...) or ErrorRate.reference_uer(src_dict)")
        return self._run(pred, in_len, ref, ref_len, self.blank, False)

    @torch.no_grad()
    def score_hypotheses(self, hypos, ref, ref_len, strip_eos=None, ops=False):
        """hypos: per sentence a list of dicts with `tokens` (1-D device tensors), best first, what CTCDecoder.generate and
        SequenceGenerator.generate return; the best hypothesis of every sentence is scored (a sentence without one counts as
        empty).  strip_eos: that token is dropped from the end of a hypothesis and of a reference that ends in it."""
        dev = ref.device
        best = best_rows(hypos, dev)
        if len(best) != ref.shape[0]:
            raise ValueError("ErrorRate.score_hypotheses: %d sentences of hypotheses, %d references" % (len(best), ref.shape[0]))
        hyp, hyp_len = pad_rows(best, dev)                              # lengths are shapes: no host read
        ref, ref_len = as_ints(ref, ref_len, dev)
        if strip_eos is not None:
            hyp_len = _strip(hyp, hyp_len, int(strip_eos))
            ref_len = _strip(ref, ref_len, int(strip_eos))
        return self._run(hyp, hyp_len, ref, ref_len, None, ops)

    @staticmethod
    def chunk_sentences(hyp_width, ref_width):
        """sentences one call with ops=True takes so that its step storage stays under WORKSPACE_LIMIT (at least 1)"""
        per = 4 * (hyp_width + 1) * ((ref_width + 1 + 15) // 16) + 8 * hyp_width + 512
        return max(1, WORKSPACE_LIMIT // per)

    def _run(self, hyp, hyp_len, ref, ref_len, collapse_blank, ops):
        if hyp.dim() != 2 or ref.dim() != 2 or hyp.shape[0] != ref.shape[0]:
            raise ValueError("ErrorRate: hypotheses and references must be [B, width] matrices with one B, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        if hyp.shape[1] > MAX_HYP:
            raise ValueError("ErrorRate: hypotheses of at most %d tokens or frames (S2T_EDIT_MAX_A), got a padded width of %d"
                             % (MAX_HYP, hyp.shape[1]))
        if ref.shape[1] > MAX_REF:
            raise ValueError("ErrorRate: references of at most %d tokens (S2T_EDIT_MAX_B), got a padded width of %d"
                             % (MAX_REF, ref.shape[1]))
        dev = hyp.device
        hyp, hyp_len = as_ints(hyp, hyp_len, dev)
        ref, ref_len = as_ints(ref, ref_len, dev)
        B = hyp.shape[0]
        step = self.chunk_sentences(hyp.shape[1], ref.shape[1]) if ops else max(B, 1)
        parts = [K.edit_align(hyp[s:s + step], hyp_len[s:s + step], ref[s:s + step], ref_len[s:s + step], self.costs,
                              collapse_blank=collapse_blank, want_ops=ops) for s in range(0, max(B, 1), step)]
        # sentences are independent: the chunks' results are the unchunked call's
        counts, cost, status, a_n, a_out, op, n_ops = [None if p[0] is None else (p[0] if len(parts) == 1 else torch.cat(p))
                                                       for p in zip(*parts)]
        done = status == 0
        out = {"matches": counts[:, 0], "substitutions": counts[:, 1], "deletions": counts[:, 2], "insertions": counts[:, 3],
               "errors": counts[:, 1:].sum(1, dtype=torch.int32), "cost": cost, "ref_len": ref_len.long() * done, "status": status}
        if ops:
            out["ops"], out["n_ops"] = op, n_ops
        if collapse_blank is not None:
            out["hyp"], out["hyp_len"] = a_out, a_n
        sums = torch.stack([out["errors"].sum(), out["substitutions"].sum(), out["insertions"].sum(), out["deletions"].sum(),
                            out["ref_len"].sum(), done.sum()]).long()
        self._acc = sums if self._acc is None else self._acc + sums.to(self._acc.device)
        return out

    # ------------------------------------------------------------------ accumulation
    def result(self):
        """the sums over every call since the last reset() -- errors, substitutions, insertions, deletions, ref_tokens, sentences
        (refused sentences left out) -- with `error_rate` = 100 * errors / max(ref_tokens, 1) in percent, not capped, and
        `accuracy` = 100 - min(error_rate, 100), the form of ctc_acc.  The object's one device-to-host copy."""
        vals = [0] * len(_SUMS) if self._acc is None else self._acc.tolist()
        out = dict(zip(_SUMS, vals))
        out["error_rate"] = 100.0 * out["errors"] / max(out["ref_tokens"], 1)
        out["accuracy"] = 100.0 - min(out["error_rate"], 100.0)
        return out

    def reset(self):
        self._acc = None


def _strip(tok, ln, eos):
    """lengths without a trailing `eos`"""
    if tok.shape[1] == 0:
        return ln
    last = tok.gather(1, (ln.long() - 1).clamp(0, tok.shape[1] - 1)[:, None])[:, 0]
    return ln - ((ln > 0) & (ln <= tok.shape[1]) & (last == eos)).to(ln.dtype)
