"""Minimum-Bayes-risk selection over n-best lists, on the device: among the candidates of a sentence, the one with the highest
expected sentence BLEU against the other hypotheses of the same sentence, used as pseudo-references.

`MBRDecoder(generator, pad, eos, unk)` (`MBRDecoder.for_dictionary(generator, tgt_dict)`) wraps a generator -- a beam, diverse or
sampling `SequenceGenerator` -- and is handed to `task.inference_step` in its place, like `SequenceScorer` and `CTCDecoder`:
`generate` runs the generator and returns its lists reordered by expected utility.  `rerank` does the same on lists the caller
made (the pseudo-references may be another list per sentence, for example beam candidates judged against samples), and
`expected_bleu` is the matrix level, device tensors in and out.

The utility of a pair is the smoothed sentence BLEU of `BleuScorer` (bleu_scorer.sentence_bleu on the pair's ten statistics, bit
for bit what `BleuScorer.score` gives that pair), with the candidate as the hypothesis and the pseudo-reference as the reference.
The gain of a candidate is the weighted mean of its utilities over the pseudo-references of its sentence.  When the
pseudo-references are the candidates themselves (`pseudo` is `hypos`, and always in `generate`), a sentence's own hypothesis is among
its pseudo-references: nothing is left out.  A hypothesis that contains `unk` therefore scores below 100 against itself -- a
reference-side `unk` matches nothing: that is the reference's rule for references, kept as it is.

With `utility=ChrfScorer(...)` the utility of a pair is instead the chrF of the two detokenised texts (chrf_scorer.py):
the pairs of a sentence go through `ChrfScorer.score_pairs` on two device row maps, and `mbr_score` is in chrF percent.  With
`utility=TextErrorRate(...)` (text_error_rate.py) it is the word or character accuracy of the candidate's text against
the pseudo-reference's, 100 - min(error rate, 100): the classic MBR for speech recognition, by expected word error.  A utility
object has `score_pairs` and may name the pair score it returns (`utility_key`; "sentence_chrf" without one) and the bytes a pair
costs (`pair_bytes`); the score lies in [0, 100] with 0 worst.

The hot path is csrc/bleu_pairs.hip (kernels.bleu_pairs; include/s2t_hip.h states the operands, the rule is s2t_bleu_stats's): one
launch for all pairs of a call, no copies of the lists, no host read.  Padded widths of at most MAX_LEN tokens, lists of at most
MAX_LIST pseudo-references per sentence.
"""
import torch

from . import kernels as K
from .bleu_scorer import sentence_bleu
from .token_rows import as_ints, pad_rows

MAX_LEN = K.MBR_MAX_LEN                 # S2T_MBR_MAX_LEN
MAX_LIST = K.MBR_MAX_LIST               # S2T_MBR_MAX_LIST
OUTPUT_LIMIT = 1 << 30                  # bytes of stats and status one kernel call may ask for: above it a batch is cut by sentences
STATUS = {0: "done", 2: "refused: a length outside the padded width, a sentence outside the batch, or offsets that are no list"}
_CHRF_PAIR_BYTES = 4 * K.CHRF_STATS + 4 + 8 + 8      # stats, status, the two row maps and the float64 score of a pair of the chrF utility


class MBRDecoder:
    """generator: anything with `generate(models, sample, prefix_tokens=None)` that returns, per sentence, a list of dicts with
    `tokens` (and `score`, for weights="score"); None for an object that only reranks.  pad, eos, unk: the ids `BleuScorer` takes
    (unk < 0: a reference-side unk is an ordinary token).  weights: the default of `generate` and `rerank` --
      "uniform"  every pseudo-reference counts the same;
      "score"    pseudo-reference k counts exp(score_k - max score of its sentence), computed in float64 on the device;
      a tensor or list [M] of non-negative numbers: pseudo-reference k of every sentence counts weights[k]; or one such sequence
      per sentence (a list of them, or a tensor [B, M]), each at least as long as the sentence's list.
    utility: None for the sentence BLEU over token ids described above, or a `ChrfScorer`: then the utility of a pair is the
    scorer's `sentence_chrf` of the two texts (chrf_scorer.py; its `score_pairs` on two device row maps built from the lists'
    shapes, one launch of kernels.chrf_stats per cut), `mbr_score` is in chrF percent, and the pairs the kernel refuses count for
    nothing.  The scorer's accumulator takes the pairs' sums as with any `score_pairs` call.  A `TextErrorRate` takes the same
    route with its `sentence_accuracy` (two launches per cut); `mbr_score` is then the expected accuracy in percent."""

    def __init__(self, generator, pad, eos, unk=-1, weights="uniform", utility=None):
        self.generator = generator
        self.utility = utility
        self.pad, self.eos, self.unk = int(pad), int(eos), int(unk)
        if self.pad == self.eos or (self.unk >= 0 and self.unk in (self.pad, self.eos)):
            raise ValueError("MBRDecoder: pad, eos and unk must be three different ids, got %d, %d and %d" % (self.pad, self.eos, self.unk))
        if isinstance(weights, str) and weights not in ("uniform", "score"):
            raise ValueError("MBRDecoder: weights is 'uniform', 'score' or a sequence of numbers, got %r" % (weights,))
        self.weights = weights

    @classmethod
    def for_dictionary(cls, generator, tgt_dict, weights="uniform", utility=None):
        return cls(generator, tgt_dict.pad(), tgt_dict.eos(), tgt_dict.unk(), weights=weights, utility=utility)

    # ------------------------------------------------------------------ the generator's place
    @torch.no_grad()
    def generate(self, models, sample, prefix_tokens=None, **kw):
        """runs the generator (its route, the device search included, is untouched) and returns its lists -- the same dicts --
        reordered by expected utility, every list judged against itself; see `rerank` for what each dict gains"""
        if self.generator is None:
            raise ValueError("MBRDecoder.generate: built without a generator")
        return self.rerank(self.generator.generate(models, sample, prefix_tokens=prefix_tokens, **kw))

    # ------------------------------------------------------------------ lists
    @torch.no_grad()
    def rerank(self, hypos, pseudo=None, weights=None):
        """hypos: per sentence a list of dicts with `tokens` (1-D device tensors).  pseudo: per sentence the list of dicts that
        serve as pseudo-references; None takes hypos itself.  weights: None takes the object's.  Returns new lists of the same
        dicts in descending order of expected utility; the order is stable, so ties keep the order they came in.  Each dict gains
        `mbr_score` (the expected sentence BLEU in percent, a float64 device scalar; 0 against an empty list) and `mbr_index` (its
        place in the list that came in).  One device-to-host copy: the order."""
        same = pseudo is None
        pseudo = hypos if same else pseudo
        B = len(hypos)
        if len(pseudo) != B:
            raise ValueError("MBRDecoder.rerank: %d sentences of hypotheses, %d of pseudo-references" % (B, len(pseudo)))
        nc, nr = [len(h) for h in hypos], [len(p) for p in pseudo]
        if max(nr + [0]) > MAX_LIST:
            raise ValueError("MBRDecoder: lists of at most %d pseudo-references (S2T_MBR_MAX_LIST), got %d" % (MAX_LIST, max(nr)))
        weights = self.weights if weights is None else weights
        dev = next((h["tokens"].device for hs in list(hypos) + list(pseudo) for h in hs), torch.device("cpu"))
        out = [[] for _ in range(B)]
        for b0, b1 in self.chunk_sentences(nc, nr, self._pair_bytes(hypos, pseudo)):
            gain = self._gains(hypos[b0:b1], pseudo[b0:b1], same, weights, b0, B, dev)
            if gain is None:
                continue
            sent = torch.tensor([b for b in range(b0, b1) for _ in range(nc[b])], dtype=torch.int64, device=dev)
            order = torch.argsort(-gain, stable=True)
            order = order[torch.argsort(sent[order], stable=True)].tolist()            # by sentence, then by gain; ties as they came
            first = [0] * (b1 - b0 + 1)
            for b in range(b0, b1):
                first[b - b0 + 1] = first[b - b0] + nc[b]
            at = 0
            for b in range(b0, b1):
                for c in order[at:at + nc[b]]:
                    k = c - first[b - b0]
                    h = hypos[b][k]
                    h["mbr_score"], h["mbr_index"] = gain[c], k
                    out[b].append(h)
                at += nc[b]
        return out

    def _pair_bytes(self, hypos, pseudo):
        """what a call writes per pair: 44 for the BLEU kernel, else the utility's `pair_bytes` -- a number, or a function of the two
        token widths (the longest candidate and pseudo-reference: shapes, no device read) -- and _CHRF_PAIR_BYTES without one"""
        if self.utility is None:
            return 44
        per = getattr(self.utility, "pair_bytes", _CHRF_PAIR_BYTES)
        if callable(per):
            per = per(max([h["tokens"].numel() for hs in hypos for h in hs] + [0]), max([h["tokens"].numel() for hs in pseudo for h in hs] + [0]))
        return int(per)

    @staticmethod
    def chunk_sentences(nc, nr, pair_bytes=44):
        """nc, nr: candidates and pseudo-references per sentence; pair_bytes: what a call writes per pair.  -> ranges [b0, b1) of
        sentences, in order, each as long as the stats and status of one call stay under OUTPUT_LIMIT (a sentence that passes it
        alone is a range of its own)"""
        ranges, b0, rows, width = [], 0, 0, 0
        for b in range(len(nc)):
            r, w = rows + nc[b], max(width, nr[b])
            if b > b0 and r * w * pair_bytes > OUTPUT_LIMIT:
                ranges.append((b0, b))
                b0, r, w = b, nc[b], nr[b]
            rows, width = r, w
        if len(nc) > b0:
            ranges.append((b0, len(nc)))
        return ranges

    def _gains(self, hypos, pseudo, same, weights, b0, B, dev):
        """the gain of every candidate of these sentences, float64 [candidates]; None without candidates"""
        nc, nr = [len(h) for h in hypos], [len(p) for p in pseudo]
        if sum(nc) == 0:
            return None
        cand, cand_len = pad_rows([h["tokens"].to(dev).reshape(-1) for hs in hypos for h in hs], dev)
        if same:
            ref, ref_len = cand, cand_len
        else:
            ref, ref_len = pad_rows([h["tokens"].to(dev).reshape(-1) for hs in pseudo for h in hs], dev)
        cand_sent = torch.tensor([b for b, n in enumerate(nc) for _ in range(n)], dtype=torch.int32, device=dev)   # lists' shapes
        off = [0]
        for n in nr:
            off.append(off[-1] + n)
        ref_off = torch.tensor(off, dtype=torch.int32, device=dev)
        w = self._weights(weights, pseudo, nr, b0, B, dev)
        if self.utility is not None:
            return self._expected_utility(cand, cand_len, cand_sent, nc, ref, ref_len, ref_off, nr, w, dev)
        return self.expected_bleu(cand, cand_len, cand_sent, ref, ref_len, ref_off, weights=w, max_list=max(nr))["gain"]

    @staticmethod
    def _weights(weights, pseudo, nr, b0, B, dev):
        """-> None (uniform) or float64 [pseudo-reference rows] on dev"""
        if isinstance(weights, str):
            if weights == "uniform":
                return None
            if weights != "score":
                raise ValueError("MBRDecoder: weights is 'uniform', 'score' or a sequence of numbers, got %r" % (weights,))
            if sum(nr) == 0:
                return torch.zeros((0,), dtype=torch.float64, device=dev)
            s = torch.stack([torch.as_tensor(h["score"], dtype=torch.float64, device=dev).reshape(()) for hs in pseudo for h in hs])
            sent = torch.tensor([b for b, n in enumerate(nr) for _ in range(n)], dtype=torch.int64, device=dev)
            top = torch.full((len(nr),), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, sent, s, "amax")
            return torch.exp(s - top[sent])
        if torch.is_tensor(weights) and weights.dim() == 2:
            weights = list(weights)
        per_sentence = isinstance(weights, (list, tuple)) and len(weights) > 0 and not isinstance(weights[0], (int, float))
        if per_sentence:
            if len(weights) != B:
                raise ValueError("MBRDecoder: %d sequences of weights for %d sentences" % (len(weights), B))
            rows = [torch.as_tensor(weights[b0 + b], dtype=torch.float64).reshape(-1) for b in range(len(nr))]
        else:
            rows = [torch.as_tensor(weights, dtype=torch.float64).reshape(-1)] * len(nr)
        for b, (r, n) in enumerate(zip(rows, nr)):
            if r.numel() < n:
                raise ValueError("MBRDecoder: %d weights for the %d pseudo-references of sentence %d" % (r.numel(), n, b0 + b))
            if not r.is_cuda and bool((r[:n] < 0).any()):
                raise ValueError("MBRDecoder: weights are non-negative numbers, sentence %d has %s" % (b0 + b, r[:n].tolist()))
        if sum(nr) == 0:
            return torch.zeros((0,), dtype=torch.float64, device=dev)
        return torch.cat([r[:n].to(dev) for r, n in zip(rows, nr)])

    def _expected_utility(self, cand, cand_len, cand_sent, nc, ref, ref_len, ref_off, nr, weights, dev):
        """the gains under `self.utility`: every pair of a sentence through score_pairs, then the weighted mean per candidate.  The
        two row maps come from the lists' shapes (nc, nr) by device arithmetic: no host read"""
        Rc, M = cand.shape[0], max(nr + [0])
        total = sum(c * r for c, r in zip(nc, nr))
        gain = torch.zeros((Rc,), dtype=torch.float64, device=dev)
        if total == 0:
            return gain
        sent = cand_sent.long()
        lo = ref_off.long()[:-1][sent]                                          # the first pseudo-reference row of each candidate
        n = (ref_off.long()[1:] - ref_off.long()[:-1])[sent]                    # and how many it has
        first = torch.cumsum(n, 0) - n                                          # the candidate's first pair
        hyp_row = torch.repeat_interleave(torch.arange(Rc, device=dev), n, output_size=total)
        k = torch.arange(total, device=dev) - first[hyp_row]                    # the pair's place in its candidate's list
        ref_row = lo[hyp_row] + k
        got = self.utility.score_pairs(cand, cand_len, hyp_row.int(), ref, ref_len, ref_row.int())
        utility = torch.zeros((Rc, M), dtype=torch.float64, device=dev)
        counts = torch.zeros((Rc, M), dtype=torch.bool, device=dev)
        utility[hyp_row, k] = got[getattr(self.utility, "utility_key", "sentence_chrf")]
        counts[hyp_row, k] = got["status"] == 0
        if weights is None:
            w = counts.double()
        else:
            wk = torch.zeros((Rc, M), dtype=torch.float64, device=dev)
            wk[hyp_row, k] = weights[ref_row]
            w = torch.where(counts, wk, torch.zeros_like(wk))
        mass = w.sum(1)
        return torch.where(mass > 0, (w * utility).sum(1) / torch.where(mass > 0, mass, torch.ones_like(mass)), gain)

    # ------------------------------------------------------------------ matrices
    @torch.no_grad()
    def expected_bleu(self, cand, cand_len, cand_sent, ref, ref_len, ref_off, weights=None, max_list=None):
        """cand [Rc, Hmax] and ref [Rr, Pmax] integer token matrices (device) with their lengths; cand_sent [Rc] the sentence of each
        candidate row; ref_off [B + 1]: the pseudo-references of sentence b are the rows ref_off[b] .. ref_off[b+1] - 1 of ref.  cand
        and ref may be the same tensor.  weights: None (uniform) or one non-negative number per row of ref.  max_list: the widest
        list M when the caller knows it; None reads it from ref_off, the only host read.  Returns device tensors:
          stats    int32 [Rc, M, 10], the ten numbers of every pair (zeros behind a sentence's list and for a refused pair);
          status   int32 [Rc, M], see STATUS;
          utility  float64 [Rc, M], bleu_scorer.sentence_bleu(stats);
          gain     float64 [Rc], the weighted mean of the utilities of the pairs with status 0: sum_k w U / sum_k w; 0 when that
                   weight is 0 (no such pair), -1 for a refused candidate (its length outside [0, Hmax], its sentence outside
                   [0, B), or its sentence's offsets no list);
          best     int64 [B], the first candidate row of the highest gain of every sentence, -1 for a sentence without candidates.
        Everything behind the kernel is torch on the device."""
        if cand.dim() != 2 or ref.dim() != 2:
            raise ValueError("MBRDecoder: candidates and pseudo-references must be [rows, width] matrices, got %s and %s"
                             % (tuple(cand.shape), tuple(ref.shape)))
        if cand.shape[1] > MAX_LEN or ref.shape[1] > MAX_LEN:
            raise ValueError("MBRDecoder: padded widths of at most %d tokens (S2T_MBR_MAX_LEN), got %d and %d"
                             % (MAX_LEN, cand.shape[1], ref.shape[1]))
        dev = cand.device
        same = ref is cand
        cand, cand_len = as_ints(cand, cand_len, dev)
        ref, ref_len = (cand, cand_len) if same else as_ints(ref, ref_len, dev)
        cand_sent, ref_off = cand_sent.to(device=dev, dtype=torch.int32), ref_off.to(device=dev, dtype=torch.int32)
        stats, status = K.bleu_pairs(cand, cand_len, cand_sent, ref, ref_len, ref_off, self.pad, self.eos, self.unk, max_list=max_list)
        Rc, M = status.shape
        B, Rr = ref_off.shape[0] - 1, ref.shape[0]
        utility = sentence_bleu(stats)
        # the lists, as the kernel reads them
        lo, hi = ref_off[:-1].long(), ref_off[1:].long()
        is_list = (lo >= 0) & (hi >= lo) & (hi <= Rr) & (hi - lo <= M)
        sent = cand_sent.long()
        in_batch = (sent >= 0) & (sent < B)
        s = torch.where(in_batch, sent, torch.zeros_like(sent))
        if B:
            has_list = in_batch & is_list[s]
            start, n = lo[s], (hi - lo)[s]
        else:
            has_list, start, n = in_batch, s, s
        refused = ~has_list | (cand_len < 0) | (cand_len > cand.shape[1])
        cols = torch.arange(M, device=dev)
        counts = (status == 0) & (cols[None, :] < n[:, None]) & ~refused[:, None]
        if weights is None:
            w = counts.double()
        else:
            weights = torch.as_tensor(weights, dtype=torch.float64, device=dev).reshape(-1)
            if weights.shape[0] != Rr:
                raise ValueError("MBRDecoder: one weight per pseudo-reference row, got %d for %d" % (weights.shape[0], Rr))
            rows = (start[:, None] + cols[None, :]).clamp(min=0, max=max(Rr - 1, 0))
            w = torch.where(counts, weights[rows] if Rr else torch.zeros_like(utility), torch.zeros_like(utility))
        mass = w.sum(1)
        gain = torch.where(mass > 0, (w * utility).sum(1) / torch.where(mass > 0, mass, torch.ones_like(mass)), torch.zeros_like(mass))
        gain = torch.where(refused, torch.full_like(gain, -1.0), gain)
        # the first row of every sentence's highest gain; row B collects the candidates outside the batch
        slot = torch.where(in_batch, sent, torch.full_like(sent, B))
        top = torch.full((B + 1,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce(0, slot, gain, "amax")
        rows = torch.arange(Rc, device=dev)
        first = torch.full((B + 1,), Rc, dtype=torch.int64, device=dev).scatter_reduce(
            0, slot, torch.where(gain == top[slot], rows, torch.full_like(rows, Rc)), "amin")
        best = torch.where(first[:B] < Rc, first[:B], torch.full_like(first[:B], -1))
        return {"stats": stats, "status": status, "utility": utility, "gain": gain, "best": best}
