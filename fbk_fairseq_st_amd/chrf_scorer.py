"""chrF / chrF++ of detokenised hypotheses against references, on the device: the character and word n-gram statistics of every pair
of token rows (24 integers), the sentence score, and the corpus score from their sums.  DESIGN.md 5j and include/s2t_hip.h
(s2t_chrf_stats) state the rule; it is the rule sacrebleu's CHRF applies to whitespace-split text, restated -- sacrebleu itself was
never run beside this code.

Token ids become characters through a piece table: `piece_table(dictionary, bpe)` renders every symbol once, on the host, so that
the text of a row equals `" ".join(dictionary.string(row, bpe).split())` with pads left out; `ChrfScorer` puts the table on the
device once.  `score` takes two padded matrices, `score_hypotheses` the best hypothesis of every sentence of what
`SequenceGenerator.generate` returns, `score_nbest` every hypothesis of every sentence (the list shares its reference through a row
map), `score_pairs` any pairs of rows of two matrices named by two row maps -- nothing is copied or repeated.  Every call returns
per-pair device tensors and adds the sums of its finished pairs to a device accumulator; `result()` makes the object's one
device-to-host copy.

The hot path is csrc/chrf_stats.hip (kernels.chrf_stats): one launch per call, no host read.  Padded widths of at most MAX_LEN
tokens; a side of more than MAX_CHARS characters is refused by the kernel (status 2).
"""
import numpy as np
import torch

from . import kernels as K
from .token_rows import as_ints, best_rows, nbest_tables, pad_rows

MAX_LEN = K.CHRF_MAX_LEN                # S2T_CHRF_MAX_LEN
MAX_CHARS = K.CHRF_MAX_CHARS            # S2T_CHRF_MAX_CHARS
SEP = K.CHRF_SEP                        # S2T_CHRF_SEP
STATUS = {0: "done", 2: "refused: a row outside its matrix, a length outside the padded width, a token outside the dictionary, or "
                        "a side of more than %d characters" % MAX_CHARS}
_ORDERS = 8                             # six character orders, two word orders
_SUMS = tuple("%s%d_%s" % (kind, n, what) for kind, top in (("char", 6), ("word", 2)) for n in range(1, top + 1)
              for what in ("hyp", "ref", "match"))


def piece_table(dictionary, bpe="sentencepiece"):
    """dictionary: a Dictionary; bpe: None (every symbol is a word), "sentencepiece" (U+2581 is the word break) or a continuation
    marker that ends in one space, such as "@@ " (a symbol that ends in the marker loses it and joins the next one).  Returns a dict
    of host values: `pieces` (uint32 code points, SEP for a word break), `piece_off` (int32 [V + 2]; the piece of id t is
    pieces[piece_off[t] : piece_off[t + 1]], entry V is the reference-side rendering of unk, `unk_string(True)`), `V`, `unk` and `bpe`.
    pad, eos and bos have empty pieces.  ValueError for another bpe value and for a symbol that holds a whitespace character."""
    if bpe is None or bpe == "sentencepiece":
        marker = None
    elif isinstance(bpe, str) and len(bpe) >= 2 and bpe[-1] == " " and not any(c.isspace() for c in bpe[:-1]):
        marker = bpe[:-1]
    else:
        raise ValueError("piece_table: bpe is None, 'sentencepiece' or a marker that ends in one space such as '@@ ', got %r" % (bpe,))

    def render(sym, what):
        if any(c.isspace() for c in sym):
            raise ValueError("piece_table: %s %r holds a whitespace character" % (what, sym))
        if bpe is None:
            return [ord(c) for c in sym] + [SEP]
        if marker is None:
            return [SEP if c == "▁" else ord(c) for c in sym]
        return [ord(c) for c in sym[:-len(marker)]] if sym.endswith(marker) else [ord(c) for c in sym] + [SEP]

    V = len(dictionary)
    empty = {dictionary.pad(), dictionary.eos(), dictionary.bos()}
    pieces, off = [], [0]
    for t in range(V + 1):
        if t == V:
            pieces += render(dictionary.unk_string(True), "the reference-side unk")
        elif t == dictionary.unk():
            pieces += render(dictionary.unk_string(False), "the unk string")
        elif t not in empty:
            pieces += render(dictionary[t], "symbol %d" % t)
        off.append(len(pieces))
    return {"pieces": np.asarray(pieces, dtype=np.uint32), "piece_off": np.asarray(off, dtype=np.int32), "V": V,
            "unk": int(dictionary.unk()), "bpe": bpe}


class DeviceTable:
    """what `piece_table` returns, checked once and copied to each device once: the part ChrfScorer and TextErrorRate share.  who: the
    owner's name in the errors.  Also the table's extremes, which bound a row's units from its token width without a device read:
    `max_chars` (the characters of the longest piece), `max_breaks` (the most breaks in one piece) and `max_spaced` (the most
    characters plus breaks in one piece); entry V, the reference-side unk, is among them."""

    def __init__(self, table, who):
        pieces, off = np.asarray(table["pieces"]), np.asarray(table["piece_off"])
        self.V, self.unk = int(table["V"]), int(table["unk"])
        if pieces.dtype != np.uint32 or off.dtype != np.int32 or off.shape != (self.V + 2,) or not self.unk < self.V:
            raise ValueError("%s: the table is what piece_table returns: pieces uint32, piece_off int32 [V + 2], unk < V; got %s, %s %s, "
                             "V = %d, unk = %d" % (who, pieces.dtype, off.dtype, off.shape, self.V, self.unk))
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != pieces.shape[0]:
            raise ValueError("%s: piece_off must rise from 0 to the %d elements of pieces" % (who, pieces.shape[0]))
        breaks = np.concatenate([[0], np.cumsum(pieces == SEP)])[off]           # the breaks in front of every piece
        self.max_breaks = int(np.diff(breaks).max())
        self.max_chars = int((np.diff(off) - np.diff(breaks)).max())
        self.max_spaced = int(np.diff(off).max())
        self._host = (torch.from_numpy(pieces.view(np.int32).copy()), torch.from_numpy(off.copy()))
        self._on = {}

    def on(self, dev):
        """the table's two tensors on dev: copied there once"""
        key = str(dev)
        if key not in self._on:
            self._on[key] = tuple(t.to(dev) for t in self._host)
        return self._on[key]


class ChrfScorer:
    """table: what `piece_table` returns.  char_order 1 .. 6 and word_order 0 .. 2 (chrF is 6 and 0, chrF++ 6 and 2); beta weighs
    recall over precision.  A reference-side unk is rendered as the table's entry V and so matches nothing a hypothesis can hold."""

    def __init__(self, table, char_order=6, word_order=0, beta=2.0):
        self.char_order, self.word_order, self.beta = int(char_order), int(word_order), float(beta)
        if not 1 <= self.char_order <= K.CHRF_MAX_CHAR_ORDER:
            raise ValueError("ChrfScorer: char_order from 1 to %d (S2T_CHRF_MAX_CHAR_ORDER), got %r" % (K.CHRF_MAX_CHAR_ORDER, char_order))
        if not 0 <= self.word_order <= K.CHRF_MAX_WORD_ORDER:
            raise ValueError("ChrfScorer: word_order from 0 to %d (S2T_CHRF_MAX_WORD_ORDER), got %r" % (K.CHRF_MAX_WORD_ORDER, word_order))
        if not self.beta > 0:
            raise ValueError("ChrfScorer: beta must be positive, got %r" % (beta,))
        self.table = DeviceTable(table, "ChrfScorer")
        self.V, self.unk = self.table.V, self.table.unk
        self._acc = None

    @classmethod
    def for_dictionary(cls, tgt_dict, bpe="sentencepiece", char_order=6, word_order=0, beta=2.0):
        return cls(piece_table(tgt_dict, bpe), char_order=char_order, word_order=word_order, beta=beta)

    def table_on(self, dev):
        """the table's two tensors on dev: copied there once"""
        return self.table.on(dev)

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def score(self, hyp, hyp_len, ref, ref_len):
        """hyp [B, Hmax] and ref [B, Rmax] integer token matrices (device), hyp_len / ref_len [B] their lengths.  Returns a dict of
        per-pair device tensors: `stats` (int32 [B, 24]: hyp_n, ref_n, match_n of the character orders 1 .. 6, then of the word orders
        1 .. 2; zeros above the configured orders), `status` (see STATUS; the numbers of a refused pair are 0 and it adds nothing to
        the accumulator) and `sentence_chrf` (float64, in percent; 0 for a refused pair)."""
        if hyp.dim() != 2 or ref.dim() != 2 or hyp.shape[0] != ref.shape[0]:
            raise ValueError("ChrfScorer: hypotheses and references must be [B, width] matrices with one B, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        out = self._run(hyp, hyp_len, None, ref, ref_len, None)
        self._add(out["stats"].sum(0, dtype=torch.int64))
        return out

    @torch.no_grad()
    def score_hypotheses(self, hypos, ref, ref_len):
        """hypos: per sentence a list of dicts with `tokens` (1-D device tensors), best first; the best hypothesis of every sentence
        is scored (a sentence without one counts as empty).  Returns what `score` returns."""
        dev = ref.device
        best = best_rows(hypos, dev)
        if len(best) != ref.shape[0]:
            raise ValueError("ChrfScorer.score_hypotheses: %d sentences of hypotheses, %d references" % (len(best), ref.shape[0]))
        hyp, hyp_len = pad_rows(best, dev)
        return self.score(hyp, hyp_len, ref, ref_len)

    @torch.no_grad()
    def score_nbest(self, hypos, ref, ref_len, accumulate=None):
        """every hypothesis of every sentence against the sentence's reference, in one call.  Returns a dict of device tensors shaped
        [B, N] (N the longest list, at least 1) -- `stats` [B, N, 24], `status`, `sentence_chrf` -- with zeros, and -1 in
        `sentence_chrf`, behind `n_hyp` [B] (int64, the lists' lengths), and `oracle` [B] (int64), the first index of the highest
        sentence chrF (0 for a sentence without hypotheses).  accumulate: None adds nothing to the accumulator, "best" the stats of
        hypothesis 0 of every sentence, "oracle" those of hypothesis oracle[b]; a sentence without hypotheses adds nothing."""
        if accumulate not in (None, "best", "oracle"):
            raise ValueError("ChrfScorer.score_nbest: accumulate is None, 'best' or 'oracle', got %r" % (accumulate,))
        dev = ref.device
        B = len(hypos)
        if B != ref.shape[0]:
            raise ValueError("ChrfScorer.score_nbest: %d sentences of hypotheses, %d references" % (B, ref.shape[0]))
        stats, status, chrf, n_hyp, oracle, pick = nbest_tables(
            hypos, B, dev, lambda hyp, hyp_len, rows: self._run(hyp, hyp_len, None, ref, ref_len, rows), K.CHRF_STATS, "sentence_chrf")
        if accumulate is not None and B:
            self._add(pick(accumulate))
        return {"stats": stats, "status": status, "sentence_chrf": chrf, "n_hyp": n_hyp, "oracle": oracle}

    @torch.no_grad()
    def score_pairs(self, hyp, hyp_len, hyp_row, ref, ref_len, ref_row):
        """pair p is row hyp_row[p] of hyp [Hrows, Hmax] against row ref_row[p] of ref [Rrows, Rmax]; a map that is None means row p.
        hyp and ref may be the same matrix.  Returns what `score` returns, per pair, and adds the finished pairs' sums."""
        if hyp.dim() != 2 or ref.dim() != 2:
            raise ValueError("ChrfScorer: hypotheses and references must be [rows, width] matrices, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        out = self._run(hyp, hyp_len, hyp_row, ref, ref_len, ref_row)
        self._add(out["stats"].sum(0, dtype=torch.int64))
        return out

    def _run(self, hyp, hyp_len, hyp_row, ref, ref_len, ref_row):
        if hyp.shape[1] > MAX_LEN or ref.shape[1] > MAX_LEN:
            raise ValueError("ChrfScorer: padded widths of at most %d tokens (S2T_CHRF_MAX_LEN), got %d and %d"
                             % (MAX_LEN, hyp.shape[1], ref.shape[1]))
        dev = hyp.device
        same = ref is hyp
        hyp, hyp_len = as_ints(hyp, hyp_len, dev)
        ref, ref_len = (hyp, hyp_len) if same else as_ints(ref, ref_len, dev)
        hyp_row = None if hyp_row is None else hyp_row.to(device=dev, dtype=torch.int32)
        ref_row = None if ref_row is None else ref_row.to(device=dev, dtype=torch.int32)
        pieces, off = self.table_on(dev)
        stats, status = K.chrf_stats(hyp, hyp_len, ref, ref_len, pieces, off, unk=self.unk, char_order=self.char_order,
                                     word_order=self.word_order, hyp_row=hyp_row, ref_row=ref_row)
        return {"stats": stats, "status": status, "sentence_chrf": sentence_chrf(stats, self.char_order, self.word_order, self.beta)}

    # ------------------------------------------------------------------ accumulation
    def _add(self, sums):
        self._acc = sums if self._acc is None else self._acc + sums.to(self._acc.device)

    def result(self):
        """the 24 sums over every call since the last reset() (refused pairs left out), by name (char1_hyp, char1_ref, char1_match,
        ... word2_match), with `chrf` in percent from the sums by the rule of `sentence_chrf`, `precisions` and `recalls` (one per
        configured order, characters first; 0 where the total is 0) and `effective_order`, the orders that have n-grams on both
        sides.  The object's one device-to-host copy."""
        vals = [0] * len(_SUMS) if self._acc is None else self._acc.tolist()
        out = dict(zip(_SUMS, vals))
        out.update(_corpus(vals, self.char_order, self.word_order, self.beta))
        return out

    def result_string(self):
        """"chrF2 = 57.31", or "chrF2++ = ..." with word n-grams; the number behind chrF is beta"""
        return "chrF%g%s = %.2f" % (self.beta, "++" if self.word_order > 0 else "", self.result()["chrf"])

    def reset(self):
        self._acc = None


def _orders(char_order, word_order):
    return list(range(char_order)) + list(range(6, 6 + word_order))


def _corpus(vals, char_order, word_order, beta):
    """the score's rule on 24 host integers"""
    idx = _orders(char_order, word_order)
    hyp, ref, match = [vals[3 * k] for k in idx], [vals[3 * k + 1] for k in idx], [vals[3 * k + 2] for k in idx]
    prec = [m / h if h > 0 else 0.0 for m, h in zip(match, hyp)]
    rec = [m / r if r > 0 else 0.0 for m, r in zip(match, ref)]
    ok = [h > 0 and r > 0 for h, r in zip(hyp, ref)]
    eff = sum(ok)
    chrf = 0.0
    if eff:
        p = sum(x for x, o in zip(prec, ok) if o) / eff
        r = sum(x for x, o in zip(rec, ok) if o) / eff
        if p + r > 0:
            chrf = 100.0 * (1 + beta * beta) * p * r / (beta * beta * p + r)
    return {"chrf": chrf, "precisions": prec, "recalls": rec, "effective_order": eff}


def sentence_chrf(stats, char_order=6, word_order=0, beta=2.0):
    """stats [..., 24] integers -> float64 [...], in percent: over the configured orders that have n-grams on both sides, P the mean
    of match / hyp and R the mean of match / ref; 100 (1 + beta^2) P R / (beta^2 P + R), 0 without such an order or with P + R = 0"""
    s = stats.double().reshape(tuple(stats.shape[:-1]) + (_ORDERS, 3))
    s = s[..., _orders(int(char_order), int(word_order)), :]
    hyp, ref, match = s[..., 0], s[..., 1], s[..., 2]
    ok = (hyp > 0) & (ref > 0)
    one, zero = torch.ones_like(hyp), torch.zeros_like(hyp)
    eff = ok.sum(-1).double()
    n = torch.where(eff > 0, eff, torch.ones_like(eff))
    p = torch.where(ok, match / torch.where(ok, hyp, one), zero).sum(-1) / n
    r = torch.where(ok, match / torch.where(ok, ref, one), zero).sum(-1) / n
    b2 = float(beta) * float(beta)
    den = b2 * p + r
    some = den > 0
    return torch.where(some, 100.0 * (1 + b2) * p * r / torch.where(some, den, torch.ones_like(den)), torch.zeros_like(den))
