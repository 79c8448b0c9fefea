"""WER and CER of detokenised hypotheses against references, on the device: substitutions, insertions and deletions from the plain
Levenshtein alignment of the two texts' words or characters, per pair and summed.  DESIGN.md 5k and include/s2t_hip.h
(s2t_text_units) state the rule: the text of a token row is what `Dictionary.string` gives (chrf_scorer.piece_table),
words are its whitespace-split parts -- the words the reference's examples/speech_recognition/infer.py counts -- and characters are
its code points, with one space between words ("char", how ESPnet and jiwer count CER) or without ("char_nospace").  There is no
punctuation or case normaliser.

Every scoring call is two launches and no host read: csrc/text_units.hip (kernels.text_units) turns each pair of token rows into two
int32 unit rows, csrc/edit_align.hip (kernels.edit_align) aligns them under the costs (1, 1, 1) with the reference's tie rule.  The
methods mean what they mean on `ChrfScorer`: `score` takes two padded matrices, `score_hypotheses` the best hypothesis of every
sentence of what `SequenceGenerator.generate` or `CTCDecoder.generate` returns, `score_nbest` every hypothesis of every sentence,
`score_pairs` any pairs of rows of two matrices named by two row maps.  Every call returns per-pair device tensors and adds the sums
of its finished pairs to a device accumulator; `result()` makes the object's one device-to-host copy.

`MBRDecoder(generator, pad, eos, unk, utility=TextErrorRate(...))` selects by expected word or character accuracy: the object names
its pair score (`utility_key`) and the bytes a pair costs (`pair_bytes`).

Padded widths of at most MAX_LEN tokens; the unit rows' widths follow from the token widths and the table on the host
(`unit_width`), at most MAX_UNITS; a side that exceeds its width is refused by the kernel (status 2).
"""
import torch

from . import kernels as K
from .chrf_scorer import DeviceTable, piece_table
from .error_rate import OPS, ErrorRate  # noqa: F401  (OPS: the step codes of `ops`)
from .token_rows import as_ints, best_rows, nbest_tables, pad_rows

MAX_LEN = K.CHRF_MAX_LEN                # S2T_CHRF_MAX_LEN
MAX_UNITS = K.TEXT_MAX_UNITS            # S2T_TEXT_MAX_UNITS
UNITS = tuple(K.TEXT_MODES)             # "word", "char", "char_nospace"
STATUS = {0: "done", 2: "refused: a row outside its matrix, a length outside the padded width, a token outside the dictionary, a side "
                        "of more than %d characters, or a side with more units than its width" % K.CHRF_MAX_CHARS}
_SUMS = ("errors", "substitutions", "insertions", "deletions", "ref_units", "hyp_units", "pairs")
_COLS = _SUMS + ("matches",)            # the columns of a pair's integer record: the sums, then what is not summed
_FIELDS = {"errors": "errors", "substitutions": "substitutions", "insertions": "insertions", "deletions": "deletions",
           "ref_units": "ref_units_n", "hyp_units": "hyp_units_n", "matches": "matches"}      # column -> the name of its per-pair tensor


class TextErrorRate:
    """table: what `chrf_scorer.piece_table` returns.  unit: "word" (WER), "char" (CER with one space between words) or
    "char_nospace".  max_units: a cap on the unit rows' widths below MAX_UNITS (memory: a pair's unit rows are 4 (Uh + Ur) bytes).  A
    reference-side unk is rendered as the table's entry V and so equals nothing a hypothesis can hold."""

    utility_key = "sentence_accuracy"   # the pair score MBRDecoder reads: in [0, 100], 0 worst

    def __init__(self, table, unit="word", max_units=None):
        if unit not in K.TEXT_MODES:
            raise ValueError("TextErrorRate: unit is one of %s, got %r" % (", ".join(repr(u) for u in UNITS), unit))
        self.unit, self.mode = unit, K.TEXT_MODES[unit]
        self.max_units = MAX_UNITS if max_units is None else int(max_units)
        if not 0 <= self.max_units <= MAX_UNITS:
            raise ValueError("TextErrorRate: max_units from 0 to %d (S2T_TEXT_MAX_UNITS), got %r" % (MAX_UNITS, max_units))
        self.table = DeviceTable(table, "TextErrorRate")
        self.V, self.unk = self.table.V, self.table.unk
        self._acc = None

    @classmethod
    def for_dictionary(cls, tgt_dict, bpe="sentencepiece", unit="word", max_units=None):
        return cls(piece_table(tgt_dict, bpe), unit=unit, max_units=max_units)

    def table_on(self, dev):
        """the table's two tensors on dev: copied there once"""
        return self.table.on(dev)

    def unit_width(self, token_width, side="hyp"):
        """the width of the unit rows of a side ("hyp" or "ref": one bound serves both, entry V included) whose token matrix is
        token_width wide: no row of that width has more units, from the table alone.  Words: every word but the first follows a
        break, so at most token_width * max(1, most breaks in one piece) + 1.  Characters: at most token_width * the longest piece;
        with spaces every break adds at most one, so token_width * the most characters plus breaks in one piece.  Clipped to MAX_UNITS
        and to max_units: a side that has more is the kernel's status 2."""
        if side not in ("hyp", "ref"):
            raise ValueError("TextErrorRate.unit_width: side is 'hyp' or 'ref', got %r" % (side,))
        n, t = int(token_width), self.table
        width = n * max(1, t.max_breaks) + 1 if self.mode == 0 else n * t.max_spaced if self.mode == 1 else n * t.max_chars
        return max(0, min(width, MAX_UNITS, self.max_units))

    def pair_bytes(self, hyp_token_width, ref_token_width):
        """the bytes a pair costs a call: the two unit rows and their lengths, the alignment's counts, cost and row count, two
        statuses, two row-map entries and the two float64 scores"""
        return 4 * (self.unit_width(hyp_token_width, "hyp") + self.unit_width(ref_token_width, "ref")) + 4 * 3 + 4 * 4 + 4 + 2 * 4 + 2 * 4 + 2 * 8

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def score(self, hyp, hyp_len, ref, ref_len, ops=False):
        """hyp [B, Hmax] and ref [B, Rmax] integer token matrices (device), hyp_len / ref_len [B] their lengths.  Returns a dict of
        per-pair device tensors: `substitutions`, `insertions` (hypothesis units left alone), `deletions` (reference units left
        alone), `matches`, `errors` (int32), `hyp_units_n`, `ref_units_n` (int32, the units of the two texts), `status` (see STATUS;
        the numbers of a refused pair are 0 and it adds nothing to the accumulator), `sentence_rate` (float64: 100 * errors /
        max(ref_units_n, 1), not capped; 0 for a refused pair) and `sentence_accuracy` (100 - min(rate, 100); 0 for a refused pair).
        With ops=True also `ops` (uint8 [B, Uh + Ur], error_rate.OPS codes over units; entries behind `n_ops` are not written),
        `n_ops`, and the unit rows `hyp_units` [B, Uh] and `ref_units` [B, Ur] (int32; entries behind hyp_units_n / ref_units_n are
        not written; word units are first-occurrence ids inside their pair)."""
        if hyp.dim() != 2 or ref.dim() != 2 or hyp.shape[0] != ref.shape[0]:
            raise ValueError("TextErrorRate: hypotheses and references must be [B, width] matrices with one B, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        out = self._run(hyp, hyp_len, None, ref, ref_len, None, ops)
        self._add(out.pop("record").sum(0, dtype=torch.int64)[:len(_SUMS)])
        return out

    @torch.no_grad()
    def score_hypotheses(self, hypos, ref, ref_len, ops=False):
        """hypos: per sentence a list of dicts with `tokens` (1-D device tensors), best first; the best hypothesis of every sentence
        is scored (a sentence without one counts as empty).  Returns what `score` returns."""
        dev = ref.device
        best = best_rows(hypos, dev)
        if len(best) != ref.shape[0]:
            raise ValueError("TextErrorRate.score_hypotheses: %d sentences of hypotheses, %d references" % (len(best), ref.shape[0]))
        hyp, hyp_len = pad_rows(best, dev)
        return self.score(hyp, hyp_len, ref, ref_len, ops=ops)

    @torch.no_grad()
    def score_nbest(self, hypos, ref, ref_len, accumulate=None):
        """every hypothesis of every sentence against the sentence's reference, in one call.  Returns a dict of device tensors shaped
        [B, N] (N the longest list, at least 1) -- the fields of `score` without ops -- with zeros, and -1 in `sentence_rate`,
        behind `n_hyp` [B] (int64, the lists' lengths), and `oracle` [B] (int64), the first index of the lowest sentence rate among
        the list's finished hypotheses (0 for a sentence without one).  accumulate: None adds nothing to the accumulator, "best" the
        numbers of hypothesis 0 of every sentence, "oracle" those of hypothesis oracle[b]; a sentence without hypotheses adds
        nothing."""
        if accumulate not in (None, "best", "oracle"):
            raise ValueError("TextErrorRate.score_nbest: accumulate is None, 'best' or 'oracle', got %r" % (accumulate,))
        dev = ref.device
        B = len(hypos)
        if B != ref.shape[0]:
            raise ValueError("TextErrorRate.score_nbest: %d sentences of hypotheses, %d references" % (B, ref.shape[0]))

        def run(hyp, hyp_len, rows):
            got = self._run(hyp, hyp_len, None, ref, ref_len, rows, False)
            return {"stats": got["record"], "status": got["status"], "sentence_rate": got["sentence_rate"]}
        record, status, rate, n_hyp, oracle, pick = nbest_tables(hypos, B, dev, run, len(_COLS), "sentence_rate", lowest=True)
        if accumulate is not None and B:
            self._add(pick(accumulate)[:len(_SUMS)])
        out = {name: record[..., _COLS.index(col)] for col, name in _FIELDS.items()}
        done = record[..., _COLS.index("pairs")] == 1
        out.update(status=status, sentence_rate=rate, n_hyp=n_hyp, oracle=oracle,
                   sentence_accuracy=torch.where(done, 100.0 - rate.clamp(max=100.0), torch.zeros_like(rate)))
        return out

    @torch.no_grad()
    def score_pairs(self, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, ops=False):
        """pair p is row hyp_row[p] of hyp [Hrows, Hmax] against row ref_row[p] of ref [Rrows, Rmax]; a map that is None means row p.
        hyp and ref may be the same matrix.  Returns what `score` returns, per pair, and adds the finished pairs' sums."""
        if hyp.dim() != 2 or ref.dim() != 2:
            raise ValueError("TextErrorRate: hypotheses and references must be [rows, width] matrices, got %s and %s"
                             % (tuple(hyp.shape), tuple(ref.shape)))
        out = self._run(hyp, hyp_len, hyp_row, ref, ref_len, ref_row, ops)
        self._add(out.pop("record").sum(0, dtype=torch.int64)[:len(_SUMS)])
        return out

    def _run(self, hyp, hyp_len, hyp_row, ref, ref_len, ref_row, ops):
        """the two launches: the fields of `score` plus `record`, int32 [P, len(_COLS)], the pair's integers in the order of _COLS"""
        if hyp.shape[1] > MAX_LEN or ref.shape[1] > MAX_LEN:
            raise ValueError("TextErrorRate: padded widths of at most %d tokens (S2T_CHRF_MAX_LEN), got %d and %d"
                             % (MAX_LEN, hyp.shape[1], ref.shape[1]))
        dev = hyp.device
        same = ref is hyp
        hyp, hyp_len = as_ints(hyp, hyp_len, dev)
        ref, ref_len = (hyp, hyp_len) if same else as_ints(ref, ref_len, dev)
        hyp_row = None if hyp_row is None else hyp_row.to(device=dev, dtype=torch.int32)
        ref_row = None if ref_row is None else ref_row.to(device=dev, dtype=torch.int32)
        pieces, off = self.table_on(dev)
        Uh, Ur = self.unit_width(hyp.shape[1], "hyp"), self.unit_width(ref.shape[1], "ref")
        hu, hn, ru, rn, refused = K.text_units(hyp, hyp_len, ref, ref_len, pieces, off, self.unk, self.mode, Uh, Ur, hyp_row=hyp_row, ref_row=ref_row)
        P = refused.shape[0]
        # the alignment's step storage is cut by pairs; pairs are independent: the chunks' results are the unchunked call's
        step = ErrorRate.chunk_sentences(Uh, Ur) if ops else max(P, 1)
        parts = [K.edit_align(hu[s:s + step], hn[s:s + step], ru[s:s + step], rn[s:s + step], (1, 1, 1), want_ops=ops)
                 for s in range(0, max(P, 1), step)]
        counts, _, aligned, _, _, op, n_ops = [None if p[0] is None else (p[0] if len(parts) == 1 else torch.cat(p)) for p in zip(*parts)]
        status = torch.where(refused != 0, refused, aligned)                    # a refused pair has no units: its alignment is zeros
        done = status == 0
        counts = counts * done[:, None].to(counts.dtype)
        errors = counts[:, 1:].sum(1, dtype=torch.int32)
        hyp_n, ref_n = hn * done.to(hn.dtype), rn * done.to(rn.dtype)
        rate = 100.0 * errors.double() / ref_n.clamp(min=1).double()
        out = {"matches": counts[:, 0], "substitutions": counts[:, 1], "deletions": counts[:, 2], "insertions": counts[:, 3],
               "errors": errors, "hyp_units_n": hyp_n, "ref_units_n": ref_n, "status": status, "sentence_rate": rate,
               "sentence_accuracy": torch.where(done, 100.0 - rate.clamp(max=100.0), torch.zeros_like(rate))}
        out["record"] = torch.stack([errors, out["substitutions"], out["insertions"], out["deletions"], ref_n, hyp_n,
                                     done.to(torch.int32), out["matches"]], 1)
        if ops:
            out.update(ops=op, n_ops=n_ops * done.to(n_ops.dtype), hyp_units=hu, ref_units=ru)
        return out

    # ------------------------------------------------------------------ accumulation
    def _add(self, sums):
        self._acc = sums if self._acc is None else self._acc + sums.to(self._acc.device)

    def result(self):
        """the sums over every call since the last reset() -- errors, substitutions, insertions, deletions, ref_units, hyp_units,
        pairs (refused pairs left out) -- with `rate` = 100 * errors / max(ref_units, 1) in percent, not capped, and `accuracy` =
        100 - min(rate, 100).  The object's one device-to-host copy."""
        vals = [0] * len(_SUMS) if self._acc is None else self._acc.tolist()
        out = dict(zip(_SUMS, vals))
        out["rate"] = 100.0 * out["errors"] / max(out["ref_units"], 1)
        out["accuracy"] = 100.0 - min(out["rate"], 100.0)
        return out

    def result_string(self):
        """"WER = 12.34 (S 10, D 3, I 2, N 122)"; CER for either character unit"""
        r = self.result()
        return "%s = %.2f (S %d, D %d, I %d, N %d)" % ("WER" if self.mode == 0 else "CER", r["rate"], r["substitutions"], r["deletions"],
                                                       r["insertions"], r["ref_units"])

    def reset(self):
        self._acc = None
