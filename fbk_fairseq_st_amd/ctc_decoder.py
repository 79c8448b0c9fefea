"""CTC transcripts from the encoder's CTC head: greedy (best path) and prefix beam search, both on the device.

Every model of this package carries a CTC head over the transcript vocabulary -- `encoder.ctc_fc` of `--ctc-compress-out` models,
`ctc_aware_model.fc_out` of a `ctc_multi_loss` criterion for the others.  `CTCDecoder.generate(models, sample)` runs the encoder of
ONE model on the audio of `sample["net_input"]` and decodes the `ctc_out` it returns; `decode_logits(logits, in_len)` is the same
decoding for logits the caller made (the criterion's `fc_out` applied to an encoder state, for instance).  The reference has no
importable counterpart: its only CTC inference path (examples/speech_recognition/infer.py, w2l_decoder.py) needs the wav2letter
bindings.

  * strategy "greedy": per-frame arg-max (first index of the maximum), runs collapsed, blanks dropped -- what `ctc_acc` logging
    collapses on the host -- plus the frames every token was emitted on and its log-probability.
  * strategy "prefix": prefix beam search without a language model (Hannun et al. 2014; DESIGN.md states the rule), `beam_size`
    live prefixes, the `cand` most likely non-blank symbols per frame, the `nbest` best hypotheses.

The hot path is csrc/ctc_decode.hip (kernels.ctc_greedy / kernels.ctc_prefix_beam): two launches per call, no host read between
them; the one device-to-host copy of a call fetches the hypotheses' lengths at the end.  Like SequenceScorer, the class is handed to
`task.inference_step(decoder, models, sample)` in place of a generator; `registry.build_generator` does not build it.
"""
import torch

from . import kernels as K
from .ctc_head import blank_index, encoder_logits, single_model

STRATEGIES = ("greedy", "prefix")
MAX_BEAM = MAX_CAND = 16          # s2t_ctc_prefix_beam


class CTCDecoder:
    """src_dict: the transcript dictionary; the blank is its `<ctc_blank>` entry."""

    def __init__(self, src_dict, strategy="greedy", beam_size=8, cand=8, nbest=1):
        if strategy not in STRATEGIES:
            raise ValueError("strategy must be one of %s, got %r" % (", ".join(STRATEGIES), strategy))
        if strategy == "greedy" and nbest > 1:
            raise ValueError("strategy 'greedy' yields the one best path: nbest = %d needs strategy 'prefix'" % nbest)
        if strategy == "prefix" and not (1 <= nbest <= beam_size <= MAX_BEAM and 1 <= cand <= MAX_CAND):
            raise ValueError("prefix search takes 1 <= nbest <= beam_size <= %d and 1 <= cand <= %d, got nbest %d, beam_size %d, cand %d"
                             % (MAX_BEAM, MAX_CAND, nbest, beam_size, cand))
        self.blank = blank_index(src_dict)
        self.strategy, self.beam_size, self.cand, self.nbest = strategy, int(beam_size), int(cand), int(nbest)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        """per sentence a list of nbest dicts: `tokens` (int64, no blank, no EOS, may be empty), `score` (f32 0-dim device tensor: the
        best path's log-probability / the prefix' log-probability over all alignments), `positional_scores` and `frames` (greedy:
        f32 [n] and int32 [n, 2] = first frame, one past the last frame, in CTC frame units; prefix: None), `attention`, `alignment`
        (None)."""
        model = single_model(models, "CTCDecoder decodes the CTC head of exactly one model, got %d")
        return self.decode_logits(*encoder_logits(model, sample["net_input"], "decode_logits(logits, in_len)"))

    @torch.no_grad()
    def decode_logits(self, logits, in_len):
        """logits [T, B, V] time-major CTC logits (f32 / bf16, device), in_len [B] integer frames per sentence"""
        in_len = in_len.to(device=logits.device, dtype=torch.int32)
        B = logits.shape[1]
        if self.strategy == "greedy":
            tokens, n, frames, tok_score, score = K.ctc_greedy(logits, in_len, self.blank)
            tokens = tokens.long()
            counts = n.tolist()                                           # the call's one device-to-host copy
            return [[{"tokens": tokens[b, :k], "score": score[b], "positional_scores": tok_score[b, :k], "frames": frames[b, :k],
                      "attention": None, "alignment": None}] for b, k in zip(range(B), counts)]
        cand = min(self.cand, logits.shape[2] - 1)                        # a vocabulary smaller than the option: every symbol
        tokens, lens, scores, n_hyp = K.ctc_prefix_beam(logits, in_len, self.blank, self.beam_size, cand, self.nbest)
        tokens = tokens.long()
        host = torch.cat([lens.reshape(-1), n_hyp]).tolist()              # the call's one device-to-host copy
        lens_h, n_h = host[:B * self.nbest], host[B * self.nbest:]
        return [[{"tokens": tokens[b, i, :lens_h[b * self.nbest + i]], "score": scores[b, i], "positional_scores": None, "frames": None,
                  "attention": None, "alignment": None} for i in range(n_h[b])] for b in range(B)]
