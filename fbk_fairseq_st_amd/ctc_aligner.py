"""Forced alignment of known transcripts to the frames of the encoder's CTC head, on the device.

`CTCAligner.generate(models, sample)` runs the encoder of ONE model on the audio of `sample["net_input"]` and aligns
`sample["transcript_target"]` (with `sample["transcript_target_lengths"]`, the operands the criterion gives the CTC loss) to the
`ctc_out` it returns: the most likely CTC path among those that collapse to the transcript, with the frames every token occupies and
how well it fits.  `align_logits(logits, in_len, targets, tgt_len)` is the same alignment for logits the caller made.  It serves
time-stamping of transcripts, cutting recordings at token boundaries, filtering pairs whose transcript does not fit the audio
(`status`, `score`) and per-token confidences (`positional_scores`).  CTCDecoder's greedy strategy reports frames only for the
transcript it chose itself.

The hot path is csrc/ctc_align.hip (kernels.ctc_align; include/s2t_hip.h states the rule): two launches per call, no host read
between them; the one device-to-host copy of a call fetches status and lengths at the end.  Transcripts of at most MAX_TARGET tokens.
Like CTCDecoder, the class is handed to `task.inference_step(aligner, models, sample)` in place of a generator;
`registry.build_generator` does not build it.
"""
import torch

from . import kernels as K
from .ctc_head import blank_index, encoder_logits, single_model

MAX_TARGET = K.CTC_ALIGN_MAX_TARGET     # S2T_CTC_ALIGN_MAX_TARGET
SUBSAMPLING = 4                         # two stride-2 convolutions in front of the encoder
STATUS = {0: "aligned", 1: "no path: too few frames for the transcript, or a needed symbol has probability 0 everywhere",
          2: "refused: length outside the padded width, or a token that is the blank or outside the vocabulary"}


class CTCAligner:
    """src_dict: the transcript dictionary; the blank is its `<ctc_blank>` entry."""

    def __init__(self, src_dict):
        self.blank = blank_index(src_dict)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        """per sentence a one-element list holding the dict of align_logits, for sample["transcript_target"]"""
        model = single_model(models, "CTCAligner aligns to the CTC head of exactly one model, got %d")
        logits, in_len = encoder_logits(model, sample["net_input"], "align_logits(logits, in_len, targets, tgt_len)")
        return self.align_logits(logits, in_len, sample["transcript_target"], sample["transcript_target_lengths"])

    @torch.no_grad()
    def align_logits(self, logits, in_len, targets, tgt_len):
        """logits [T, B, V] time-major CTC logits (f32 / bf16, device), in_len [B] integer frames per sentence, targets [B, Lmax]
        integer transcripts, tgt_len [B] their lengths.  Per sentence a one-element list holding a dict: `tokens` (int64 [L], the
        transcript), `score` (f32 0-dim device tensor: the path's log-probability, blank frames included; -inf without a path),
        `positional_scores` (f32 [L]: each token's log-probability over its frames), `frames` (int32 [L, 2] = first frame, one past
        the last frame, in CTC frame units), `states` (int32 [n]: the state of the extended transcript on every frame, 2i + 1 =
        token i, even = blank; empty without a path), `status` (int: 0 aligned, 1 no path, 2 refused; see STATUS), `attention`,
        `alignment` (None)."""
        dev = logits.device
        if targets.dim() != 2 or targets.shape[1] > MAX_TARGET:
            raise ValueError("CTCAligner aligns transcripts of at most %d tokens (S2T_CTC_ALIGN_MAX_TARGET), got targets of shape %s"
                             % (MAX_TARGET, tuple(targets.shape)))
        in_len = in_len.to(device=dev, dtype=torch.int32)
        targets = targets.to(device=dev, dtype=torch.int64)
        tgt_len = tgt_len.to(device=dev, dtype=torch.int64)
        T, B, Lmax = logits.shape[0], logits.shape[1], targets.shape[1]
        states, frames, tok_score, score, status = K.ctc_align(logits, in_len, targets, tgt_len, self.blank)
        host = torch.cat([status.long(), tgt_len, in_len.long()]).tolist()      # the call's one device-to-host copy
        out = []
        for b in range(B):
            code, L, n = host[b], host[B + b], min(max(host[2 * B + b], 0), T)
            if not 0 <= L <= Lmax:
                L = 0                                                           # status 2: no usable length, nothing was written
            out.append([{"tokens": targets[b, :L], "score": score[b], "positional_scores": tok_score[b, :L], "frames": frames[b, :L],
                         "states": states[b, :n if code == 0 else 0], "status": int(code), "attention": None, "alignment": None}])
        return out


def input_frames(frames, src_lengths=None):
    """CTC frame ranges [..., 2] (first, one past the last) -> ranges of input feature frames: a CTC frame stands for SUBSAMPLING
    input frames.  With src_lengths (one length per leading index of `frames`, or a number) the ranges are clipped to the
    utterance; ranges of -1 (no path) stay -1."""
    out = frames * SUBSAMPLING
    if src_lengths is not None:
        lim = torch.as_tensor(src_lengths, device=frames.device)
        lim = lim.reshape(lim.shape + (1,) * (frames.dim() - lim.dim())).to(out.dtype)
        out = torch.minimum(out, lim)
    return torch.where(frames < 0, frames, out)
