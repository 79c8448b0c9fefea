"""Cutting long recordings at utterance boundaries with the encoder's CTC head, on the device.

A recording of tens of minutes comes with its transcript as a list of sentences.  `CTCSegmenter.generate(models, sample)` runs the
encoder of ONE model over the recording in overlapping windows, aligns the concatenated sentences to the stitched CTC frames with
FREE ENDS -- applause, music and untranscribed speech before and after the text cost nothing -- and returns per sentence its frames
and three numbers that say how well it fits: the sum, the mean, and the lowest mean over any `window` consecutive frames, which finds a
sentence whose middle does not match the audio although its ends do.  `segment_logits(logits, in_len, utterances)` is the same for
logits the caller made, `logits_of_recording` the windowed encoder alone, `input_segments` the ranges in input feature frames.  The
reference side cut its corpora with an external forced aligner (examples/speech_recognition/scripts/resegment_data_mustc.py
post-processes its output); CTCAligner aligns one utterance, pinned at both ends, of at most 4,095 tokens.

The hot path is csrc/ctc_segment.hip (kernels.ctc_segment; include/s2t_hip.h states the rule): three launches per call, no host read
between them; the one device-to-host copy of a segment_logits call fetches statuses and lengths at the end.  At most MAX_TARGET tokens
and MAX_UTT utterances per recording; a batch is cut by recordings so that one call's workspace stays under WORKSPACE_LIMIT.  Like
CTCAligner, the class is handed to `task.inference_step(segmenter, models, sample)`; `registry.build_generator` does not build it.
"""
import torch

from . import kernels as K
from .ctc_aligner import SUBSAMPLING, input_frames
from .ctc_head import blank_index, ctc_out, eval_mode, single_model

MAX_TARGET = K.CTC_SEGMENT_MAX_TARGET   # S2T_CTC_SEGMENT_MAX_TARGET
MAX_UTT = K.CTC_SEGMENT_MAX_UTT         # S2T_CTC_SEGMENT_MAX_UTT
MAX_WINDOW = K.CTC_SEGMENT_MAX_WINDOW   # S2T_CTC_SEGMENT_MAX_WINDOW
WORKSPACE_LIMIT = 1 << 30               # bytes of workspace one call may ask for
STATUS = {0: "segmented", 1: "no path: too few frames for the transcript, or a needed symbol has probability 0 everywhere",
          2: "refused: tgt_len outside [1, Lmax], n_utt outside [1, Umax], offsets that are not strictly ascending from >= 1 to "
             "tgt_len, or one of the first L tokens equal to the blank or outside [0, V)"}


def workspace_bytes(T, B, Lmax):
    """the formula of s2t_ctc_segment_workspace: per (frame, recording) the row's maximum and log-sum-exp, the path's emission, and one
    dword of back-pointers per 16 states"""
    return (4 * T * B * (3 + (2 * Lmax + 1 + 15) // 16) + 255) // 256 * 256


class CTCSegmenter:
    """src_dict: the transcript dictionary; the blank is its `<ctc_blank>` entry.  window: the frames of the sliding mean behind
    `conf_min`.  free_start / free_end: the path may begin / end anywhere in the recording at no cost."""

    def __init__(self, src_dict, window=30, free_start=True, free_end=True):
        self.blank = blank_index(src_dict)
        self.window = int(window)
        if not 1 <= self.window <= MAX_WINDOW:
            raise ValueError("CTCSegmenter: window must lie in [1, %d] (S2T_CTC_SEGMENT_MAX_WINDOW), got %d" % (MAX_WINDOW, self.window))
        self.free_start, self.free_end = bool(free_start), bool(free_end)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        """sample["net_input"]: one long recording per row (src_tokens [B, frames, features], src_lengths [B]); sample["utterances"]:
        per recording its list of token tensors.  logits_of_recording for every row, then segment_logits."""
        model = single_model(models, "CTCSegmenter segments with the CTC head of exactly one model, got %d")
        src, lengths = sample["net_input"]["src_tokens"], sample["net_input"]["src_lengths"].tolist()
        parts = [self.logits_of_recording(model, src[b], lengths[b]) for b in range(src.shape[0])]
        T = max([n for _, n in parts] + [1])
        logits = parts[0][0].new_zeros((T, len(parts), parts[0][0].shape[2]))
        for b, (x, n) in enumerate(parts):
            logits[:n, b] = x[:, 0]
        in_len = torch.tensor([n for _, n in parts], dtype=torch.int32, device=logits.device)
        return self.segment_logits(logits, in_len, sample["utterances"])

    @staticmethod
    def window_plan(length, window_frames=2000, context_frames=200):
        """the windows of a recording of `length` input frames: a list of (start, stop, keep_from, keep_to).  [start, stop) are the
        input frames of a window; windows start at multiples of window_frames - 2 * context_frames.  Of the window's CTC frames the
        local range [keep_from, keep_to) is kept (keep_to None: to the window's end): context_frames / SUBSAMPLING are dropped at
        either side, except at the recording's own ends."""
        if window_frames % SUBSAMPLING or context_frames % SUBSAMPLING or context_frames < 0 or window_frames <= 2 * context_frames:
            raise ValueError("CTCSegmenter: window_frames and context_frames must be multiples of %d with window_frames > 2 * "
                             "context_frames, got %d and %d" % (SUBSAMPLING, window_frames, context_frames))
        step, c4 = window_frames - 2 * context_frames, context_frames // SUBSAMPLING
        starts = [0]
        while starts[-1] + window_frames < length:
            starts.append(starts[-1] + step)
        return [(s, min(s + window_frames, length), c4 if i else 0, None if i == len(starts) - 1 else (window_frames - context_frames) // SUBSAMPLING)
                for i, s in enumerate(starts)]

    @torch.no_grad()
    def logits_of_recording(self, model, features, length, window_frames=2000, context_frames=200, windows_per_call=8):
        """features [frames, feature size] of ONE recording, length its input frames.  Runs the encoder of a --ctc-compress-out model
        over the windows of window_plan, windows_per_call of them per encoder call, and stitches the kept `ctc_out` rows.  Returns
        (logits [n4, 1, V], n4)."""
        length = int(length)
        plan = self.window_plan(length, window_frames, context_frames)
        pieces = []
        with eval_mode(model):
            for c in range(0, len(plan), windows_per_call):
                chunk = plan[c:c + windows_per_call]
                width = max(stop - start for start, stop, _, _ in chunk)
                src = features.new_zeros((len(chunk), width, features.shape[1]))
                for i, (start, stop, _, _) in enumerate(chunk):
                    src[i, :stop - start] = features[start:stop]
                lens = torch.tensor([stop - start for start, stop, _, _ in chunk], dtype=torch.long, device=features.device)
                logits, _ = ctc_out(model, {"src_tokens": src, "src_lengths": lens}, "segment_logits(logits, in_len, utterances)")
                for i, (start, stop, lo, hi) in enumerate(chunk):
                    own = -(-(stop - start) // SUBSAMPLING)            # the CTC frames of the window's own input frames
                    pieces.append(logits[lo:own if hi is None else hi, i])
        out = torch.cat(pieces)[:, None]
        return out, out.shape[0]

    @staticmethod
    def chunk_recordings(T, lengths):
        """[start, stop) ranges of consecutive recordings (token counts `lengths`) whose call, padded to the longest transcript of the
        range, stays under WORKSPACE_LIMIT"""
        out, start, width = [], 0, 1
        for b, n in enumerate(lengths):
            n = min(max(int(n), 1), MAX_TARGET)
            if workspace_bytes(T, 1, n) > WORKSPACE_LIMIT:
                raise ValueError("CTCSegmenter: recording %d alone (%d frames, %d tokens) needs %d bytes of workspace, the limit is %d"
                                 % (b, T, n, workspace_bytes(T, 1, n), WORKSPACE_LIMIT))
            if b > start and workspace_bytes(T, b + 1 - start, max(width, n)) > WORKSPACE_LIMIT:
                out.append((start, b))
                start, width = b, 1
            width = max(width, n)
        if len(lengths) > start:
            out.append((start, len(lengths)))
        return out

    @torch.no_grad()
    def segment_logits(self, logits, in_len, utterances):
        """logits [T, B, V] time-major CTC logits (f32 / bf16, device), in_len [B] integer frames per recording, utterances: per
        recording a list of 1-D token tensors or lists, at least one token each.  Per recording a dict: `utterances` -- per utterance
        a dict of `tokens` (int64), `frames` (int32 [2]: first frame, one past the last, CTC frame units), `score` (the sum of the
        path's log-probabilities over that span), `conf_mean` (score / frames), `conf_min` (the lowest mean over `window`
        consecutive frames of the span), `positional_scores` (f32 per token), `token_frames` (int32 [tokens, 2]) -- and `score`
        (the whole path, free frames counting 0; -inf without a path), `states` (int32 [n]; empty without a path), `status`
        (0 segmented, 1 no path, 2 refused; see STATUS).  The utterances of a recording that was not segmented carry `tokens` only
        and None elsewhere."""
        dev = logits.device
        T, B = logits.shape[0], logits.shape[1]
        if len(utterances) != B:
            raise ValueError("CTCSegmenter: %d recordings of logits, %d lists of utterances" % (B, len(utterances)))
        # lengths are shapes: no host read.  A recording's tokens are concatenated where they lie (host lists and tensors in one
        # piece, then one copy; device tensors on the device)
        toks = [[torch.as_tensor(u, dtype=torch.int64).reshape(-1) for u in rec] for rec in utterances]
        lens = [[int(u.numel()) for u in rec] for rec in toks]
        for b, rec in enumerate(lens):
            if not 1 <= len(rec) <= MAX_UTT or min(rec) < 1:
                raise ValueError("CTCSegmenter: a recording has 1 to %d utterances (S2T_CTC_SEGMENT_MAX_UTT) of at least one token, recording "
                                 "%d has %d, the shortest of %d tokens" % (MAX_UTT, b, len(rec), min(rec) if rec else 0))
            if sum(rec) > MAX_TARGET:
                raise ValueError("CTCSegmenter: transcripts of at most %d tokens (S2T_CTC_SEGMENT_MAX_TARGET), recording %d has %d"
                                 % (MAX_TARGET, b, sum(rec)))
        total = [sum(rec) for rec in lens]
        in_len = in_len.to(device=dev, dtype=torch.int32)
        results, host = [], []
        for start, stop in self.chunk_recordings(T, total):
            nb = stop - start
            Lmax, Umax = max(total[start:stop]), max(len(rec) for rec in lens[start:stop])
            rows = [torch.cat(rec) if len({u.device for u in rec}) == 1 else torch.cat([u.to(dev) for u in rec]) for rec in toks[start:stop]]
            targets = torch.nn.utils.rnn.pad_sequence([r.to(dev) for r in rows], batch_first=True)
            utt_end = torch.zeros((nb, Umax), dtype=torch.int64)
            for i in range(nb):
                utt_end[i, :len(lens[start + i])] = torch.tensor(lens[start + i]).cumsum(0)
            utt_end = utt_end.to(dev)
            tgt_len = torch.tensor(total[start:stop], dtype=torch.int64, device=dev)
            n_utt = torch.tensor([len(rec) for rec in lens[start:stop]], dtype=torch.int64, device=dev)
            x = logits if nb == B else (logits[:, start:stop] if nb == 1 else logits[:, start:stop].contiguous())
            out = K.ctc_segment(x, in_len[start:stop], targets, tgt_len, utt_end, n_utt, self.blank, self.free_start, self.free_end, self.window)
            results.append((targets, utt_end) + tuple(out))
            host.append(out[-1])
        host = torch.cat([t.long() for t in host] + [in_len.long()]).tolist()      # the call's one device-to-host copy
        res = []
        for (start, stop), (targets, utt_end, states, frames, tok_score, score, u_frames, u_score, u_mean, u_min, _) in \
                zip(self.chunk_recordings(T, total), results):
            for i in range(stop - start):
                b = start + i
                code, n = host[b], min(max(host[B + b], 0), T)
                utts, lo = [], 0
                for u, cnt in enumerate(lens[b]):
                    d = {"tokens": targets[i, lo:lo + cnt]}
                    if code == 0:
                        d.update(frames=u_frames[i, u], score=u_score[i, u], conf_mean=u_mean[i, u], conf_min=u_min[i, u],
                                 positional_scores=tok_score[i, lo:lo + cnt], token_frames=frames[i, lo:lo + cnt])
                    else:
                        d.update(frames=None, score=None, conf_mean=None, conf_min=None, positional_scores=None, token_frames=None)
                    utts.append(d)
                    lo += cnt
                res.append({"utterances": utts, "score": score[i] if code != 2 else score.new_full((), float("-inf")),
                            "states": states[i, :n if code == 0 else 0], "status": int(code)})
        return res

    @staticmethod
    def input_segments(result, src_length, pad_frames=0):
        """result: one recording's dict of segment_logits; src_length: its input feature frames.  int64 [U, 2] ranges of input
        frames, one per utterance (ctc_aligner.input_frames of its CTC frames), widened by pad_frames at either side but never past
        the neighbouring utterance's token frames or the recording; None for a recording that was not segmented."""
        if result["status"] != 0:
            return None
        seg = input_frames(torch.stack([u["frames"] for u in result["utterances"]]).long(), int(src_length))
        lo, hi = seg[:, 0] - int(pad_frames), seg[:, 1] + int(pad_frames)
        floor = torch.cat([seg.new_zeros(1), seg[:-1, 1]])            # the end of the utterance before, the recording's start
        ceil = torch.cat([seg[1:, 0], seg.new_full((1,), int(src_length))])
        return torch.stack([torch.maximum(lo, floor), torch.minimum(hi, ceil)], 1)
