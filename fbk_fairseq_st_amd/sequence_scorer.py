"""Teacher-forced scoring of reference translations (fairseq/sequence_scorer.py, generate.py --score-reference).

`SequenceScorer.generate(models, sample)` runs every model once on `sample["net_input"]` (which holds the shifted target as
`prev_output_tokens`) and returns, per sentence, the log-probability of every target token -- for an ensemble the log of the members'
mean probability.  The reference takes `get_normalized_probs` of every member ([B, L, V] in f32) and gathers one column per row;
here ONE kernel launch (kernels.score_targets, csrc/score.hip) reads the members' logits once and writes the [B, L] scores, so no
probability tensor exists at any point.

Deviations from the reference, both documented where they apply:
  * two or more members are combined in log space (max, sum of exp, log), the reference averages probabilities and takes the log at
    the end.  The two agree to rounding wherever the reference's probabilities are normal f32 numbers; where they underflow and the
    reference returns log(0) = -inf, this class stays finite.
  * `compute_alignment` works (see SequenceScorer): in the reference the option is dead for this model family.

It is handed to `task.inference_step(scorer, models, sample)` in place of a generator; `registry.build_generator` does not build it.
"""
import torch

from . import kernels as K
from .sequence_generator import hard_alignment

MAX_MEMBERS = 8          # s2t_score_targets takes up to eight members in one launch


def _support_end(attn):
    """attn (B, L, Ts) -> int64 [B]: one past the last encoder frame that holds any weight in any row"""
    used = (attn > 0).any(1)                                              # (B, Ts)
    idx = torch.arange(1, attn.shape[-1] + 1, device=attn.device)
    return (used * idx).amax(-1)


class SequenceScorer:
    """Scores the target for a given source sentence (fairseq/sequence_scorer.py:12-20).

    softmax_batch: accepted and without effect.  The reference uses it to bound the size of the softmax tensor it materialises; there
    is no such tensor here.
    compute_alignment: the decoder of this fairseq version returns `{"attn": [tensor]}`, a list, so the reference's
    `torch.is_tensor(attn)` test fails and its `attention` / `alignment` are None whatever the option says.  They are None by default
    here too.  With compute_alignment=True the decoders are asked for their encoder attention (need_attn=True), the members'
    (B, L, Ts) maps are averaged, every result carries `attention` as Ts x tgt_len (the orientation of the generator's hypotheses)
    and `alignment` from the rule of SequenceGenerator (sequence_generator.hard_alignment).  Members whose encoder outputs differ
    in length (CTC compression gives each model its own) are refused; more than 2,048 encoder frames raise the `not supported`
    error of s2t_attn_probs_avg."""

    def __init__(self, tgt_dict, softmax_batch=None, compute_alignment=False, eos=None):
        self.pad = tgt_dict.pad()
        self.eos = tgt_dict.eos() if eos is None else eos
        self.softmax_batch = softmax_batch
        assert softmax_batch is None or softmax_batch > 0
        self.compute_alignment = bool(compute_alignment)

    @torch.no_grad()
    def generate(self, models, sample, **kwargs):
        """Score a batch of translations: per sentence a list holding one dict with `tokens` (the target from start_indices[i] on,
        pad stripped), `positional_scores` (f32, one per token), `score` (their mean, an f32 device scalar), `attention`, `alignment`."""
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not 1 <= len(models) <= MAX_MEMBERS:
            raise ValueError("an ensemble of 1..%d models (s2t_score_targets), got %d" % (MAX_MEMBERS, len(models)))
        was_training = [m.training for m in models]
        for m in models:
            m.eval()                                                      # sequence_scorer.py:55
        try:
            return self._score(models, sample)
        finally:
            for m, t in zip(models, was_training):
                m.train(t)

    def _score(self, models, sample):
        net_input = sample["net_input"]
        target = sample["target"]
        extra = {"need_attn": True} if self.compute_alignment else {}
        logits, attns = [], []
        for m in models:
            out = m(**net_input, **extra)
            if not torch.is_tensor(out[0]):
                raise TypeError("%s returns one output per decoder: SequenceScorer scores models with a single decoder"
                                % type(m).__name__)
            logits.append(out[0])
            attn = out[1].get("attn") if len(out) > 1 and isinstance(out[1], dict) else None
            attns.append(attn[0] if isinstance(attn, (list, tuple)) and attn else attn)
        if len({x.dtype for x in logits}) > 1:
            raise ValueError("the members of an ensemble must share one compute dtype to be scored in one launch, got %s"
                             % ", ".join(str(x.dtype) for x in logits))
        avg_attn = None
        if self.compute_alignment:
            if any(a is None for a in attns):
                raise ValueError("compute_alignment: a member returned no encoder attention (a decoder without layers)")
            if len({a.shape[-1] for a in attns}) > 1:
                raise ValueError("compute_alignment: the members' encoder outputs differ in length (%s frames): their attention "
                                 "maps cannot be averaged" % ", ".join(str(a.shape[-1]) for a in attns))
            # the batch's width can agree while a sentence's own length does not: frames past a sentence's encoder length carry
            # exactly 0 in every row (s2t_attn_probs_avg), so a sentence's length is where its map's support ends
            ends = [_support_end(a) for a in attns]
            if any(not torch.equal(e, ends[0]) for e in ends[1:]):
                raise ValueError("compute_alignment: the members' encoder outputs differ in length (per sentence: %s): their "
                                 "attention maps cannot be averaged" % " against ".join(str(e.tolist()) for e in ends))
            avg_attn = attns[0].float() if len(attns) == 1 else torch.stack([a.float() for a in attns]).mean(0)
        scores = K.score_targets(logits, target)                          # f32 [B, L], one launch for all members

        bsz = target.shape[0]
        start_idxs = sample["start_indices"] if "start_indices" in sample else [0] * bsz
        hypos = []
        for i in range(bsz):                                              # sequence_scorer.py:96-127, its slices kept
            start = int(start_idxs[i])
            row = target[i, start:]
            ref = row[row.ne(self.pad)]                                   # utils.strip_pad
            tgt_len = ref.numel()
            pos = scores[i][start:start + tgt_len]
            attention = alignment = None
            if avg_attn is not None:
                attention = avg_attn[i][start:start + tgt_len].t()        # Ts x tgt_len
                alignment = hard_alignment(attention, ref, self.pad, self.eos)
            hypos.append([{"tokens": ref, "score": pos.sum() / tgt_len, "attention": attention, "alignment": alignment,
                           "positional_scores": pos}])
        return hypos
