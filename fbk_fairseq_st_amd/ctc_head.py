"""What CTCDecoder, CTCAligner and CTCSegmenter do alike in front of their kernels: the blank of the transcript dictionary, the one
model whose CTC head they read, and that head's logits for the audio of a batch."""
import contextlib

import torch


def blank_index(src_dict):
    """the dictionary's `<ctc_blank>` entry"""
    blank = src_dict.index("<ctc_blank>")
    if blank == src_dict.unk():
        raise ValueError("the dictionary has no <ctc_blank> entry")
    return blank


def single_model(models, message):
    """the one model of `models` (a model, or a list or tuple of one); message: the caller's error for any other count, with one %d"""
    models = list(models) if isinstance(models, (list, tuple)) else [models]
    if len(models) != 1:
        raise ValueError(message % len(models))
    return models[0]


@contextlib.contextmanager
def eval_mode(model):
    """the model in eval mode, and back in the mode it was in afterwards, also when the body raises"""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


def ctc_out(model, net_input, direct):
    """One encoder call on the audio of net_input: the `ctc_out` it returns ([T, B, V]) and its padding mask ([B, T], or None).
    direct: the caller's method for logits made elsewhere, with its arguments; the error for a model without `ctc_out` names it."""
    enc = model.encoder(**{k: v for k, v in net_input.items() if k in ("src_tokens", "src_lengths")})
    logits = getattr(enc, "ctc_out", None)
    if logits is None:
        raise ValueError("the encoder returned no ctc_out (a model built without --ctc-compress-out): apply the criterion's "
                         "fc_out to its encoder state and call %s" % direct)
    return logits, enc.ctc_padding_mask


def encoder_logits(model, net_input, direct):
    """ctc_out in eval mode -> (logits [T, B, V], in_len [B] int32: the frames the padding mask leaves every sentence)"""
    with eval_mode(model):
        logits, mask = ctc_out(model, net_input, direct)
    T, B = logits.shape[0], logits.shape[1]
    if mask is None:
        return logits, torch.full((B,), T, dtype=torch.int32, device=logits.device)
    return logits, (~mask).sum(1).to(torch.int32)
