#!/usr/bin/env python
"""The f32 oracle against its own float64 run, on the fp32 cases of tests/test_configs_gpu.py (host only, no GPU).

Prints, per case, the tensors on which the f32 oracle's element error (in units of the tensor's largest element) exceeds a quarter
of the fp32 bound FP32_NORTH_STAR: the figures test_configs_gpu.ref_only() is given at each test.  Both runs take the same
discrete decisions (CTC arg-max, ReLU active sets), so the figures are rounding only; they move by tens of percent with the host's
f32 summation order (thread count).

    python tools/parity_reference_noise.py [case ...]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

import numpy as np  # noqa: E402

import test_configs_gpu as C  # noqa: E402


def cases():
    rs = np.random.RandomState(5)
    ragged = tuple(sorted([1000] + [int(v) for v in rs.randint(300, 1000, 31)], reverse=True))
    mustc = tuple(C.mustc_lengths(4, 2))
    ctc = {
        "cfg2_s_fp32_32x1000": ("s2t_transformer_s", 32, 1000, 30, 12, None),
        "cfg2_s_fp32_32x1000_ragged": ("s2t_transformer_s", 32, 1000, 30, 13, ragged),
        "cfg3_m_ctc_compression_T1500": ("s2t_transformer_m", 2, 1500, 40, 3, None),
        "cfg3_m_ctc_compression_ragged": ("s2t_transformer_m", 3, 1500, 40, 4, (1500, 1210, 777)),
        "cfg4_l_mustc_shaped_lengths": ("s2t_transformer_l", 4, max(mustc), 24, 6, mustc),
    }
    out = {k: (lambda v=v: C.reference_pair(*v)["elem"]) for k, v in ctc.items()}
    out["cfg3_m_gelu_model_level"] = lambda: C.reference_pair("s2t_transformer_m", 2, 600, 20, 5, (600, 455), activation_fn="gelu",
                                                              encoder_layers=4, decoder_layers=2, ctc_layer=2)["elem"]
    out["cfg5_m_knowledge_distillation"] = lambda: C.reference_pair_of(C.KD_BUILD, C.kd_case)
    out["shared_decoder_input_output_embedding"] = lambda: C.reference_pair_of(C.SHARED_EMBED_BUILD, C.shared_embed_case)
    out["cfg5_m_dual_decoder_loss"] = lambda: C.reference_pair_of(C.DUAL_BUILD, C.dual_case)
    return out


def main(names):
    todo = cases()
    for name in names or todo:
        elem = todo[name]()
        over = sorted(((v, k) for k, v in elem.items() if v > C.FP32_NORTH_STAR / 4), reverse=True)
        print("%-40s %s" % (name, ", ".join("%s %.2e" % (k, v) for v, k in over) or "none above %.1e" % (C.FP32_NORTH_STAR / 4)), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
