"""Times the decoder-shaped attention calls (short queries) with dropout: python tools/attn_time_short_q.py
encoder-attention B 64, H 8, Tq 40, Tk 368 and causal self-attention T 40; forward and backward in us per call.
A/B against another build of the library: bash tools/ab_lib.sh <rounds> tools/attn_time_short_q.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from fbk_fairseq_st_amd import kernels as K
dev = "cuda"; B, H, d = 64, 8, 64; D = H * d
def timeit(fn, n=200):
    for _ in range(20): fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True); e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3
for name, Tq, Tk, causal in (("cross Tq40 Tk368", 40, 368, False), ("self T40 causal", 40, 40, True)):
    q = torch.randn(Tq, B, D, device=dev).to(torch.bfloat16)
    kv = torch.randn(Tk, B, 2 * D, device=dev).to(torch.bfloat16)
    k, v = kv[:, :, :D], kv[:, :, D:]
    p = 0.1
    o, lse = K.attn_fwd(q, k, v, H, causal=causal, p_drop=p, seed=1)
    do = torch.randn_like(o); dq = torch.empty_like(q); dkv = torch.empty_like(kv)
    # back-to-back launches on one stream: the time per call is the kernels' own when the queue stays full
    tf = min(timeit(lambda: K.attn_fwd(q, k, v, H, causal=causal, p_drop=p, seed=1, out=o)) for _ in range(3))
    tb = min(timeit(lambda: K.attn_bwd(q, k, v, o, do, lse, H, dq, dkv[:, :, :D], dkv[:, :, D:], causal=causal, p_drop=p, seed=1)) for _ in range(3))
    print("%-18s p_drop=%.1f  fwd %.1f us  bwd %.1f us" % (name, p, tf, tb))
