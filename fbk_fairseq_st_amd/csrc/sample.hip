// s2t_sample_rows (include/s2t_hip.h): the draws of the sampling search for rows of log-probabilities -- what `Sampling.step`
// (sequence_generator.py) runs on the step-by-step route.  One workgroup of 1024 threads per row holds the row in registers (up to
// 32 columns per thread: V <= 32768), finds the kept set once and draws `draws` tokens from it, each with its own slot's uniforms.
// The function itself is sample.hpp, which the device-resident search (decode.hip) calls on the row it already holds.
#include "sample.hpp"
#include "s2t_hip.h"

namespace {
constexpr int NT = 1024;
template <int VPT>
__global__ __launch_bounds__(NT) void sample_rows_kernel(const float* __restrict__ x, int V, int ld, int draws, int topk, float topp,
                                                          unsigned long long key, int step, int* __restrict__ tok, float* __restrict__ lp_out,
                                                          int* __restrict__ n_kept) {
    __shared__ smp::Scratch sc;
    const int r = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (size_t)r * ld;
    float lp[VPT];
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int v = tid + i * NT;
        float a = v < V ? row[v] : -INFINITY;
        if (a != a) a = -INFINITY;                                 // NaN is -inf (sequence_generator.py:263)
        lp[i] = a + 0.f;                                           // -0 is +0: one image per value
    }
    int turn = 0;
    const smp::Kept k = smp::kept_set<VPT, NT>(lp, V, topk, topp, sc, turn);
    if (tid == 0) n_kept[r] = k.n;
    for (int j = 0; j < draws; ++j) {
        const int slot = r * draws + j;
        bool mine;
        float l;
        const int t = smp::draw<VPT, NT>(lp, k, smp::row_key(key, step, slot), sc, turn, mine, l);
        if (mine) { tok[slot] = t; lp_out[slot] = l; }
    }
}
}  // namespace

extern "C" int s2t_sample_rows(const float* lprobs, long rows, int V, int ld, int draws, int topk, float topp, unsigned long long key, int step,
                               int* tok, float* lp_out, int* n_kept, void* stream) {
    if (!lprobs || !tok || !lp_out || !n_kept || rows < 1 || draws < 1 || topk < 0 || topp != topp || V < 1 || ld < V || step < 0) return S2T_EINVAL;
    if (V > 32768 || rows * (long)draws > 0x7fffffffL) return S2T_ENOTSUP;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)rows);
#define SAMPLE_ROWS(VPT_) hipLaunchKernelGGL(sample_rows_kernel<VPT_>, grid, dim3(NT), 0, st, lprobs, V, ld, draws, topk, topp, key, step, tok, lp_out, n_kept)
    const int vpt = (V + NT - 1) / NT;
    if (vpt <= 1) SAMPLE_ROWS(1); else if (vpt <= 2) SAMPLE_ROWS(2); else if (vpt <= 4) SAMPLE_ROWS(4); else if (vpt <= 8) SAMPLE_ROWS(8);
    else if (vpt <= 16) SAMPLE_ROWS(16); else SAMPLE_ROWS(32);
#undef SAMPLE_ROWS
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
