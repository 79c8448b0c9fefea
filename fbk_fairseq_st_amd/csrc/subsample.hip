// 2-D convolutional subsampler over (B, T, F=80) log-mel filterbanks: the HBM-bound pieces.
// Reference: examples/speech_recognition/models/conv_transformer.py:202-232 (+ :348-368):
//   2 x [ Conv2d(3x3, stride 2, pad 1) + bias -> act -> BatchNorm2d -> dropout ] -> flatten -> fc3 -> act -> + pos.
// Layout decisions (MI355X-first, not the reference's NCHW):
//   * activations are channels-last:  y1[b][t2][f2][c]  and  z2[t4][b][f4][c]  (c contiguous), so that
//     a wavefront = 64 channels of one pixel: coalesced 128-B stores, input taps broadcast, BatchNorm
//     statistics accumulate thread-locally (lane = channel) with no cross-lane reduction;
//   * conv1 (1 input channel, 9 MACs/output) is a direct VALU kernel bound by the y1 write;
//   * conv2 (64->64, 576 MACs/output) runs as an implicit GEMM on MFMA through s2t_gemm's row-gather
//     path (gemm.hip); this file only provides its BatchNorm / bias / index plumbing;
//   * fc3 consumes z2 directly: its weight is re-ordered once per step from the reference's
//     k = c*F4+f (conv_transformer.py:225-226) to k' = f*C+c (permute kernels below).
#include "common.hpp"
#include "prof.hpp"

// ------------------------------------------------------------------ 8-channel vectors
// Every HBM-bound kernel of this file gives a thread 8 consecutive channels of one pixel (one 16-byte bf16 access),
// so a wavefront instruction moves 1 KiB and a pixel is spread over LP = C/8 lanes; per-channel reductions first
// fold the lanes of a wave that own the same channel group (xor shuffles LP, 2LP, .. 32), then the four waves
// through LDS, then one atomic per channel per workgroup.
template <typename T> __device__ __forceinline__ void load8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void load8<bf16>(const bf16* p, float (&v)[8]) {
    bf16 t[8];
    *reinterpret_cast<u32x4*>(t) = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&v)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void store8<bf16>(bf16* p, const float (&v)[8]) {
    bf16 t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (bf16)v[e];
    *reinterpret_cast<u32x4*>(p) = *reinterpret_cast<const u32x4*>(t);
}
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&v)[8]) {
    *reinterpret_cast<f32x4*>(p) = (f32x4){v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = (f32x4){v[4], v[5], v[6], v[7]};
}
__device__ __forceinline__ float group_sum(float v, int LP) {          // over the lanes of a wave with equal lane % LP
    for (int o = LP; o < 64; o <<= 1) v += __shfl_xor(v, o);
    return v;
}
// per-channel pair of sums (s1, s2) of a workgroup of 256 threads -> sums[c] += s1, sums[C+c] += s2 (double atomics)
template <int NW = 4>
__device__ __forceinline__ void chan_pair_reduce(float (&s1)[8], float (&s2)[8], int LP, int g, double* sums, int C,
                                                 float (*red)[16][16]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = group_sum(s1[e], LP); s2[e] = group_sum(s2[e], LP); }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < LP) {
#pragma unroll
        for (int e = 0; e < 8; ++e) { red[wave][g][e] = s1[e]; red[wave][g][8 + e] = s2[e]; }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * C; t += NW * 64) {
        const int which = t / C, c = t % C;
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) a += (double)red[w][c >> 3][which * 8 + (c & 7)];
        atomicAdd(sums + which * C + c, a);
    }
}
// the 3x3 stride-2 window of output pixel (b, t2, f2) over x[b][Tin][F] (zero padding 1).  All nine loads are issued
// from clamped (always valid) addresses before any is used: left to itself the compiler sinks each load under its
// bounds test and waits for it there, i.e. nine serial memory latencies per pixel (seen in the ISA).
// Three 12-byte loads per pixel, one per window row (global_load_dwordx3 needs 4-byte alignment only) instead of nine 4-byte ones
// (forward 152 -> 134 us; the kernel's bound is its VALU work -- 72 FMAs + statistics per 8 channels of a pixel at ~40 % issue
// utilisation --, not bytes: 2.0 TB/s of useful traffic).  The three columns start at `fs` = fc - 1 clamped into the row; at the
// row's borders the wanted columns sit shifted inside the triple.
typedef float f32x3_t __attribute__((ext_vector_type(3)));
struct Conv1Win { f32x3_t r[3]; float mt0, mt2, mf0, mf2; int shift; };
__device__ __forceinline__ void conv1_window_issue(const float* __restrict__ x, unsigned p, int Tin, int F, int T2, int F2, Conv1Win& w) {
    const unsigned r = p / (unsigned)F2;
    const int f2 = (int)(p - r * F2), t2 = (int)(r % (unsigned)T2), b = (int)(r / (unsigned)T2);
    const int tc = 2 * t2, fc = 2 * f2;                       // centre tap: always inside
    const float* r1 = x + ((long)b * Tin + tc) * F;
    const float* r0 = r1 - (tc > 0 ? F : 0);
    const float* r2 = r1 + (tc + 1 < Tin ? F : 0);
    const int fs = min(max(fc - 1, 0), max(F - 3, 0));        // first column of the triple (F >= 3: checked on the host)
    w.shift = fc - 1 - fs;                                    // -1 at the left border, +1 at the right border of an odd row, else 0
    w.r[0] = *reinterpret_cast<const f32x3_t*>(r0 + fs);
    w.r[1] = *reinterpret_cast<const f32x3_t*>(r1 + fs);
    w.r[2] = *reinterpret_cast<const f32x3_t*>(r2 + fs);
    w.mt0 = tc > 0 ? 1.f : 0.f; w.mt2 = tc + 1 < Tin ? 1.f : 0.f;
    w.mf0 = fc > 0 ? 1.f : 0.f; w.mf2 = fc + 1 < F ? 1.f : 0.f;
}
__device__ __forceinline__ void conv1_window_finish(Conv1Win& w, float (&xv)[9]) {
    float v[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f32x3_t t = w.r[k];
        asm volatile("" : "+v"(t));
        // wanted columns fc-1, fc, fc+1 = triple index (0,1,2) + shift; out-of-row ones are masked to zero below, any value will do
        v[3 * k + 0] = w.shift > 0 ? t[1] : t[0];
        v[3 * k + 1] = w.shift < 0 ? t[0] : (w.shift > 0 ? t[2] : t[1]);
        v[3 * k + 2] = w.shift < 0 ? t[1] : t[2];
    }
    xv[0] = v[0] * (w.mt0 * w.mf0); xv[1] = v[1] * w.mt0; xv[2] = v[2] * (w.mt0 * w.mf2);
    xv[3] = v[3] * w.mf0;           xv[4] = v[4];         xv[5] = v[5] * w.mf2;
    xv[6] = v[6] * (w.mt2 * w.mf0); xv[7] = v[7] * w.mt2; xv[8] = v[8] * (w.mt2 * w.mf2);
}

// ------------------------------------------------------------------ conv1 forward (+ BN statistics) on the f32 matrix cores
// x [B][T][F] f32 -> y [B][T2][F2][C] T, y = act(conv(x)+bias); sums[c] += y, sums[C+c] += y^2 (double).  GELU (--activation-fn gelu): the
// pre-activation is stored next to y (`pre`), the backward needs it.
// The convolution as 16 x 16 x 4 f32 MFMAs (exact f32 products and sums: 7e-7 from a float64 evaluation): per unit of 16 consecutive
// output pixels, D[channel][pixel] = W[channel][tap] . X^T[tap][pixel] with the nine taps padded to 12 = three MFMAs per 16 channels.
// Lane (r16, q) of a wave supplies taps q, 4 + q, 8 + q of pixel r16 (three, two, two, two scalar loads) and receives channels
// 4q .. 4q + 3 of every 16-channel tile of that pixel: the 72 FMAs per 8 channels of a pixel that bound the round-1 kernel (8 channels per thread, 134 us)
// become 12 MFMAs per 16 pixels, and what is left per output value is bias, activation, rounding and the statistics (93 us).
// quotient and remainder of n < 2^24 by a runtime constant d (rcp = 1.f / d): a float multiply and a correction instead of the ~40
// instructions of a 32-bit division
__device__ __forceinline__ void divmod_small(unsigned n, unsigned d, float rcp, unsigned& qo, unsigned& ro) {     // n < 2^24
    unsigned qv = (unsigned)((float)n * rcp);
    int rr = (int)(n - qv * d);
    if (rr < 0) { qv -= 1; rr += (int)d; } else if (rr >= (int)d) { qv += 1; rr -= (int)d; }
    qo = qv; ro = (unsigned)rr;
}
struct Conv1Taps {                                    // this lane's three taps: row / column offsets and validity
    int dt[3], df[3]; bool on[3];
    __device__ __forceinline__ void init(int q) {
#pragma unroll
        for (int m = 0; m < 3; ++m) { const int k = 4 * m + q; on[m] = k < 9; dt[m] = k / 3 - 1; df[m] = k % 3 - 1; }
    }
};
// window values of pixel (b, t2, f2) for this lane's taps; out-of-plane taps read a clamped address and are zeroed by select
__device__ __forceinline__ void conv1_taps_load(const float* __restrict__ x, const Conv1Taps& tp, int b, int t2, int f2, int Tin, int F,
                                                bool live, float (&xv)[3]) {
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        const int t = 2 * t2 + tp.dt[m], f = 2 * f2 + tp.df[m];
        const bool ok = live && tp.on[m] && t >= 0 && t < Tin && f >= 0 && f < F;
        const float v = x[(unsigned)((b * Tin + min(max(t, 0), Tin - 1)) * F + min(max(f, 0), F - 1))];      // B T F < 2^31: checked on the host
        xv[m] = ok ? v : 0.f;
    }
}
template <int NT>
struct Conv1W {                                       // weight fragments: wa[j][m] = w[16 j + r16][4 m + q] (0 past the ninth tap)
    float wa[NT][3];
    __device__ __forceinline__ void init(const float* __restrict__ w, int r16, int q) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int m = 0; m < 3; ++m) wa[j][m] = 4 * m + q < 9 ? w[(16 * j + r16) * 9 + 4 * m + q] : 0.f;
    }
    __device__ __forceinline__ void mul(const float (&xv)[3], const f32x4 (&init)[NT], f32x4 (&acc)[NT]) const {     // acc = init + W . X^T
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            acc[j] = init[j];
#pragma unroll
            for (int m = 0; m < 3; ++m) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j][m], xv[m], acc[j], 0, 0, 0);
        }
    }
};

// forward: y = act(conv + bias) (+ pre for GELU) stored, statistics of the stored values.
// 8 waves per workgroup; a wave walks units of 16 pixels.  bf16 stores: the quads of two neighbouring 16-channel tiles are exchanged
// between lane rows q and q ^ 1 (v_permlane16_swap) so that every lane stores 8 consecutive channels = 16 bytes.
template <typename T, int NT, bool GELU>
__global__ __launch_bounds__(512) void conv1_mfma_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, T* __restrict__ y, T* __restrict__ pre,
                                                             double* __restrict__ sums, int B, int Tin, int F, int T2, int F2) {
    constexpr int C = 16 * NT;
    __shared__ float red[8][2][C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    Conv1Taps tp; tp.init(q);
    Conv1W<NT> cw; cw.init(w, r16, q);
    f32x4 b4[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) b4[j] = *reinterpret_cast<const f32x4*>(bias + 16 * j + 4 * q);
    float s1[NT][4], s2[NT][4];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) s1[j][e] = s2[j][e] = 0.f;
    const unsigned P = (unsigned)B * T2 * F2, units = (P + 15) / 16, stride = gridDim.x * 8;
    const bool small = P < (1u << 24);
    const float rF2 = 1.f / (float)F2, rT2 = 1.f / (float)T2;
    auto swap2 = [](uint32_t& a, uint32_t& b) {
        const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
        a = r[0]; b = r[1];
    };
    // the window values of the next unit are requested before this unit is consumed (a wave owns its units alone)
    float xn[3];
    auto issue = [&](unsigned u) {
        const unsigned p = u * 16 + r16, pc = min(p, P - 1);
        unsigned row, f2u, bu, t2u;
        if (small) { divmod_small(pc, (unsigned)F2, rF2, row, f2u); divmod_small(row, (unsigned)T2, rT2, bu, t2u); }
        else { row = pc / (unsigned)F2; f2u = pc - row * F2; bu = row / (unsigned)T2; t2u = row - bu * T2; }
        conv1_taps_load(x, tp, (int)bu, (int)t2u, (int)f2u, Tin, F, p < P, xn);
    };
    if (blockIdx.x * 8 + wave < units) issue(blockIdx.x * 8 + wave);
    for (unsigned u = blockIdx.x * 8 + wave; u < units; u += stride) {
        const unsigned p = u * 16 + r16;
        float xv[3] = {xn[0], xn[1], xn[2]};
        if (u + stride < units) issue(u + stride);
        f32x4 acc[NT];
        cw.mul(xv, b4, acc);                          // the bias is the accumulators' starting value
        const bool live = p < P;
        const bool full = u * 16 + 16 <= P;            // wave-uniform: every unit but (possibly) the last one
        uint32_t oq[NT][2], pq[NT][2];                 // packed bf16 quads (bf16 path)
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            T o[4], pr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = acc[j][e];
                if constexpr (GELU) { pr[e] = from_f32<T>(v); v = gelu_f(to_f32(pr[e])); }     // gelu of the stored pre-activation
                else v = fmaxf(v, 0.f);
                o[e] = from_f32<T>(v);
                const float r = (full || live) ? to_f32(o[e]) : 0.f;                          // statistics of the value that is stored
                s1[j][e] += r; s2[j][e] += r * r;
            }
            if constexpr (sizeof(T) == 4) {
                if (live) {
                    *reinterpret_cast<f32x4*>(y + (size_t)p * C + 16 * j + 4 * q) = *reinterpret_cast<const f32x4*>(o);
                    if constexpr (GELU) *reinterpret_cast<f32x4*>(pre + (size_t)p * C + 16 * j + 4 * q) = *reinterpret_cast<const f32x4*>(pr);
                }
            } else {
                oq[j][0] = reinterpret_cast<const uint32_t*>(o)[0]; oq[j][1] = reinterpret_cast<const uint32_t*>(o)[1];
                if constexpr (GELU) { pq[j][0] = reinterpret_cast<const uint32_t*>(pr)[0]; pq[j][1] = reinterpret_cast<const uint32_t*>(pr)[1]; }
            }
        }
        if constexpr (sizeof(T) == 2) {
#pragma unroll
            for (int pp = 0; pp < NT / 2; ++pp) {
                const size_t off = (size_t)p * C + 32 * pp + 16 * (q & 1) + 8 * (q >> 1);
                uint32_t a0 = oq[2 * pp][0], a1 = oq[2 * pp][1], a2 = oq[2 * pp + 1][0], a3 = oq[2 * pp + 1][1];
                swap2(a0, a2); swap2(a1, a3);
                if (live) *reinterpret_cast<u32x4*>(y + off) = (u32x4){a0, a1, a2, a3};
                if constexpr (GELU) {
                    uint32_t c0 = pq[2 * pp][0], c1 = pq[2 * pp][1], c2 = pq[2 * pp + 1][0], c3 = pq[2 * pp + 1][1];
                    swap2(c0, c2); swap2(c1, c3);
                    if (live) *reinterpret_cast<u32x4*>(pre + off) = (u32x4){c0, c1, c2, c3};
                }
            }
        }
    }
    // per-channel sums: over the 16 pixels of a lane row, then the 8 waves, then one double atomic per channel and workgroup
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float a = s1[j][e], b2 = s2[j][e];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) { a += __shfl_xor(a, o); b2 += __shfl_xor(b2, o); }
            if (r16 == 0) { red[wave][0][16 * j + 4 * q + e] = a; red[wave][1][16 * j + 4 * q + e] = b2; }
        }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * C; t += 512) {
        const int which = t / C, c = t % C;
        double a = 0.0;
#pragma unroll
        for (int wv = 0; wv < 8; ++wv) a += (double)red[wv][which][c];
        atomicAdd(sums + which * C + c, a);
    }
}

// ------------------------------------------------------------------ conv1 backward (weights, bias)
// dpre [B][T2][F2][C] T (gradient w.r.t. conv1 + bias, i.e. after the ReLU mask)
template <typename T>
__global__ __launch_bounds__(256) void conv1_bwd_kernel(const float* __restrict__ x, const T* __restrict__ dpre,
                                                        float* __restrict__ dw, float* __restrict__ db, int B,
                                                        int Tin, int F, int T2, int F2, int C, int pos_per_block) {
    __shared__ float red[4][16][80];
    const int LP = C >> 3, g = threadIdx.x % LP, slot = threadIdx.x / LP, nslot = 256 / LP;
    float a[8][10];
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < 10; ++i) a[e][i] = 0.f;
    const unsigned P = (unsigned)B * T2 * F2;
    const unsigned p0 = blockIdx.x * (unsigned)pos_per_block, pend = min(P, p0 + (unsigned)pos_per_block);
    Conv1Win wn;
    float gn[8];
    if (p0 + slot < pend) {
        conv1_window_issue(x, p0 + slot, Tin, F, T2, F2, wn);
        load8<T>(dpre + (size_t)(p0 + slot) * C + 8 * g, gn);
    }
    for (unsigned p = p0 + slot; p < pend; p += nslot) {
        float xv[9], gq[8];
        conv1_window_finish(wn, xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) gq[e] = gn[e];
        const unsigned pn = min(p + nslot, P - 1);
        conv1_window_issue(x, pn, Tin, F, T2, F2, wn);
        load8<T>(dpre + (size_t)pn * C + 8 * g, gn);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a[e][i] += gq[e] * xv[i];
            a[e][9] += gq[e];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const float v = group_sum(a[e][i], LP);
            if (lane < LP) red[wave][g][e * 10 + i] = v;
        }
    __syncthreads();
    for (int t = threadIdx.x; t < 10 * C; t += 256) {
        const int c = t / 10, i = t % 10;
        float v = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) v += red[wv][c >> 3][(c & 7) * 10 + i];
        if (i < 9) atomicAdd(dw + c * 9 + i, v); else atomicAdd(db + c, v);
    }
}


// BatchNorm backward + activation derivative + conv1 backward in ONE pass over (dyn, y): the gradient w.r.t. the convolution's
// output, dpre = act'(.) * gamma*rstd*(dyn - dbeta/N - xhat*dgamma/N), is formed in registers (two fmas per element from three
// per-channel constants) and consumed by the weight / bias sums at once -- it was a 245 MB tensor written by s2t_bn_bwd_apply and
// read back by s2t_conv1_bwd (153 + 148 us).  Also adds the BatchNorm parameter gradients (block 0), as s2t_bn_bwd_apply does.
template <typename T, bool GELU>
__global__ __launch_bounds__(256) void conv1_bwd_bn_kernel(const float* __restrict__ x, const T* __restrict__ dyn, const T* __restrict__ y,
                                                           const T* __restrict__ pre, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const double* __restrict__ sums, float* __restrict__ dw,
                                                           float* __restrict__ db, float* dgamma, float* dbeta, int B, int Tin, int F, int T2, int F2,
                                                           int C, int pos_per_block, double count, int training) {
    __shared__ float red[4][16][80];
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < C; c += 256) {
            atomicAdd(dbeta + c, (float)sums[c]);
            atomicAdd(dgamma + c, (float)sums[C + c]);
        }
    }
    const int LP = C >> 3, g = threadIdx.x % LP, slot = threadIdx.x / LP, nslot = 256 / LP;
    // dpre = act' * (ka * dyn + kb * y + kc):  ka = gamma*rstd, kb = -ka*m2*rstd, kc = ka*(m2*rstd*mean - m1)   (m1, m2 = dbeta/N, dgamma/N)
    float ka[8], kb[8], kc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        const float rs = rstd[c], mu = mean[c];
        const float m1 = training ? (float)(sums[c] / count) : 0.f, m2 = training ? (float)(sums[C + c] / count) : 0.f;
        ka[e] = gamma[c] * rs; kb[e] = -ka[e] * m2 * rs; kc[e] = ka[e] * (m2 * rs * mu - m1);
    }
    float a[8][10];
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < 10; ++i) a[e][i] = 0.f;
    const unsigned P = (unsigned)B * T2 * F2;
    const unsigned p0 = blockIdx.x * (unsigned)pos_per_block, pend = min(P, p0 + (unsigned)pos_per_block);
    Conv1Win wn;
    float dn[8], yn[8], qn[8];
    if (p0 + slot < pend) {
        conv1_window_issue(x, p0 + slot, Tin, F, T2, F2, wn);
        load8<T>(dyn + (size_t)(p0 + slot) * C + 8 * g, dn);
        load8<T>(y + (size_t)(p0 + slot) * C + 8 * g, yn);
        if constexpr (GELU) load8<T>(pre + (size_t)(p0 + slot) * C + 8 * g, qn);
    }
    for (unsigned p = p0 + slot; p < pend; p += nslot) {
        float xv[9], gq[8];
        conv1_window_finish(wn, xv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float r = __builtin_fmaf(ka[e], dn[e], __builtin_fmaf(kb[e], yn[e], kc[e]));
            if constexpr (GELU) gq[e] = r * gelu_grad_f(qn[e]);
            else gq[e] = yn[e] > 0.f ? r : 0.f;
        }
        const unsigned pn = min(p + nslot, P - 1);
        conv1_window_issue(x, pn, Tin, F, T2, F2, wn);
        load8<T>(dyn + (size_t)pn * C + 8 * g, dn);
        load8<T>(y + (size_t)pn * C + 8 * g, yn);
        if constexpr (GELU) load8<T>(pre + (size_t)pn * C + 8 * g, qn);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
#pragma unroll
            for (int i = 0; i < 9; ++i) a[e][i] += gq[e] * xv[i];
            a[e][9] += gq[e];
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int i = 0; i < 10; ++i) {
            const float v = group_sum(a[e][i], LP);
            if (lane < LP) red[wave][g][e * 10 + i] = v;
        }
    __syncthreads();
    for (int t = threadIdx.x; t < 10 * C; t += 256) {
        const int c = t / 10, i = t % 10;
        float v = 0.f;
#pragma unroll
        for (int wv = 0; wv < 4; ++wv) v += red[wv][c >> 3][(c & 7) * 10 + i];
        if (i < 9) atomicAdd(dw + c * 9 + i, v); else atomicAdd(db + c, v);
    }
}

// The same pass on the f32 matrix cores.  Per unit of 16 pixels a wave stages the [16 pixels][C] tiles of dyn and y (and pre) through a
// private LDS region so that lane (r16, q) holds, for channel 16 j + r16 of every 16-channel tile j, the four pixels 4q .. 4q + 3; dpre is
// formed there (three per-channel constants per tile) and is at once the B operand of  dW^T[tap][channel] += X^T[tap][pixel] . dpre[pixel]
// [channel]  as four 16 x 16 x 4 f32 MFMAs per tile (instruction e contracts the pixels 4k + e, k = 0..3; lane (tap r16, q) loads
// x of pixel 4q + e for tap r16).  16 accumulator registers per lane where the FMA form above keeps 80 (2 waves per SIMD, 188 us for
// 520 MB): this one runs at the occupancy of a streaming kernel.  Workgroup sums go out as partials (chan_partials_f32_kernel).
template <typename T, int NT, bool GELU>
__global__ __launch_bounds__(256) void conv1_bwd_bn_mfma_kernel(const float* __restrict__ x, const T* __restrict__ dyn, const T* __restrict__ y,
                                                                const T* __restrict__ pre, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const double* __restrict__ sums, float* __restrict__ part, float* dgamma,
                                                                float* dbeta, int B, int Tin, int F, int T2, int F2, double count, int training) {
    constexpr int C = 16 * NT, EPV = 16 / (int)sizeof(T), VPP = C / EPV, RSB = C * (int)sizeof(T) + 16, NTEN = GELU ? 3 : 2;
    extern __shared__ __attribute__((aligned(16))) char c1smem[];
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < C; c += 256) {
            atomicAdd(dbeta + c, (float)sums[c]);
            atomicAdd(dgamma + c, (float)sums[C + c]);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    char* tile = c1smem + wave * (NTEN * 16 * RSB);
    // dpre = act' * (ka * dyn + kb * y + kc):  ka = gamma*rstd, kb = -ka*m2*rstd, kc = ka*(m2*rstd*mean - m1)   (m1, m2 = dbeta/N, dgamma/N)
    float ka[NT], kb[NT], kc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = 16 * j + r16;
        const float rs = rstd[c], mu = mean[c];
        const float m1 = training ? (float)(sums[c] / count) : 0.f, m2 = training ? (float)(sums[C + c] / count) : 0.f;
        ka[j] = gamma[c] * rs; kb[j] = -ka[j] * m2 * rs; kc[j] = ka[j] * (m2 * rs * mu - m1);
    }
    const bool tap_on = r16 < 9;
    const int dt = r16 / 3 - 1, df = r16 % 3 - 1;                        // this lane's tap as the A operand
    f32x4 accT[NT];
    float dbs[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) { accT[j] = (f32x4){0.f, 0.f, 0.f, 0.f}; dbs[j] = 0.f; }
    const unsigned P = (unsigned)B * T2 * F2, units = (P + 15) / 16, stride = gridDim.x * 4;
    const float rF2 = 1.f / (float)F2, rT2 = 1.f / (float)T2;
    // One unit ahead: the 16-byte vectors of the next unit's tiles and its x values are requested before this unit is consumed (a wave
    // owns its units alone, nothing else would cover the memory latency between them).
    constexpr int NV = 16 * VPP / 64;                                    // vectors per lane and tensor
    u32x4 nd[NV], ny[NV], np_[GELU ? NV : 1];
    float nx[4];
    auto issue = [&](unsigned u) {
        const unsigned p0 = u * 16;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int v = 64 * k + lane, pix = v / VPP, ch = v % VPP;
            const bool in = p0 + pix < P;
            const size_t off = (size_t)(in ? p0 + pix : 0) * C + ch * EPV;
            nd[k] = *reinterpret_cast<const u32x4*>(dyn + off); ny[k] = *reinterpret_cast<const u32x4*>(y + off);
            if constexpr (GELU) np_[k] = *reinterpret_cast<const u32x4*>(pre + off);
        }
        unsigned row, f2u, bu, t2u;
        divmod_small(min(p0 + 4 * q, P - 1), (unsigned)F2, rF2, row, f2u);
        divmod_small(row, (unsigned)T2, rT2, bu, t2u);
        int f2 = (int)f2u, t2 = (int)t2u, b = (int)bu;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = 2 * t2 + dt, f = 2 * f2 + df;
            const bool ok = tap_on && p0 + 4 * q + e < P && t >= 0 && t < Tin && f >= 0 && f < F;
            const float v = x[((long)b * Tin + min(max(t, 0), Tin - 1)) * F + min(max(f, 0), F - 1)];
            nx[e] = ok ? v : 0.f;
            if (++f2 == F2) { f2 = 0; if (++t2 == T2) { t2 = 0; b = min(b + 1, B - 1); } }
        }
    };
    unsigned u = blockIdx.x * 4 + wave;
    if (u < units) issue(u);
    for (; u < units; u += stride) {
        const unsigned p0 = u * 16;
        // ---- this unit's tiles -> LDS (rows past P as zeros), its x values -> registers
        float xt[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xt[e] = nx[e];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int v = 64 * k + lane, pix = v / VPP, ch = v % VPP;
            const bool in = p0 + pix < P;
            const u32x4 z = {0u, 0u, 0u, 0u};
            *reinterpret_cast<u32x4*>(tile + pix * RSB + ch * 16) = in ? nd[k] : z;
            *reinterpret_cast<u32x4*>(tile + 16 * RSB + pix * RSB + ch * 16) = in ? ny[k] : z;
            if constexpr (GELU) *reinterpret_cast<u32x4*>(tile + 32 * RSB + pix * RSB + ch * 16) = in ? np_[k] : z;
        }
        if (u + stride < units) issue(u + stride);
        // the staged rows are read by OTHER lanes of this wave: LDS serves a wave's instructions in order; the asm keeps the compiler from
        // moving the reads above the writes (and, at the end of the body, the next unit's writes above these reads) without making
        // it wait for the global loads just issued
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        // ---- dpre per channel tile from the staged values; weight-gradient products
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int c = 16 * j + r16;
            // bf16: one transposed LDS read per tensor and tile -- the 16-lane group q addresses the 4 x 16 block (pixels 4q .. 4q + 3,
            // channels 16 j ..) in 8-byte pieces, lane r16 receives the four pixels of channel 16 j + r16 (ds_read_b64_tr_b16)
            T dq[4], yq[4], pq[4];
            if constexpr (sizeof(T) == 2) {
                typedef short s16x4_c1 __attribute__((ext_vector_type(4)));
                const char* a0 = tile + (4 * q + (r16 >> 2)) * RSB + (16 * j + 4 * (r16 & 3)) * 2;
                *reinterpret_cast<s16x4_c1*>(dq) = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_c1*)a0);
                *reinterpret_cast<s16x4_c1*>(yq) = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_c1*)(a0 + 16 * RSB));
                if constexpr (GELU) *reinterpret_cast<s16x4_c1*>(pq) = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_c1*)(a0 + 32 * RSB));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dq[e] = *reinterpret_cast<const T*>(tile + (4 * q + e) * RSB + c * (int)sizeof(T));
                    yq[e] = *reinterpret_cast<const T*>(tile + 16 * RSB + (4 * q + e) * RSB + c * (int)sizeof(T));
                    if constexpr (GELU) pq[e] = *reinterpret_cast<const T*>(tile + 32 * RSB + (4 * q + e) * RSB + c * (int)sizeof(T));
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int pix = 4 * q + e;
                const float dv = to_f32(dq[e]), yv = to_f32(yq[e]);
                const float r = __builtin_fmaf(ka[j], dv, __builtin_fmaf(kb[j], yv, kc[j]));
                float gq;
                if constexpr (GELU) gq = r * gelu_grad_f(to_f32(pq[e]));
                else gq = yv > 0.f ? r : 0.f;
                gq = p0 + pix < P ? gq : 0.f;
                dbs[j] += gq;
                accT[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(xt[e], gq, accT[j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    // ---- this workgroup's sums -> partials: part[blockIdx.x][c * 10 + tap] (tap 9 = bias gradient)
    __syncthreads();                                                     // every wave is done with its staging region
    float* red = reinterpret_cast<float*>(c1smem);                      // [4 waves][C * 10]
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int c = 16 * j + r16;
        float d = dbs[j];
        d += __shfl_xor(d, 16); d += __shfl_xor(d, 32);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * q + i < 9) red[wave * (C * 10) + c * 10 + 4 * q + i] = accT[j][i];
        if (q == 0) red[wave * (C * 10) + c * 10 + 9] = d;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 10 * C; t += 256)
        part[(size_t)blockIdx.x * (10 * C) + t] = (red[t] + red[C * 10 + t]) + (red[2 * C * 10 + t] + red[3 * C * 10 + t]);
}
// out(i) += sum over the workgroups' partials part[w][i], i = c * 10 + tap: taps 0..8 -> dw[c * 9 + tap], 9 -> db[c]; one workgroup per i
__global__ __launch_bounds__(256) void chan_partials_f32_kernel(const float* __restrict__ part, int nparts, int C, float* __restrict__ dw,
                                                                float* __restrict__ db) {
    __shared__ float sh[16];
    const int i = blockIdx.x;
    float a = 0.f;
    for (int w = threadIdx.x; w < nparts; w += 256) a += part[(size_t)w * (10 * C) + i];
    a = block_sum(a, sh);
    if (threadIdx.x == 0) { const int c = i / 10, tap = i % 10; if (tap < 9) dw[c * 9 + tap] += a; else db[c] += a; }
}

// ------------------------------------------------------------------ per-channel sums over [P][C]
// mode 0: sums[c] += y, sums[C+c] += y^2            (BatchNorm statistics)
// mode 1: sums[c] += dyn, sums[C+c] += dyn*xhat     (BatchNorm backward: dbeta, dgamma)
// NW waves per workgroup: every workgroup ends in 2 C double atomics on the same 2 C addresses, served one after the other at the
// memory side (~40 ns each) -- with 1024 four-wave workgroups that tail was 18 us of a 59 us pass; the big tensors run 256
// sixteen-wave workgroups (the same number of waves in flight, a quarter of the chain).
template <typename T, int NW>
__global__ __launch_bounds__(NW * 64) void chan_sums_kernel(const T* __restrict__ y, const T* __restrict__ dyn,
                                                        const float* __restrict__ mean, const float* __restrict__ rstd,
                                                        double* __restrict__ sums, long P, int C, int mode,
                                                        int pos_per_block) {
    __shared__ float red[NW][16][16];
    const int LP = C >> 3, g = threadIdx.x % LP, slot = threadIdx.x / LP, nslot = NW * 64 / LP;
    const long p0 = (long)blockIdx.x * pos_per_block;
    const long pend = min(P, p0 + (long)pos_per_block);
    float s1[8], s2[8], mu[8], rs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = s2[e] = 0.f; mu[e] = mode ? mean[8 * g + e] : 0.f; rs[e] = mode ? rstd[8 * g + e] : 0.f; }
    for (long p = p0 + slot; p < pend; p += nslot) {
        float v[8];
        load8<T>(y + p * C + 8 * g, v);
        if (mode == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { s1[e] += v[e]; s2[e] += v[e] * v[e]; }
        } else {
            float d[8];
            load8<T>(dyn + p * C + 8 * g, d);
#pragma unroll
            for (int e = 0; e < 8; ++e) { s1[e] += d[e]; s2[e] += d[e] * (v[e] - mu[e]) * rs[e]; }
        }
    }
    chan_pair_reduce<NW>(s1, s2, LP, g, sums, C, red);
}

// ------------------------------------------------------------------ BatchNorm finalize
// training: batch statistics from the double sums (biased variance normalises; running_var gets the
// unbiased one; momentum update; nn.BatchNorm2d semantics, conv_transformer.py:212,364-368)
// eval: running statistics.  Outputs mean, rstd, scale = gamma*rstd, shift = beta - mean*scale.
__global__ void bn_finalize_kernel(const double* sums, const float* gamma, const float* beta, float* run_mean,
                                   float* run_var, long long* num_batches, float* mean, float* rstd, float* scale,
                                   float* shift, double count, int C, int training, float momentum, float eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float mu, var;
    if (training) {
        const double m = sums[c] / count;
        double v = sums[C + c] / count - m * m;
        if (v < 0.0) v = 0.0;
        mu = (float)m; var = (float)v;
        const double unb = count > 1.0 ? v * (count / (count - 1.0)) : v;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mu;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
        if (c == 0 && num_batches) *num_batches += 1;
    } else { mu = run_mean[c]; var = run_var[c]; }
    const float rs = rsqrtf(var + eps);
    mean[c] = mu; rstd[c] = rs;
    scale[c] = gamma[c] * rs;
    shift[c] = beta[c] - mu * gamma[c] * rs;
}

// yn = y*scale[c] + shift[c]   ([P][C], c contiguous): 8 channels per thread; the grid stride is a multiple of C/8
// vectors, so a thread keeps its channel group (scale/shift stay in registers)
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ y, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, T* __restrict__ yn, long n, int C,
                                                       float p_drop, unsigned long long seed) {
    const int LP = C >> 3, g = threadIdx.x % LP;
    float sc[8], sh[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { sc[e] = scale[8 * g + e]; sh[e] = shift[8 * g + e]; }
    const long nv = n >> 3;
    const uint32_t th16 = (uint32_t)fminf(p_drop * 4294967296.f, 4294967295.f) >> 16;
    const float inv_keep = 1.f / (1.f - p_drop);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        float v[8];
        load8<T>(y + i * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = v[e] * sc[e] + sh[e];
        if (p_drop > 0.f) {                  // the dropout that follows the BatchNorm (conv_transformer.py:214): same mask and rounding as s2t_dropout on yn
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const u32x2 h = drop_hash4(seed, (uint64_t)i * 2 + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * k + e] = drop_field(h, e) >= th16 ? to_f32(from_f32<T>(v[4 * k + e])) * inv_keep : 0.f;
            }
        }
        store8<T>(yn + i * 8, v);
    }
}

// BatchNorm backward (training statistics) fused with the derivative of the preceding activation:
//   dy = gamma*rstd*(dyn - dbeta/N - xhat*dgamma/N);  dpre = dy * (y > 0)   (ReLU)   |   dy * gelu'(pre)   (GELU, pre != null)
// also accumulates dgamma/dbeta into the f32 parameter gradients (block 0).
template <typename T, bool GELU>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dyn, const T* __restrict__ y, const T* __restrict__ pre,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const double* __restrict__ sums,
                                                           T* __restrict__ dpre, float* dgamma, float* dbeta, long n,
                                                           int C, double count, int training) {
    if (blockIdx.x == 0) {
        for (int c = threadIdx.x; c < C; c += 256) {
            atomicAdd(dbeta + c, (float)sums[c]);
            atomicAdd(dgamma + c, (float)sums[C + c]);
        }
    }
    const int LP = C >> 3, g = threadIdx.x % LP;
    float k1[8], mu[8], rs[8], m1[8], m2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = 8 * g + e;
        mu[e] = mean[c]; rs[e] = rstd[c]; k1[e] = gamma[c] * rstd[c];
        m1[e] = training ? (float)(sums[c] / count) : 0.f;
        m2[e] = training ? (float)(sums[C + c] / count) : 0.f;
    }
    const long nv = n >> 3;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += (long)gridDim.x * 256) {
        float v[8], d[8], q[8];
        load8<T>(y + i * 8, v);
        load8<T>(dyn + i * 8, d);
        if constexpr (GELU) load8<T>(pre + i * 8, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float xh = (v[e] - mu[e]) * rs[e];
            const float r = k1[e] * (d[e] - m1[e] - xh * m2[e]);
            if constexpr (GELU) d[e] = r * gelu_grad_f(q[e]);
            else d[e] = v[e] > 0.f ? r : 0.f;
        }
        store8<T>(dpre + i * 8, d);
    }
}

// ------------------------------------------------------------------ weight re-ordering for channels-last
// mode 0 (fc3 forward):  dst[n][f*C+c]  = src[n][c*F+f]          (src f32 master -> dst T)
// mode 1 (fc3 grads):    dst[n][c*F+f] += src[n][f*C+c]          (src f32 -> dst f32 accumulate)
template <typename TD>
__global__ __launch_bounds__(256) void permute_cf_kernel(const float* __restrict__ src, TD* __restrict__ dst, int N, int C, int F, int mode) {
    const long n_el = (long)N * C * F;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {
        const int k = (int)(i % (C * F)); const long n = i / (C * F);
        if (mode == 0) { const int f = k / C, c = k % C; dst[i] = from_f32<TD>(src[n * C * F + c * F + f]); }
        else { const int c = k / F, f = k % F; dst[i] = from_f32<TD>(to_f32(dst[i]) + src[n * C * F + f * C + c]); }
    }
}
// conv2 weight [co][ci][3][3] (f32 master) <-> implicit-GEMM layouts
// mode 0: dst[co][tap*Ci+ci] = src[co][ci][tap]                       (forward B operand, T)
// mode 1: dst[ci][slot(tap)*Co+co] = src[co][ci][tap], class-major tap order (backward-data B operand, T)
// mode 2: dst[co][ci][tap] += src[co][tap*Ci+ci]                      (f32 grads back to the master layout)
__device__ __constant__ int kTapSlot[9] = {5, 3, 6, 1, 0, 2, 7, 4, 8};   // tap (kh*3+kw) -> class-major slot
template <typename TD>
__global__ __launch_bounds__(256) void permute_conv_w_kernel(const float* __restrict__ src, TD* __restrict__ dst, int Co, int Ci, int mode) {
    const long n_el = (long)Co * Ci * 9;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_el; i += (long)gridDim.x * 256) {
        if (mode == 0) {
            const int ci = (int)(i % Ci), tap = (int)((i / Ci) % 9), co = (int)(i / (9L * Ci));
            dst[i] = from_f32<TD>(src[((long)co * Ci + ci) * 9 + tap]);
        } else if (mode == 1) {
            const int co = (int)(i % Co), slot = (int)((i / Co) % 9), ci = (int)(i / (9L * Co));
            int tap = 0;
            for (int t = 0; t < 9; ++t) if (kTapSlot[t] == slot) tap = t;
            dst[i] = from_f32<TD>(src[((long)co * Ci + ci) * 9 + tap]);
        } else {
            const int tap = (int)(i % 9), ci = (int)((i / 9) % Ci), co = (int)(i / (9L * Ci));
            dst[i] = from_f32<TD>(to_f32(dst[i]) + src[(long)co * 9 * Ci + tap * Ci + ci]);
        }
    }
}

// ------------------------------------------------------------------ positional embedding add (+ dropout)
// dst[t][b][:] = dropout(src[t][b][:] + table[(t < len[b]) ? t+1 : 0][:])   (positional_embedding_audio.py:21-27 +
// sinusoidal_positional_embedding.py: positions 1..len, padding row 0 = zeros; conv_transformer.py:229-232: x += positions, then
// F.dropout); table is f32 [>=T+1][D].  One pass from the activation the backward keeps (src) to the encoder's input (dst); the mask
// is the one of s2t_dropout on the flat element index.  VEC: 16-byte accesses (D a multiple of the elements per access).
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void add_pos_kernel(const T* __restrict__ src, T* __restrict__ dst, const float* __restrict__ table,
                                                      const int* __restrict__ len, int Tn, int B, int D, float p, unsigned long long seed) {
    const uint32_t th = (uint32_t)fminf(p * 4294967296.f, 4294967295.f);
    const float inv = 1.f / (1.f - p);
    const long n = (long)Tn * B * D;
    if constexpr (VEC) {
        constexpr int E = 16 / (int)sizeof(T);
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n / E; i += (long)gridDim.x * 256) {
            const long e0 = i * E, row = e0 / D;
            const int d = (int)(e0 - row * D), b = (int)(row % B), t = (int)(row / B);
            const float* tab = table + (long)((t < len[b]) ? t + 1 : 0) * D + d;
            T v[E];
            *reinterpret_cast<u32x4*>(v) = *reinterpret_cast<const u32x4*>(src + e0);
#pragma unroll
            for (int k = 0; k < E / 4; ++k) {
                const f32x4 tb = *reinterpret_cast<const f32x4*>(tab + 4 * k);
                u32x2 h = {0u, 0u};
                if (p > 0.f) h = drop_hash4(seed, (uint64_t)i * (E / 4) + k);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = to_f32(from_f32<T>(to_f32(v[4 * k + e]) + tb[e]));          // rounded like the separate passes did
                    if (p > 0.f) x = drop_field(h, e) >= (th >> 16) ? x * inv : 0.f;
                    v[4 * k + e] = from_f32<T>(x);
                }
            }
            *reinterpret_cast<u32x4*>(dst + e0) = *reinterpret_cast<const u32x4*>(v);
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
            const int d = (int)(i % D), b = (int)((i / D) % B), t = (int)(i / ((long)D * B));
            const int pos = (t < len[b]) ? t + 1 : 0;
            float x = to_f32(from_f32<T>(to_f32(src[i]) + table[(long)pos * D + d]));
            if (p > 0.f) x = dropout_keep(seed, (uint64_t)i, th) ? x * inv : 0.f;
            dst[i] = from_f32<T>(x);
        }
    }
}

// ------------------------------------------------------------------ C ABI
static inline int nblocks(long n, int cap = 4096) { long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > cap ? cap : b)); }
#define DISPATCH_T(dtype, EXPR_BF16, EXPR_F32) \
    if ((dtype) == S2T_BF16) { EXPR_BF16; } else if ((dtype) == S2T_F32) { EXPR_F32; } else return S2T_ENOTSUP;

extern "C" int s2t_conv1_fwd(int dtype, const float* x, const float* w, const float* bias, void* y, void* pre, double* sums,
                             int B, int T, int F, int C, int act, void* stream) {
    if (B <= 0 || T <= 0) return S2T_OK;
    if (!x || !w || !bias || !y || !sums || (C != 64 && C != 128 && C != 32) || F < 3) return S2T_EINVAL;
    if ((act != ACT_RELU && act != ACT_GELU) || (act == ACT_GELU && !pre)) return S2T_EINVAL;
    if ((long)B * T * F >= (1l << 31)) return S2T_ENOTSUP;                   // 32-bit element offsets into x
    const int T2 = (T + 1) / 2, F2 = (F + 1) / 2;
    const long P = (long)B * T2 * F2;
    hipStream_t st = (hipStream_t)stream;
    const long units = (P + 15) / 16;
    dim3 grid((unsigned)(units < 8 * 512 ? (units + 7) / 8 : 512));          // 512 workgroups of 8 waves: each ends in 2C double atomics
#define S2T_C1(T_, NT_, G_) hipLaunchKernelGGL((conv1_mfma_fwd_kernel<T_, NT_, G_>), grid, dim3(512), 0, st, x, w, bias, (T_*)y, (T_*)pre, sums, B, T, F, T2, F2)
#define S2T_C1_NT(T_, G_) { if (C == 64) S2T_C1(T_, 4, G_); else if (C == 128) S2T_C1(T_, 8, G_); else S2T_C1(T_, 2, G_); }
    if (act == ACT_GELU) { DISPATCH_T(dtype, S2T_C1_NT(bf16, true), S2T_C1_NT(float, true)); }
    else { DISPATCH_T(dtype, S2T_C1_NT(bf16, false), S2T_C1_NT(float, false)); }
#undef S2T_C1_NT
#undef S2T_C1
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_conv1_bwd(int dtype, const float* x, const void* dpre, float* dw, float* db, int B, int T, int F,
                             int C, void* stream) {
    if (B <= 0 || T <= 0) return S2T_OK;
    if (!x || !dpre || !dw || !db || (C != 64 && C != 128 && C != 32) || F < 3) return S2T_EINVAL;
    const int T2 = (T + 1) / 2, F2 = (F + 1) / 2;
    const long P = (long)B * T2 * F2;
    const int ppb = (int)((P + 767) / 768 < 256 ? 256 : (P + 767) / 768);       // <= 768 workgroups = 3 per CU at 148 VGPRs, all resident (10C atomics each)
    dim3 grid((unsigned)((P + ppb - 1) / ppb));
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(conv1_bwd_kernel<bf16>, grid, dim3(256), 0, st, x, (const bf16*)dpre, dw, db, B, T, F, T2, F2, C, ppb),
        hipLaunchKernelGGL(conv1_bwd_kernel<float>, grid, dim3(256), 0, st, x, (const float*)dpre, dw, db, B, T, F, T2, F2, C, ppb));
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_conv1_bwd_bn(int dtype, const float* x, const void* dyn, const void* y, const void* pre, const float* mean, const float* rstd,
                                const float* gamma, const double* sums, float* dw, float* db, float* dgamma, float* dbeta, int B, int T, int F,
                                int C, double count, int training, void* stream) {
    if (B <= 0 || T <= 0) return S2T_OK;
    if (!x || !dyn || !y || !mean || !rstd || !gamma || !sums || !dw || !db || !dgamma || !dbeta || (C != 64 && C != 128 && C != 32) || F < 3) return S2T_EINVAL;
    const int T2 = (T + 1) / 2, F2 = (F + 1) / 2;
    const long P = (long)B * T2 * F2;
    hipStream_t st = (hipStream_t)stream;
    if (P < (1l << 24)) {
        // matrix-core form: 1,024 workgroups of 4 waves; LDS = 4 waves x (2 or 3 tensors) x 16 pixel rows, at least the 4 x 10 C reduction floats
        const long units = (P + 15) / 16;
        const unsigned nwg = (unsigned)(units < 4 * 1024 ? (units + 3) / 4 : 1024);
        const size_t esz = dtype == S2T_BF16 ? 2 : 4;
        size_t lds = 4 * (size_t)(pre ? 3 : 2) * 16 * (C * esz + 16);
        if (lds < (size_t)4 * 10 * C * 4) lds = (size_t)4 * 10 * C * 4;
        hipError_t se = hipSuccess;                                              // 1,024 workgroups x 10 x 128, per (device, stream)
        float* part = (float*)s2t_scratch(S2T_SCRATCH_CONV1_BWD, st, (size_t)1024 * 1280 * sizeof(float), &se);
        if (!part) return S2T_EHIP(se);
#define S2T_C1B(T_, NT_, G_) do { static bool attr = false;                                                                                   \
        if (!attr) { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv1_bwd_bn_mfma_kernel<T_, NT_, G_>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024); attr = true; } \
        hipLaunchKernelGGL((conv1_bwd_bn_mfma_kernel<T_, NT_, G_>), dim3(nwg), dim3(256), lds, st, x, (const T_*)dyn, (const T_*)y, (const T_*)pre, mean, rstd, gamma, sums, part, dgamma, dbeta, B, T, F, T2, F2, count, training); } while (0)
#define S2T_C1B_NT(T_, G_) { if (C == 64) S2T_C1B(T_, 4, G_); else if (C == 128) S2T_C1B(T_, 8, G_); else S2T_C1B(T_, 2, G_); }
        if (pre) { DISPATCH_T(dtype, S2T_C1B_NT(bf16, true), S2T_C1B_NT(float, true)); }
        else { DISPATCH_T(dtype, S2T_C1B_NT(bf16, false), S2T_C1B_NT(float, false)); }
#undef S2T_C1B_NT
#undef S2T_C1B
        hipLaunchKernelGGL(chan_partials_f32_kernel, dim3(10 * C), dim3(256), 0, st, part, (int)nwg, C, dw, db);
        S2T_LAUNCH_CHECK();
        return S2T_OK;
    }
    const int ppb = (int)((P + 511) / 512 < 256 ? 256 : (P + 511) / 512);     // <= 512 workgroups = 2 per CU at ~172 VGPRs, all resident
    dim3 grid((unsigned)((P + ppb - 1) / ppb));
    if (pre) {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((conv1_bwd_bn_kernel<bf16, true>), grid, dim3(256), 0, st, x, (const bf16*)dyn, (const bf16*)y, (const bf16*)pre, mean, rstd, gamma, sums, dw, db, dgamma, dbeta, B, T, F, T2, F2, C, ppb, count, training),
            hipLaunchKernelGGL((conv1_bwd_bn_kernel<float, true>), grid, dim3(256), 0, st, x, (const float*)dyn, (const float*)y, (const float*)pre, mean, rstd, gamma, sums, dw, db, dgamma, dbeta, B, T, F, T2, F2, C, ppb, count, training));
    } else {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((conv1_bwd_bn_kernel<bf16, false>), grid, dim3(256), 0, st, x, (const bf16*)dyn, (const bf16*)y, (const bf16*)nullptr, mean, rstd, gamma, sums, dw, db, dgamma, dbeta, B, T, F, T2, F2, C, ppb, count, training),
            hipLaunchKernelGGL((conv1_bwd_bn_kernel<float, false>), grid, dim3(256), 0, st, x, (const float*)dyn, (const float*)y, (const float*)nullptr, mean, rstd, gamma, sums, dw, db, dgamma, dbeta, B, T, F, T2, F2, C, ppb, count, training));
    }
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_chan_sums(int dtype, const void* y, const void* dyn, const float* mean, const float* rstd,
                             double* sums, long P, int C, int mode, void* stream) {
    if (P <= 0) return S2T_OK;
    if (!y || !sums || (C != 64 && C != 128 && C != 32) || (mode && (!dyn || !mean || !rstd))) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (P >= 256L * 1024) {                                    // big tensors: 256 workgroups of 16 waves
        const int ppb = (int)((P + 255) / 256);
        dim3 grid((unsigned)((P + ppb - 1) / ppb));
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((chan_sums_kernel<bf16, 16>), grid, dim3(1024), 0, st, (const bf16*)y, (const bf16*)dyn, mean, rstd, sums, P, C, mode, ppb),
            hipLaunchKernelGGL((chan_sums_kernel<float, 16>), grid, dim3(1024), 0, st, (const float*)y, (const float*)dyn, mean, rstd, sums, P, C, mode, ppb));
    } else {
        const int ppb = (int)((P + 255) / 256 < 256 ? 256 : (P + 255) / 256);
        dim3 grid((unsigned)((P + ppb - 1) / ppb));
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((chan_sums_kernel<bf16, 4>), grid, dim3(256), 0, st, (const bf16*)y, (const bf16*)dyn, mean, rstd, sums, P, C, mode, ppb),
            hipLaunchKernelGGL((chan_sums_kernel<float, 4>), grid, dim3(256), 0, st, (const float*)y, (const float*)dyn, mean, rstd, sums, P, C, mode, ppb));
    }
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_bn_finalize(const double* sums, const float* gamma, const float* beta, float* run_mean,
                               float* run_var, long long* num_batches, float* mean, float* rstd, float* scale,
                               float* shift, double count, int C, int training, float momentum, float eps, void* stream) {
    if (!gamma || !beta || !run_mean || !run_var || !mean || !rstd || !scale || !shift || (training && !sums)) return S2T_EINVAL;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream, sums, gamma, beta, run_mean,
                       run_var, num_batches, mean, rstd, scale, shift, count, C, training, momentum, eps);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_bn_apply(int dtype, const void* y, const float* scale, const float* shift, void* yn, long n, int C,
                            float p_drop, unsigned long long seed, void* stream) {
    if (n <= 0) return S2T_OK;
    if (!y || !scale || !shift || !yn || (C % 8) || (256 % (C / 8)) || (n % C) || p_drop < 0.f || p_drop >= 1.f) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dtype,
        hipLaunchKernelGGL(bn_apply_kernel<bf16>, dim3(nblocks(n)), dim3(256), 0, st, (const bf16*)y, scale, shift, (bf16*)yn, n, C, p_drop, seed),
        hipLaunchKernelGGL(bn_apply_kernel<float>, dim3(nblocks(n)), dim3(256), 0, st, (const float*)y, scale, shift, (float*)yn, n, C, p_drop, seed));
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_bn_bwd_apply(int dtype, const void* dyn, const void* y, const void* pre, const float* mean, const float* rstd,
                                const float* gamma, const double* sums, void* dpre, float* dgamma, float* dbeta, long n,
                                int C, double count, int training, void* stream) {
    if (n <= 0) return S2T_OK;
    if (!dyn || !y || !mean || !rstd || !gamma || !sums || !dpre || !dgamma || !dbeta || C > 256 || (C % 8) || (256 % (C / 8)) || (n % C)) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (pre) {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((bn_bwd_apply_kernel<bf16, true>), dim3(nblocks(n)), dim3(256), 0, st, (const bf16*)dyn, (const bf16*)y, (const bf16*)pre, mean, rstd, gamma, sums, (bf16*)dpre, dgamma, dbeta, n, C, count, training),
            hipLaunchKernelGGL((bn_bwd_apply_kernel<float, true>), dim3(nblocks(n)), dim3(256), 0, st, (const float*)dyn, (const float*)y, (const float*)pre, mean, rstd, gamma, sums, (float*)dpre, dgamma, dbeta, n, C, count, training));
    } else {
        DISPATCH_T(dtype,
            hipLaunchKernelGGL((bn_bwd_apply_kernel<bf16, false>), dim3(nblocks(n)), dim3(256), 0, st, (const bf16*)dyn, (const bf16*)y, (const bf16*)nullptr, mean, rstd, gamma, sums, (bf16*)dpre, dgamma, dbeta, n, C, count, training),
            hipLaunchKernelGGL((bn_bwd_apply_kernel<float, false>), dim3(nblocks(n)), dim3(256), 0, st, (const float*)dyn, (const float*)y, (const float*)nullptr, mean, rstd, gamma, sums, (float*)dpre, dgamma, dbeta, n, C, count, training));
    }
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_permute_cf(int dst_dtype, const float* src, void* dst, int N, int C, int F, int mode, void* stream) {
    const long n = (long)N * C * F;
    if (n <= 0) return S2T_OK;
    if (!src || !dst || (mode == 1 && dst_dtype != S2T_F32)) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dst_dtype,
        hipLaunchKernelGGL(permute_cf_kernel<bf16>, dim3(nblocks(n)), dim3(256), 0, st, src, (bf16*)dst, N, C, F, mode),
        hipLaunchKernelGGL(permute_cf_kernel<float>, dim3(nblocks(n)), dim3(256), 0, st, src, (float*)dst, N, C, F, mode));
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_permute_conv_w(int dst_dtype, const float* src, void* dst, int Co, int Ci, int mode, void* stream) {
    const long n = (long)Co * Ci * 9;
    if (n <= 0) return S2T_OK;
    if (!src || !dst || (mode == 2 && dst_dtype != S2T_F32) || mode < 0 || mode > 2) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    DISPATCH_T(dst_dtype,
        hipLaunchKernelGGL(permute_conv_w_kernel<bf16>, dim3(nblocks(n)), dim3(256), 0, st, src, (bf16*)dst, Co, Ci, mode),
        hipLaunchKernelGGL(permute_conv_w_kernel<float>, dim3(nblocks(n)), dim3(256), 0, st, src, (float*)dst, Co, Ci, mode));
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

extern "C" int s2t_add_pos(int dtype, const void* src, void* dst, const float* table, const int* len, int T, int B, int D,
                           float p_drop, unsigned long long seed, void* stream) {
    const long n = (long)T * B * D;
    if (n <= 0) return S2T_OK;
    if (!src || !dst || !table || !len || p_drop < 0.f || p_drop >= 1.f) return S2T_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int E = dtype == S2T_BF16 ? 8 : 4;
    const bool vec = D % E == 0 && ((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)table) & 15) == 0);
    const int nb = nblocks(vec ? n / E : n);
#define S2T_ADD_POS(T_, V_) hipLaunchKernelGGL((add_pos_kernel<T_, V_>), dim3(nb), dim3(256), 0, st, (const T_*)src, (T_*)dst, table, len, T, B, D, p_drop, seed)
    if (vec) { DISPATCH_T(dtype, S2T_ADD_POS(bf16, true), S2T_ADD_POS(float, true)); }
    else { DISPATCH_T(dtype, S2T_ADD_POS(bf16, false), S2T_ADD_POS(float, false)); }
#undef S2T_ADD_POS
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}


// ------------------------------------------------------------------ input augmentation
// TimeStretch + SpecAugment of examples/speech_recognition/modules/{time_stretch,specaugment}.py as ONE pass over the batch:
// out[b][t][f] = x[b][row_map[b][t]][f] (row_map -1 / absent rows = 0), zeroed inside the utterance's time masks [t0, t0+w) and
// frequency masks [f0, f0+w).  The tables come from the host, which draws them from the same random streams as the reference
// (augment.py); the reference applies them with per-utterance slice writes from Python.
__global__ __launch_bounds__(256) void augment_kernel(const float* __restrict__ x, float* __restrict__ out, const int* __restrict__ row_map,
                                                      const int* __restrict__ fmask, const int* __restrict__ tmask, int B, int T, int To,
                                                      int F, int nF, int nT) {
    const long row = blockIdx.x;                       // (b, t)
    const int b = (int)(row / To), t = (int)(row % To);
    int src = row_map ? row_map[row] : (t < T ? t : -1);
    for (int i = 0; i < nT; ++i) {
        const int t0 = tmask[(b * nT + i) * 2], w = tmask[(b * nT + i) * 2 + 1];
        if (t >= t0 && t < t0 + w) src = -1;
    }
    for (int f = threadIdx.x; f < F; f += 256) {
        bool keep = src >= 0;
        for (int i = 0; i < nF; ++i) {
            const int f0 = fmask[(b * nF + i) * 2], w = fmask[(b * nF + i) * 2 + 1];
            keep = keep && !(f >= f0 && f < f0 + w);
        }
        out[row * F + f] = keep ? x[((long)b * T + src) * F + f] : 0.f;
    }
}
extern "C" int s2t_augment(const float* x, float* out, const int* row_map, const int* fmask, const int* tmask, int B, int T, int To,
                           int F, int nF, int nT, void* stream) {
    if (B <= 0 || To <= 0 || F <= 0) return (B < 0 || To < 0 || F < 0) ? S2T_EINVAL : S2T_OK;
    if (!x || !out || x == out || T <= 0 || nF < 0 || nT < 0 || (nF > 0 && !fmask) || (nT > 0 && !tmask)) return S2T_EINVAL;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)((long)B * To)), dim3(256), 0, (hipStream_t)stream, x, out, row_map, fmask, tmask, B, T, To, F, nF, nT);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}


// ------------------------------------------------------------------ conv2 weight gradient, all nine taps per workgroup
// dW[co][tap*64 + ci] += sum over output pixels (t4, b, f4) of dpre[t4][b][f4][co] * y1n[b][2 t4 + kh - 1][2 f4 + kw - 1][ci]
// (autograd of nn.Conv2d(64, 64, 3, stride 2, padding 1), conv_transformer.py:348-354).  As nine gathered GEMMs (one per tap) the
// product re-read dpre nine times and y1n nine times through row maps: 0.85 ms per step.  Here a workgroup walks (t4, b) groups:
// it stages the group's 20 output pixels and the 3 x 40 input pixels they touch ONCE (17.5 KB), and all nine taps read their
// operands out of that window with transposed LDS reads whose per-lane ROW address is 2 f4 + kw -- the stride-2 gather costs
// nothing.  Contraction = the f4 axis padded to 32 (one 16x16x32 MFMA step); 9 x 64 x 64 accumulators live in registers
// (144 VGPRs per lane over 4 waves) for the whole walk and leave as f32 atomics once.  bf16, 64 channels.
typedef short c2_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 c2_tr_frag(const char* base, int row_lo, int row_hi, int key_lo, int key_hi, int chunk, int r16) {
    // 16 columns starting at chunk*8 of 8 rows given as two groups of 4 (this lane supplies row (r16>>2) of each), 128-B rows,
    // chunk swizzle by (row key & 7)
    const int ch = chunk + ((r16 & 3) >> 1);
    const char* a0 = base + row_lo * 128 + ((ch ^ (key_lo & 7)) << 4) + ((r16 & 1) << 3);
    const char* a1 = base + row_hi * 128 + ((ch ^ (key_hi & 7)) << 4) + ((r16 & 1) << 3);
    const u32x2 w0 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) c2_s16x4*)a0));
    const u32x2 w1 = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) c2_s16x4*)a1));
    return (u32x4){w0[0], w0[1], w1[0], w1[1]};
}
__global__ __launch_bounds__(256, 2) void conv2_wgrad_kernel(const bf16* __restrict__ dpre, const bf16* __restrict__ y1n, float* __restrict__ gw,
                                                             int B, int T2, int F2, int T4, int F4, int groups_per_wg) {
    constexpr int WROWS = 66, WIN = 3 * WROWS * 128, DYB = 32 * 128;
    __shared__ __attribute__((aligned(16))) char lds[WIN + DYB];
    char* win = lds;
    char* dyt = lds + WIN;
    for (int i = threadIdx.x; i < (WIN + DYB) / 16; i += 256) reinterpret_cast<u32x4*>(lds)[i] = (u32x4){0, 0, 0, 0};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, q = lane >> 4;
    const int wco = wave >> 1, wci = wave & 1;
    const int ngroups = T4 * B;
    const int g0 = blockIdx.x * groups_per_wg, g1 = min(ngroups, g0 + groups_per_wg);
    f32x4 acc[9][2][2];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[t][i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nchunk = 3 * F2 * 8 + F4 * 8;                   // 16-byte pieces of one group's window + dY rows
    u32x4 regs[5];
    auto gload = [&](int g) {
        const int t4 = g / B, b = g - t4 * B;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = threadIdx.x + 256 * i;
            u32x4 v = {0, 0, 0, 0};
            if (c < 3 * F2 * 8) {
                const int kh = c / (F2 * 8), rem = c - kh * (F2 * 8), px = rem >> 3, ch = rem & 7;
                const int t2 = 2 * t4 + kh - 1;
                if (t2 >= 0 && t2 < T2) v = *reinterpret_cast<const u32x4*>(y1n + (((long)b * T2 + t2) * F2 + px) * 64 + ch * 8);
            } else if (c < nchunk) {
                const int cc = c - 3 * F2 * 8, px = cc >> 3, ch = cc & 7;
                v = *reinterpret_cast<const u32x4*>(dpre + ((long)g * F4 + px) * 64 + ch * 8);
            }
            regs[i] = v;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int c = threadIdx.x + 256 * i;
            if (c < 3 * F2 * 8) {
                const int kh = c / (F2 * 8), rem = c - kh * (F2 * 8), r = (rem >> 3) + 1, ch = rem & 7;     // window row = f2 + 1
                *reinterpret_cast<u32x4*>(win + (kh * WROWS + r) * 128 + ((ch ^ (r & 7)) << 4)) = regs[i];
            } else if (c < nchunk) {
                const int cc = c - 3 * F2 * 8, px = cc >> 3, ch = cc & 7;
                *reinterpret_cast<u32x4*>(dyt + px * 128 + ((ch ^ (px & 7)) << 4)) = regs[i];
            }
        }
    };
    if (g0 < g1) gload(g0);
    __syncthreads();                                             // zero fill done
    for (int g = g0; g < g1; ++g) {
        lstore();
        __syncthreads();
        if (g + 1 < g1) gload(g + 1);
        // A = dY^T (rows = co), contraction over the group's f4 positions 8q .. 8q+7 of this lane's k-slice
        const int p_lo = 8 * q + (r16 >> 2), p_hi = p_lo + 4;
        u32x4 fa[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) fa[i] = c2_tr_frag(dyt, p_lo, p_hi, p_lo, p_hi, 2 * (2 * wco + i), r16);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int r_lo = 2 * p_lo + kw, r_hi = 2 * p_hi + kw;          // window row of position p under tap column kw
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const u32x4 fb = c2_tr_frag(win, kh * WROWS + r_lo, kh * WROWS + r_hi, r_lo, r_hi, 2 * (2 * wci + j), r16);
#pragma unroll
                    for (int i = 0; i < 2; ++i) acc[kh * 3 + kw][i][j] = mma16<bf16>(fa[i], fb, acc[kh * 3 + kw][i][j]);
                }
            }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = 16 * (2 * wco + i) + 4 * q + r, ci = 16 * (2 * wci + j) + r16;
                    atomicAdd(gw + (long)co * 576 + t * 64 + ci, acc[t][i][j][r]);
                }
}
extern "C" int s2t_conv2_wgrad(int dtype, const void* dpre, const void* y1n, float* gw, int B, int T2, int F2, int C, void* stream) {
    if (B <= 0 || T2 <= 0) return S2T_OK;
    if (!dpre || !y1n || !gw) return S2T_EINVAL;
    const int T4 = (T2 + 1) / 2, F4 = (F2 + 1) / 2;
    if (dtype != S2T_BF16 || C != 64 || F4 > 32 || F2 > 64 || 3 * F2 * 8 + F4 * 8 > 1280) return S2T_ENOTSUP;   // callers fall back to the gathered GEMMs
    if (((uintptr_t)dpre | (uintptr_t)y1n) & 15) return S2T_ENOTSUP;         // 16-byte staging loads (as s2t_conv2_fwd / s2t_conv2_dgrad)
    const int ngroups = T4 * B;
    int gpw = (ngroups + 511) / 512;                            // 2 workgroups per CU
    gpw = gpw < 8 ? 8 : gpw;
    hipLaunchKernelGGL(conv2_wgrad_kernel, dim3((ngroups + gpw - 1) / gpw), dim3(256), 0, (hipStream_t)stream, (const bf16*)dpre, (const bf16*)y1n,
                       gw, B, T2, F2, T4, F4, gpw);
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
