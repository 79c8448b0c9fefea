// CTC segmentation of long recordings (include/s2t_hip.h: s2t_ctc_segment): the forced alignment of ctc_align.hip with free ends, for
// transcripts of up to 16,383 tokens given as a list of utterances, and per utterance its frames and how well it fits.  Three launches:
//   * a row phase, one wave per (t, b) row: the row's maximum and the log of its sum of exp, 8 bytes per row.  No emission table:
//     at 22,500 frames and 15,000 tokens it would hold more than 1 GB;
//   * a recording phase, one workgroup of up to 1,024 threads per recording.  Every thread owns K = 2, 4, 8, 16 or 32 consecutive
//     states in registers and GATHERS the logits of its own K / 2 tokens from the frame's row (every thread of the workgroup reads
//     that row in the same frame: it comes from L2), some frames ahead; the two values below a run come from the thread below through
//     LDS behind one LDS-only barrier per frame.  The frame step and its back-pointers (2 bits per state, one dword per 16 states)
//     are ctc_lattice.hpp's, the code ctc_align.hip runs.  The backward walk moves at most two states per frame, so of a block of
//     64 frames it stages only the 9 dwords per frame the path can touch; `states`, `frames`, `tok_score`, `score` and the
//     per-frame emission of the path (frame_lp, workspace) come from the walked blocks through ctc_lattice.hpp's emit block, the
//     aligner's too: with both ends pinned the two give the same bits (the skip / live masks are each file's own: a test pairs
//     every form of the two kernels);
//   * an utterance phase, one 256-thread workgroup per (utterance, recording): the span from `frames`, its sum, mean and the lowest
//     mean of `window` consecutive frames, from frame_lp.
// No atomics, no memset, no host read; a workgroup never waits for another one.
#include "common.hpp"
#include "ctc_lattice.hpp"
#include "prof.hpp"
#include "s2t_hip.h"

namespace {

constexpr int SEG_BLOCK = 64;                                       // frames per block of the backward walk (ctc_align.hip's ALN_BLOCK)
constexpr int SEG_WIN = 9;                                          // dwords of back-pointers per frame a block's walk can touch: the
                                                                    // states s - 128 .. s of its last frame's state s
constexpr int SEG_FREE_START = S2T_CTC_SEGMENT_FREE_START, SEG_FREE_END = S2T_CTC_SEGMENT_FREE_END;

// ------------------------------------------------------------------ row phase
// rs [T*B][2]: the row's maximum m and log1p of the sum of exp(x - m) over the other columns, the two numbers ctc_align.hip's row
// phase subtracts one after the other.  Rows t >= in_len[b] and recordings whose counts are out of range are skipped.
template <typename T>
__global__ __launch_bounds__(256) void ctc_segment_row_kernel(const T* __restrict__ logits, const int* __restrict__ in_len,
                                                              const long long* __restrict__ tgt_len, const long long* __restrict__ n_utt,
                                                              float2* __restrict__ rs, int Tn, int B, int V, int ld, int Lmax, int Umax) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)Tn * B) return;                               // whole waves leave: nothing below synchronises the workgroup
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    if (t >= in_len[b]) return;
    const long long Lq = tgt_len[b], Uq = n_utt[b];
    if (Lq < 1 || Lq > Lmax || Uq < 1 || Uq > Umax) return;
    const T* x = logits + row * ld;
    const RowStat st = row_max_lse<T, true>(x, V, lane);
    if (lane == 0) rs[row] = make_float2(st.m, st.lse1);
}

// ------------------------------------------------------------------ recording phase
// A logit of a row by buffer addressing: the row's descriptor is wave-uniform, a column is one 32-bit register of byte offset (a flat
// load would keep a 64-bit address per token in registers, 32 of them at K = 32); a column past the row would load 0, none is.
template <typename T> __device__ __forceinline__ float row_logit(__amdgpu_buffer_rsrc_t r, uint32_t off);
template <> __device__ __forceinline__ float row_logit<float>(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0));
}
template <> __device__ __forceinline__ float row_logit<bf16>(__amdgpu_buffer_rsrc_t r, uint32_t off) {
    return __builtin_bit_cast(float, (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(r, off, 0, 0) << 16);
}

// The emission of lane i's state `mine` (-1 behind cnt) at frame t0 + i of a walked block of cnt frames, gathered from the logits row
// where ctc_align.hip reads its table (a free outer blank: 0) and kept in flp for the utterance phase: lattice_emit_block's lp.
template <typename T>
__device__ __forceinline__ float seg_path_lp(const T* __restrict__ logits, const float2* __restrict__ rs, const long long* __restrict__ y,
                                             int blank, int flags, int S, int ld, int t0, int cnt, int lane, int b, int B, int mine,
                                             float* __restrict__ flp) {
    if (lane >= cnt) return 0.f;
    const int t = t0 + lane;
    float lp = 0.f;
    const bool free = (mine == 0 && (flags & SEG_FREE_START)) || (mine == S - 1 && (flags & SEG_FREE_END));
    if (!free) {
        const long row = (long)t * B + b;
        const long long c = (mine & 1) ? y[mine >> 1] : (long long)blank;
        const float2 r = rs[row];
        lp = (to_f32(logits[row * ld + c]) - r.x) - r.y;
    }
    flp[t] = lp;
    return lp;
}

// Thread tid owns the states tid K .. tid K + K - 1.  bp [B][T][W] dwords, dword d of a frame holding the states 16 d .. 16 d + 15.
template <typename T, int K>
__global__ __launch_bounds__(1024) void ctc_segment_rec_kernel(const T* __restrict__ logits, const float2* __restrict__ rs,
                                                               const int* __restrict__ in_len, const long long* __restrict__ targets,
                                                               const long long* __restrict__ tgt_len, const long long* __restrict__ utt_end,
                                                               const long long* __restrict__ n_utt, uint32_t* bp, float* __restrict__ frame_lp,
                                                               int* __restrict__ states, int* __restrict__ frames, float* __restrict__ tok_score,
                                                               float* __restrict__ score, int* __restrict__ status, int Tn, int B, int V, int ld,
                                                               int Lmax, int Umax, int W, int blank, int flags) {
    constexpr int KT = K / 2;                                       // tokens of a thread's run
    constexpr int NW = (K + 15) / 16;                               // back-pointer dwords a thread fills (K < 16: a share of one)
    constexpr int D = K <= 4 ? 8 : (K <= 8 ? 4 : (K <= 16 ? 2 : 1));  // frames the logits are requested ahead: D * KT <= 16 registers
    __shared__ float2 s_hand[2][1024];                              // the two top values of every run, for the run above; two frames
    __shared__ uint32_t s_bp[SEG_BLOCK * SEG_WIN];
    __shared__ float s_end[2];
    __shared__ int s_flag, s_state;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int n = min(max(in_len[b], 0), Tn);
    const long long Lq = tgt_len[b], Uq = n_utt[b];
    if (Lq < 1 || Lq > Lmax || Uq < 1 || Uq > Umax) { if (tid == 0) status[b] = 2; return; }
    const int L = (int)Lq, U = (int)Uq, S = 2 * L + 1;
    const long long* y = targets + (long)b * Lmax;
    const long long* ue = utt_end + (long)b * Umax;
    if (tid == 0) s_flag = 0;
    __syncthreads();
    bool bad = false;
    for (int u = tid; u < U; u += nt) {
        const long long e = ue[u];
        bad = bad || e <= (u ? ue[u - 1] : 0) || (u == U - 1 && e != Lq);
    }
    if (bad) s_flag = 1;
    __syncthreads();
    bad = s_flag != 0;                                              // offsets first: only then do the L tokens lie inside the row
    if (!bad) {
        for (int i = tid; i < L; i += nt) { const long long c = y[i]; bad = bad || c < 0 || c >= V || c == blank; }
        if (bad) s_flag = 1;
    }
    __syncthreads();
    if (s_flag != 0) { if (tid == 0) status[b] = 2; return; }
    int* st = states + (long)b * Tn; int* fr = frames + (long)b * Lmax * 2; float* ts = tok_score + (long)b * Lmax;
    float* flp = frame_lp + (long)b * Tn;
    if (n == 0) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, tid, nt); return; }

    const int s0 = tid * K;
    uint32_t skip = 0, live = 0, zero = 0;
    uint32_t col[KT];                                               // byte offsets of the run's tokens in a row (a dead token: 0);
                                                                    // 32 bits each: a uniform row address plus one register
#pragma unroll
    for (int j = 0; j < K; ++j) {                                   // ctc_align.hip's align_run_bits and the free outer blanks in one
        const int s = s0 + j;                                       // loop: apart they make the frame loop slower (ctc_lattice.hpp)
        if (s < S) live |= 1u << j;
        if ((s & 1) && s >= 3 && s < S && y[(s - 1) >> 1] != y[(s - 3) >> 1]) skip |= 1u << j;
        if ((s == 0 && (flags & SEG_FREE_START)) || (s == S - 1 && (flags & SEG_FREE_END))) zero |= 1u << j;
    }
#pragma unroll
    for (int q = 0; q < KT; ++q) col[q] = s0 / 2 + q < L ? (uint32_t)y[s0 / 2 + q] * (uint32_t)sizeof(T) : 0u;
    const bool works = (tid & ~63) * K < S;                         // whole waves above the recording's states only keep the barriers

    float xb[D], xt[D][KT], xm[D], xl[D];                           // frame tg + d waits in slot d: raw logits and the row's m, lse1
    auto fetch = [&](int d, int t) {
        const long row = (long)min(t, n - 1) * B + b;               // behind the last frame: that frame again
        // vector loads although the row's (m, lse1) and its blank logit have one address for the whole workgroup: scalar loads
        // would be waited for at every frame's lgkmcnt(0), these stay in flight
        const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(logits + row * ld), 0, V * (int)sizeof(T), 0x00020000);
        const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2*>(rs + row), 0, 8, 0x00020000);
        xm[d] = row_logit<float>(rr, 0);
        xl[d] = row_logit<float>(rr, 4);
        xb[d] = row_logit<T>(rx, (uint32_t)blank * (uint32_t)sizeof(T));
#pragma unroll
        for (int q = 0; q < KT; ++q) xt[d][q] = row_logit<T>(rx, col[q]);
    };
    float v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = -INFINITY;
    const int group = tid & (16 / (K < 16 ? K : 16) - 1);           // K < 16: the thread's place among those that share a dword
    if (!works) {
        for (int t = 0; t < n; ++t) lds_barrier();                  // a loop of its own: inside the other one the requested logits
    } else {                                                        // would have to be copied, and so waited for, at every frame's end
#pragma unroll
        for (int d = 0; d < D; ++d) fetch(d, d);
        for (int tg = 0; tg < n; tg += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int t = tg + d;
                if (t >= n) break;
                const float eb = (xb[d] - xm[d]) - xl[d];
                float et[KT];
#pragma unroll
                for (int q = 0; q < KT; ++q) et[q] = (xt[d][q] - xm[d]) - xl[d];
                fetch(d, t + D);
                if (t == 0) {
#pragma unroll
                    for (int j = 0; j < K; ++j) {
                        float e = (j & 1) ? et[j >> 1] : eb;
                        if ((zero >> j) & 1) e = 0.f;
                        v[j] = (s0 + j <= 1 && s0 + j < S) ? e : -INFINITY;
                    }
                } else {
                    float p1 = -INFINITY, p2 = -INFINITY;
                    if (tid > 0) { const float2 h = s_hand[(t - 1) & 1][tid - 1]; p1 = h.x; p2 = h.y; }
                    uint32_t bits[NW];
                    lattice_step<K>(v, p1, p2, et, eb, skip, live, zero, bits);
                    uint32_t* row = bp + ((long)b * Tn + t) * W;
                    if constexpr (K >= 16) {
#pragma unroll
                        for (int w = 0; w < NW; ++w) if (tid * NW + w < W) row[tid * NW + w] = bits[w];
                    } else {
                        uint32_t word = bits[0] << (2 * K * group);
#pragma unroll
                        for (int o = 1; o < 16 / K; o <<= 1) word |= __shfl_xor(word, o);
                        if (group == 0 && s0 / 16 < W) row[s0 / 16] = word;
                    }
                }
                s_hand[t & 1][tid] = make_float2(v[K - 1], v[K - 2]);
                lds_barrier();                                      // LDS only: the requested logits and the back-pointer stores
            }                                                       // stay in flight across it
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (s0 + j == S - 1) s_end[0] = v[j];
        if (s0 + j == S - 2) s_end[1] = v[j];
    }
    __threadfence();                                                // the back-pointers were written by other threads of this workgroup
    __syncthreads();
    const float e1 = s_end[0], e2 = s_end[1];
    int s = e2 > e1 ? S - 2 : S - 1;
    if (!(fmaxf(e1, e2) > -INFINITY)) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, tid, nt); return; }
    int s_after = -1;
    float carry = 0.f, total = 0.f;
    for (int t0 = (n - 1) / SEG_BLOCK * SEG_BLOCK; t0 >= 0; t0 -= SEG_BLOCK) {
        const int cnt = min(SEG_BLOCK, n - t0);
        const int lo = max(s - 128, 0) >> 4;                        // the walk leaves at most 2 (cnt - 1) <= 126 states below s
        for (int i = tid; i < cnt * SEG_WIN; i += nt) {             // frame 0 holds no back-pointers: staged, never looked at
            const int f = i / SEG_WIN, d = lo + i - f * SEG_WIN;
            s_bp[i] = d < W ? bp[((long)b * Tn + t0 + f) * W + d] : 0u;
        }
        __syncthreads();
        if (tid < 64) {
            int mine = -1;
            for (int i = cnt - 1; i >= 0; --i) {
                if (tid == i) mine = s;
                if (i > 0 || t0 > 0) s -= (s_bp[i * SEG_WIN + (s >> 4) - lo] >> (2 * (s & 15))) & 3;
            }
            const float lp = seg_path_lp<T>(logits, rs, y, blank, flags, S, ld, t0, cnt, tid, b, B, mine, flp);
            lattice_emit_block(lp, t0, cnt, tid, mine, s, s_after, carry, total, st, fr, ts);
            if (tid == 0) s_state = s;
        }
        __syncthreads();
        s = s_state;
    }
    for (int t = n + tid; t < Tn; t += nt) st[t] = -1;
    if (tid < 64) {
        total = wave_sum(total);
        if (tid == 0) { score[b] = total; status[b] = 0; }
    }
}

// ------------------------------------------------------------------ utterance phase
// One workgroup per (utterance u, recording b): the span [first frame of the first token, one past the last frame of the last token),
// the sum of frame_lp over it, its mean, and the lowest mean over `window` consecutive frames inside it (every window summed on its
// own, in frame order: no running sum that drifts).  The sums are taken in one order whatever the batch.
__global__ __launch_bounds__(256) void ctc_segment_utt_kernel(const float* __restrict__ frame_lp, const long long* __restrict__ utt_end,
                                                              const long long* __restrict__ n_utt, const int* __restrict__ frames,
                                                              const int* __restrict__ status, int* __restrict__ utt_frames,
                                                              float* __restrict__ utt_score, float* __restrict__ conf_mean,
                                                              float* __restrict__ conf_min, int Tn, int Lmax, int Umax, int window) {
    __shared__ float sh[16];
    const int b = blockIdx.x, u = blockIdx.y, tid = threadIdx.x;
    const int code = status[b];
    if (code == 2 || u >= n_utt[b]) return;                         // a refused recording: its counts may be anything
    const long o = (long)b * Umax + u;
    if (code == 1) {
        if (tid == 0) { utt_frames[2 * o] = utt_frames[2 * o + 1] = -1; utt_score[o] = conf_mean[o] = conf_min[o] = -INFINITY; }
        return;
    }
    const long long i0 = u ? utt_end[o - 1] : 0, i1 = utt_end[o] - 1;
    const int f0 = frames[((long)b * Lmax + i0) * 2], f1 = frames[((long)b * Lmax + i1) * 2 + 1];
    const float* flp = frame_lp + (long)b * Tn;
    float part = 0.f;
    for (int t = f0 + tid; t < f1; t += 256) part += flp[t];
    const float sum = block_sum(part, sh);
    const float mean = sum / (float)(f1 - f0);
    float low = INFINITY;
    for (int t = f0 + tid; t + window <= f1; t += 256) {
        float w = 0.f;
        for (int i = 0; i < window; ++i) w += flp[t + i];
        low = fminf(low, w / (float)window);
    }
    low = -block_max(-low, sh);
    if (tid == 0) {
        utt_frames[2 * o] = f0; utt_frames[2 * o + 1] = f1;
        utt_score[o] = sum; conf_mean[o] = mean; conf_min[o] = f1 - f0 < window ? mean : low;
    }
}

inline int seg_bp_words(int Lmax) { return (2 * Lmax + 1 + 15) / 16; }

template <typename T, int K>
void seg_launch_rec(hipStream_t st, int threads, const T* logits, const float2* rs, const int* in_len, const long long* targets,
                    const long long* tgt_len, const long long* utt_end, const long long* n_utt, uint32_t* bp, float* frame_lp, int* states,
                    int* frames, float* tok_score, float* score, int* status, int T_, int B, int V, int ld, int Lmax, int Umax, int W, int blank,
                    int flags) {
    hipLaunchKernelGGL((ctc_segment_rec_kernel<T, K>), dim3(B), dim3(threads), 0, st, logits, rs, in_len, targets, tgt_len, utt_end, n_utt, bp,
                       frame_lp, states, frames, tok_score, score, status, T_, B, V, ld, Lmax, Umax, W, blank, flags);
}

template <typename T>
int seg_run(hipStream_t st, const void* logits_, const int* in_len, const long long* targets, const long long* tgt_len,
            const long long* utt_end, const long long* n_utt, void* ws, int* states, int* frames, float* tok_score, float* score,
            int* utt_frames, float* utt_score, float* conf_mean, float* conf_min, int* status, int T_, int B, int V, int ld, int Lmax,
            int Umax, int blank, int flags, int window) {
    const T* logits = (const T*)logits_;
    const int W = seg_bp_words(Lmax);
    float2* rs = (float2*)ws;                                        // [T*B] (m, lse1)
    float* frame_lp = (float*)(rs + (size_t)T_ * B);                // [B][T]
    uint32_t* bp = (uint32_t*)(frame_lp + (size_t)T_ * B);          // [B][T][W]
    {
        ProfScope prof("ctc_segment_rows", st, 0, (double)T_ * B * V * sizeof(T));
        hipLaunchKernelGGL(ctc_segment_row_kernel<T>, dim3((unsigned)(((long)T_ * B + 3) / 4)), dim3(256), 0, st, logits, in_len, tgt_len, n_utt,
                           rs, T_, B, V, ld, Lmax, Umax);
    }
    S2T_LAUNCH_CHECK();
    const int S = 2 * Lmax + 1;
    const int K = S <= 2048 ? 2 : S <= 4096 ? 4 : S <= 8192 ? 8 : S <= 16384 ? 16 : 32;
    const int threads = ((S + K - 1) / K + 63) / 64 * 64;
#define SEG_ARGS st, threads, logits, rs, in_len, targets, tgt_len, utt_end, n_utt, bp, frame_lp, states, frames, tok_score, score, status, T_, B, \
                 V, ld, Lmax, Umax, W, blank, flags
    {
        ProfScope prof("ctc_segment_recording", st, 0, 0);
        if (K == 2) seg_launch_rec<T, 2>(SEG_ARGS);
        else if (K == 4) seg_launch_rec<T, 4>(SEG_ARGS);
        else if (K == 8) seg_launch_rec<T, 8>(SEG_ARGS);
        else if (K == 16) seg_launch_rec<T, 16>(SEG_ARGS);
        else seg_launch_rec<T, 32>(SEG_ARGS);
    }
#undef SEG_ARGS
    S2T_LAUNCH_CHECK();
    {
        ProfScope prof("ctc_segment_utterances", st, 0, 0);
        hipLaunchKernelGGL(ctc_segment_utt_kernel, dim3(B, Umax), dim3(256), 0, st, frame_lp, utt_end, n_utt, frames, status, utt_frames,
                           utt_score, conf_mean, conf_min, T_, Lmax, Umax, window);
    }
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}

}  // namespace

extern "C" size_t s2t_ctc_segment_workspace(int T, int B, int Lmax, int Umax) {
    if (T <= 0 || B <= 0 || Lmax < 1 || Lmax > S2T_CTC_SEGMENT_MAX_TARGET || Umax < 1 || Umax > S2T_CTC_SEGMENT_MAX_UTT) return 0;
    const size_t bytes = (size_t)4 * (size_t)T * (size_t)B * (3 + (size_t)seg_bp_words(Lmax));
    return (bytes + 255) / 256 * 256;
}

extern "C" int s2t_ctc_segment(int dtype, const void* logits, const int* in_len, const long long* targets, const long long* tgt_len,
                               const long long* utt_end, const long long* n_utt, void* ws, int* states, int* frames, float* tok_score,
                               float* score, int* utt_frames, float* utt_score, float* utt_conf_mean, float* utt_conf_min, int* status, int T,
                               int B, int V, int ld, int Lmax, int Umax, int blank, int flags, int window, void* stream) {
    if ((long)T * B <= 0 || T <= 0) return S2T_OK;
    if (!logits || !in_len || !targets || !tgt_len || !utt_end || !n_utt || !ws || !states || !frames || !tok_score || !score || !utt_frames ||
        !utt_score || !utt_conf_mean || !utt_conf_min || !status)
        return S2T_EINVAL;
    if (V < 2 || ld < V || blank < 0 || blank >= V || Lmax < 1 || Umax < 1 || (long)T * B > 0x7fffffffL || flags < 0 || flags > 3) return S2T_EINVAL;
    if ((dtype != S2T_F32 && dtype != S2T_BF16) || Lmax > S2T_CTC_SEGMENT_MAX_TARGET || Umax > S2T_CTC_SEGMENT_MAX_UTT || window < 1 ||
        window > S2T_CTC_SEGMENT_MAX_WINDOW)
        return S2T_ENOTSUP;
    hipStream_t st = (hipStream_t)stream;
#define SEG_RUN_ARGS st, logits, in_len, targets, tgt_len, utt_end, n_utt, ws, states, frames, tok_score, score, utt_frames, utt_score, utt_conf_mean, \
                     utt_conf_min, status, T, B, V, ld, Lmax, Umax, blank, flags, window
    return dtype == S2T_BF16 ? seg_run<bf16>(SEG_RUN_ARGS) : seg_run<float>(SEG_RUN_ARGS);
#undef SEG_RUN_ARGS
}
