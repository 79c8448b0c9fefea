// CTC forced alignment (include/s2t_hip.h: s2t_ctc_align): the most likely CTC path among those that collapse to a GIVEN
// transcript, with the frames and the score of every token.  The split of ctc_decode.hip:
//   * a row phase, one wave per (t, b) row with 16-byte loads: the row's maximum and its first index, the sum of exp over the other
//     columns from the L2-resident row (ctc_rows.hpp: row_max_lse), then the L + 1 emissions the sentence needs -- lp[blank],
//     lp[y_0 .. y_{L-1}] -- gathered from the row that has just been streamed.  No [rows][V] tensor exists;
//   * a sentence phase that walks the frames keeping only the previous frame's values, writes a 2-bit back-pointer per
//     (frame, state) to the workspace, then walks them backwards through LDS, a block of frames at a time, and derives `states`,
//     `frames`, `tok_score` and `score` from the path in the same launch.
// The sentence phase has two forms.  A (2 Lmax + 1 <= 1024): one wave per sentence, every lane owns K = 1, 2, 4, 8 or 16
// consecutive states in registers, the two values below a lane's run come by two shuffles per frame, no barrier in the loop.
// B (Lmax <= S2T_CTC_ALIGN_MAX_TARGET): one 256-thread workgroup per sentence, two LDS rows of values, one barrier per frame,
// every thread owns runs of 16 states.  In both a run's back-pointers of a frame are one dword.  No atomics, no host read.
// The frame step of the recursion and the sums over the walked path are ctc_lattice.hpp's: ctc_segment.hip runs the same code.
#include "common.hpp"
#include "ctc_lattice.hpp"
#include "prof.hpp"
#include "s2t_hip.h"

namespace {

constexpr int ALN_BLOCK = 64;                                       // frames per block of the backward walk (form A: 16 KiB of LDS)

// ------------------------------------------------------------------ row phase
// em [T*B][Lmax + 1]: column 0 the blank's log-probability, column 1 + i that of token i (-inf for a token outside [0, V): the
// sentence phase refuses the sentence).  Rows t >= in_len[b] and sentences whose tgt_len is out of range are skipped.
template <typename T>
__global__ __launch_bounds__(256) void ctc_align_row_kernel(const T* __restrict__ logits, const int* __restrict__ in_len,
                                                            const long long* __restrict__ targets, const long long* __restrict__ tgt_len,
                                                            float* __restrict__ em, int Tn, int B, int V, int ld, int Lmax, int blank) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)Tn * B) return;                               // whole waves leave: nothing below synchronises the workgroup
    const int t = (int)(row / B), b = (int)(row - (long)t * B);
    if (t >= in_len[b]) return;
    const long long Lq = tgt_len[b];
    if (Lq < 0 || Lq > Lmax) return;
    const int L = (int)Lq;
    const T* x = logits + row * ld;
    const RowStat st = row_max_lse<T, true>(x, V, lane);
    float* e = em + row * (Lmax + 1);
    const long long* y = targets + (long)b * Lmax;
    for (int i = lane; i <= L; i += 64) {
        const long long c = i == 0 ? (long long)blank : y[i - 1];
        e[i] = (c >= 0 && c < V) ? (to_f32(x[c]) - st.m) - st.lse1 : -INFINITY;
    }
}

// ------------------------------------------------------------------ sentence phase: what the two forms share
// The frame step, the outputs without a path and the emit block are ctc_lattice.hpp's, shared with ctc_segment.hip.

// skip / live bits of the run of K states from s0 (S = 2 L + 1 states exist), as lattice_step takes them
template <int K>
__device__ __forceinline__ void align_run_bits(const long long* __restrict__ y, int s0, int S, uint32_t& skip, uint32_t& live) {
    skip = live = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int s = s0 + j;
        if (s < S) live |= 1u << j;
        if ((s & 1) && s >= 3 && s < S && y[(s - 1) >> 1] != y[(s - 3) >> 1]) skip |= 1u << j;
    }
}

// The backward walk over cnt consecutive frames by ONE wave, from their back-pointers staged in LDS (sbp: W dwords per frame, dword
// s / K holds state s; `first` = the stretch begins at frame 0, which has no back-pointers).  In: s = the state of the stretch's last
// frame.  Lane off + i keeps the state of the stretch's frame i in `mine`.  Out: s = the state of the frame before the stretch.
template <int K>
__device__ __forceinline__ void align_walk(const uint32_t* sbp, int W, int cnt, bool first, int lane, int off, int& s, int& mine) {
    for (int i = cnt - 1; i >= 0; --i) {
        if (lane == off + i) mine = s;
        if (i > 0 || !first) s -= (sbp[i * W + s / K] >> (2 * (s % K))) & 3;
    }
}

// The emission of lane i's state `mine` at frame t0 + i of a walked block of cnt frames, from the table: lattice_emit_block's lp
__device__ __forceinline__ float align_path_lp(const float* __restrict__ em, int t0, int cnt, int lane, int b, int B, int Lmax, int mine) {
    return lane < cnt ? em[((long)(t0 + lane) * B + b) * (Lmax + 1) + ((mine & 1) ? 1 + (mine >> 1) : 0)] : 0.f;
}

// ------------------------------------------------------------------ form A: one sentence, one wave, K states per lane
template <int K>
__global__ __launch_bounds__(64) void ctc_align_wave_kernel(const float* __restrict__ em, const int* __restrict__ in_len,
                                                            const long long* __restrict__ targets, const long long* __restrict__ tgt_len,
                                                            uint32_t* bp, int* __restrict__ states, int* __restrict__ frames,
                                                            float* __restrict__ tok_score, float* __restrict__ score,
                                                            int* __restrict__ status, int Tn, int B, int V, int Lmax, int blank) {
    constexpr int KT = K == 1 ? 1 : K / 2;                          // tokens of a lane's run
    __shared__ uint32_t s_bp[ALN_BLOCK * 64];
    __shared__ float s_v[64 * K];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int n = min(max(in_len[b], 0), Tn);
    int* st = states + (long)b * Tn; int* fr = frames + (long)b * Lmax * 2; float* ts = tok_score + (long)b * Lmax;
    const long long* y = targets + (long)b * Lmax;
    const long long Lq = tgt_len[b];
    if (Lq < 0 || Lq > Lmax) { lattice_fail(2, 0, st, fr, ts, score + b, status + b, Tn, lane, 64); return; }
    const int L = (int)Lq, S = 2 * L + 1;
    bool bad = false;
    for (int i = lane; i < L; i += 64) { const long long c = y[i]; bad = bad || c < 0 || c >= V || c == blank; }
    if (__ballot(bad)) { lattice_fail(2, L, st, fr, ts, score + b, status + b, Tn, lane, 64); return; }
    if (n == 0) {
        if (L > 0) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, lane, 64); return; }
        for (int t = lane; t < Tn; t += 64) st[t] = -1;
        if (lane == 0) { score[b] = 0.f; status[b] = 0; }
        return;
    }
    const int s0 = lane * K;
    const bool odd0 = K == 1 && (lane & 1);
    const int tok0 = K == 1 ? lane >> 1 : s0 >> 1;
    uint32_t skip, live;
    align_run_bits<K>(y, s0, S, skip, live);
    // The emissions come from L2 or HBM (the row phase ran on every XCD): a frame's few dependent instructions hide nothing of that
    // latency, so they are requested a GROUP of D frames ahead -- the loads of frames tg + D .. tg + 2D - 1 fly while tg .. tg + D - 1
    // are computed from registers.
    constexpr int D = K <= 4 ? 16 : 8;
    float nb[D], nt[D][KT];
    auto fetch = [&](int tg) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float* e = em + ((long)min(tg + d, n - 1) * B + b) * (Lmax + 1);      // behind the last frame: that frame again
            nb[d] = e[0];
#pragma unroll
            for (int q = 0; q < KT; ++q) nt[d][q] = (tok0 + q < L && (K > 1 || odd0)) ? e[1 + tok0 + q] : -INFINITY;
        }
    };
    fetch(0);
    float v[K];
    for (int tg = 0; tg < n; tg += D) {
        float cb[D], ct[D][KT];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            cb[d] = nb[d];
#pragma unroll
            for (int q = 0; q < KT; ++q) ct[d][q] = nt[d][q];
        }
        if (tg + D < n) fetch(tg + D);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tg + d;
            if (t >= n) break;
            const float eb = cb[d];
            const float (&et)[KT] = ct[d];
            if (t == 0) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    const float e = K == 1 ? (odd0 ? et[0] : eb) : ((j & 1) ? et[j >> 1] : eb);
                    v[j] = (s0 + j <= 1 && s0 + j < S) ? e : -INFINITY;
                }
                continue;
            }
            float p1 = __shfl_up(v[K - 1], 1);
            float p2 = K >= 2 ? __shfl_up(v[K >= 2 ? K - 2 : 0], 1) : __shfl_up(v[0], 2);
            if (lane == 0) p1 = p2 = -INFINITY;
            if (K == 1 && lane == 1) p2 = -INFINITY;
            uint32_t bits[1];
            lattice_step<K>(v, p1, p2, et, eb, skip, live, 0u, bits, odd0);
            bp[((long)b * Tn + t) * 64 + lane] = bits[0];
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) s_v[s0 + j] = v[j];
    __threadfence();                                                // the back-pointers were written by other lanes of this wave:
                                                                    // complete the stores, drop what L1 may hold, then plain loads
    __syncthreads();
    const float e1 = s_v[S - 1], e2 = S >= 2 ? s_v[S - 2] : -INFINITY;
    int s = e2 > e1 ? S - 2 : S - 1;
    if (!(fmaxf(e1, e2) > -INFINITY)) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, lane, 64); return; }
    int s_after = -1;
    float carry = 0.f, total = 0.f;
    for (int t0 = (n - 1) / ALN_BLOCK * ALN_BLOCK; t0 >= 0; t0 -= ALN_BLOCK) {
        const int cnt = min(ALN_BLOCK, n - t0);
        const uint32_t* src = bp + ((long)b * Tn + t0) * 64;       // frame 0 holds no back-pointers: staged, never looked at
        __syncthreads();
#pragma unroll 8
        for (int i = lane; i < cnt * 64; i += 64) s_bp[i] = src[i];   // plain loads, all in flight at once: the fence above ordered them
        __syncthreads();
        int mine = -1;
        align_walk<K>(s_bp, 64, cnt, t0 == 0, lane, 0, s, mine);
        const float lp = align_path_lp(em, t0, cnt, lane, b, B, Lmax, mine);
        lattice_emit_block(lp, t0, cnt, lane, mine, s, s_after, carry, total, st, fr, ts);
    }
    for (int t = n + lane; t < Tn; t += 64) st[t] = -1;
    total = wave_sum(total);
    if (lane == 0) { score[b] = total; status[b] = 0; }
}

// Where state s lives in an LDS row of form B: inside its run of 16, rotated by (run / 4).  A thread reads its run one state at a
// time, 64 bytes from its neighbour's: unrotated, the 64 lanes of a wave would meet in 4 of the 64 banks; rotated, lane 4a + r reads
// bank 16 r + ((q + a) & 15), all different.
__device__ __forceinline__ int lds_slot(int s) { return (s & ~15) | ((s + (s >> 6)) & 15); }

// ------------------------------------------------------------------ form B: one sentence, one 256-thread workgroup
// Dynamic LDS: two rows of 16 W floats (W = the runs of 16 states, S rounded up), 64 KiB at Lmax = 4,095; the backward walk
// reuses them for the back-pointers of 32 frames at a time.  Thread tid owns the runs tid and tid + 256.
__global__ __launch_bounds__(256) void ctc_align_block_kernel(const float* __restrict__ em, const int* __restrict__ in_len,
                                                              const long long* __restrict__ targets, const long long* __restrict__ tgt_len,
                                                              uint32_t* bp, int* __restrict__ states, int* __restrict__ frames,
                                                              float* __restrict__ tok_score, float* __restrict__ score,
                                                              int* __restrict__ status, int Tn, int B, int V, int Lmax, int blank, int W) {
    constexpr int K = 16, KT = 8, J = 2, FB = 32;
    extern __shared__ float dyn[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(in_len[b], 0), Tn);
    int* st = states + (long)b * Tn; int* fr = frames + (long)b * Lmax * 2; float* ts = tok_score + (long)b * Lmax;
    const long long* y = targets + (long)b * Lmax;
    const long long Lq = tgt_len[b];
    if (Lq < 0 || Lq > Lmax) { lattice_fail(2, 0, st, fr, ts, score + b, status + b, Tn, tid, 256); return; }
    const int L = (int)Lq, S = 2 * L + 1;
    int* flag = reinterpret_cast<int*>(dyn);
    if (tid == 0) *flag = 0;
    __syncthreads();
    bool bad = false;
    for (int i = tid; i < L; i += 256) { const long long c = y[i]; bad = bad || c < 0 || c >= V || c == blank; }
    if (bad) *flag = 1;
    __syncthreads();
    const bool refused = *flag != 0;
    __syncthreads();
    if (refused) { lattice_fail(2, L, st, fr, ts, score + b, status + b, Tn, tid, 256); return; }
    if (n == 0) {
        if (L > 0) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, tid, 256); return; }
        for (int t = tid; t < Tn; t += 256) st[t] = -1;
        if (tid == 0) { score[b] = 0.f; status[b] = 0; }
        return;
    }
    float* cur = dyn; float* nxt = dyn + 16 * W;
    uint32_t skip[J], live[J];
#pragma unroll
    for (int j = 0; j < J; ++j) align_run_bits<K>(y, (tid + 256 * j) * K, S, skip[j], live[j]);
    constexpr int D = 4;                                            // frames per group of requested emissions, as in form A
    float nb[D], nt[D][J][KT];
    auto fetch = [&](int tg) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float* e = em + ((long)min(tg + d, n - 1) * B + b) * (Lmax + 1);
            nb[d] = e[0];
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int q = 0; q < KT; ++q) { const int i = (tid + 256 * j) * KT + q; nt[d][j][q] = i < L ? e[1 + i] : -INFINITY; }
        }
    };
    fetch(0);
    for (int tg = 0; tg < n; tg += D) {
        float cb[D], ct[D][J][KT];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            cb[d] = nb[d];
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int q = 0; q < KT; ++q) ct[d][j][q] = nt[d][j][q];
        }
        if (tg + D < n) fetch(tg + D);
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int t = tg + d;
            if (t >= n) break;
            const float eb = cb[d];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = tid + 256 * j, s0 = c * K;
                if (c >= W) continue;
                float v[K];
                if (t == 0) {
#pragma unroll
                    for (int q = 0; q < K; ++q) v[q] = (s0 + q <= 1 && s0 + q < S) ? ((q & 1) ? ct[d][j][q >> 1] : eb) : -INFINITY;
                } else {
#pragma unroll
                    for (int q = 0; q < K; ++q) v[q] = cur[s0 + ((q + (c >> 2)) & 15)];
                    const float p1 = c > 0 ? cur[lds_slot(s0 - 1)] : -INFINITY, p2 = c > 0 ? cur[lds_slot(s0 - 2)] : -INFINITY;
                    uint32_t bits[1];
                    lattice_step<K>(v, p1, p2, ct[d][j], eb, skip[j], live[j], 0u, bits);
                    bp[((long)b * Tn + t) * W + c] = bits[0];
                }
#pragma unroll
                for (int q = 0; q < K; ++q) nxt[s0 + ((q + (c >> 2)) & 15)] = v[q];
            }
            lds_barrier();                                          // LDS only: the requested emissions and the back-pointer stores
                                                                    // stay in flight, a __syncthreads() would wait for them every frame
            float* sw = cur; cur = nxt; nxt = sw;
        }
    }
    const float e1 = cur[lds_slot(S - 1)], e2 = S >= 2 ? cur[lds_slot(S - 2)] : -INFINITY;
    int s = e2 > e1 ? S - 2 : S - 1;
    if (!(fmaxf(e1, e2) > -INFINITY)) { lattice_fail(1, L, st, fr, ts, score + b, status + b, Tn, tid, 256); return; }
    __threadfence();                                                // the back-pointers were written by other threads of this workgroup
    uint32_t* sbp = reinterpret_cast<uint32_t*>(dyn);               // FB frames x W dwords = the two rows
    int s_after = -1;
    float carry = 0.f, total = 0.f;
    for (int t0 = (n - 1) / ALN_BLOCK * ALN_BLOCK; t0 >= 0; t0 -= ALN_BLOCK) {
        const int cnt = min(ALN_BLOCK, n - t0);
        int mine = -1;
        for (int h = (cnt - 1) / FB * FB; h >= 0; h -= FB) {        // the block's later half first, FB frames staged at a time
            const int hc = min(FB, cnt - h);
            const uint32_t* src = bp + ((long)b * Tn + t0 + h) * W;  // frame 0 holds no back-pointers: staged, never looked at
            __syncthreads();
#pragma unroll 8
            for (int i = tid; i < hc * W; i += 256) sbp[i] = src[i];
            __syncthreads();
            if (tid < 64) align_walk<K>(sbp, W, hc, t0 + h == 0, tid, h, s, mine);
        }
        if (tid < 64) {
            const float lp = align_path_lp(em, t0, cnt, tid, b, B, Lmax, mine);
            lattice_emit_block(lp, t0, cnt, tid, mine, s, s_after, carry, total, st, fr, ts);
        }
    }
    for (int t = n + tid; t < Tn; t += 256) st[t] = -1;
    if (tid < 64) {
        total = wave_sum(total);
        if (tid == 0) { score[b] = total; status[b] = 0; }
    }
}

// dwords of back-pointers per (sentence, frame): form A one per lane, form B one per run of 16 states
inline int align_bp_words(int Lmax) { return 2 * Lmax + 1 <= 1024 ? 64 : (2 * Lmax + 1 + 15) / 16; }

template <int K>
void align_launch_wave(hipStream_t st, const float* em, const int* in_len, const long long* targets, const long long* tgt_len, uint32_t* bp,
                       int* states, int* frames, float* tok_score, float* score, int* status, int T, int B, int V, int Lmax, int blank) {
    hipLaunchKernelGGL(ctc_align_wave_kernel<K>, dim3(B), dim3(64), 0, st, em, in_len, targets, tgt_len, bp, states, frames, tok_score, score,
                       status, T, B, V, Lmax, blank);
}

}  // namespace

extern "C" size_t s2t_ctc_align_workspace(int T, int B, int Lmax) {
    if (T <= 0 || B <= 0 || Lmax < 0 || Lmax > S2T_CTC_ALIGN_MAX_TARGET) return 0;
    const size_t bytes = (size_t)4 * (size_t)T * (size_t)B * ((size_t)Lmax + 1 + (size_t)align_bp_words(Lmax));
    return (bytes + 255) / 256 * 256;
}

extern "C" int s2t_ctc_align(int dtype, const void* logits, const int* in_len, const long long* targets, const long long* tgt_len, void* ws,
                             int* states, int* frames, float* tok_score, float* score, int* status, int T, int B, int V, int ld, int Lmax,
                             int blank, void* stream) {
    if ((long)T * B <= 0 || T <= 0) return S2T_OK;
    if (!logits || !in_len || !targets || !tgt_len || !ws || !states || !frames || !tok_score || !score || !status) return S2T_EINVAL;
    if (V < 2 || ld < V || blank < 0 || blank >= V || Lmax < 0 || (long)T * B > 0x7fffffffL) return S2T_EINVAL;
    if ((dtype != S2T_F32 && dtype != S2T_BF16) || Lmax > S2T_CTC_ALIGN_MAX_TARGET) return S2T_ENOTSUP;
    hipStream_t st = (hipStream_t)stream;
    float* em = (float*)ws;                                         // [T*B][Lmax + 1]
    uint32_t* bp = (uint32_t*)(em + (size_t)T * B * ((size_t)Lmax + 1));      // [B][T][align_bp_words(Lmax)]
    const dim3 grid((unsigned)(((long)T * B + 3) / 4));
    if (dtype == S2T_BF16)
        hipLaunchKernelGGL(ctc_align_row_kernel<bf16>, grid, dim3(256), 0, st, (const bf16*)logits, in_len, targets, tgt_len, em, T, B, V, ld, Lmax, blank);
    else
        hipLaunchKernelGGL(ctc_align_row_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, in_len, targets, tgt_len, em, T, B, V, ld, Lmax, blank);
    S2T_LAUNCH_CHECK();
    const int S = 2 * Lmax + 1;
    ProfScope prof("ctc_align_sentences", st, 0, 0);               // the sentence phase alone (tools/ctc_segment_time.py)
#define ALN_ARGS st, em, in_len, targets, tgt_len, bp, states, frames, tok_score, score, status, T, B, V, Lmax, blank
    if (S <= 64) align_launch_wave<1>(ALN_ARGS);
    else if (S <= 128) align_launch_wave<2>(ALN_ARGS);
    else if (S <= 256) align_launch_wave<4>(ALN_ARGS);
    else if (S <= 512) align_launch_wave<8>(ALN_ARGS);
    else if (S <= 1024) align_launch_wave<16>(ALN_ARGS);
    else {
        const int W = align_bp_words(Lmax);
        hipLaunchKernelGGL(ctc_align_block_kernel, dim3(B), dim3(256), (size_t)2 * 16 * W * sizeof(float), st, em, in_len, targets, tgt_len, bp,
                           states, frames, tok_score, score, status, T, B, V, Lmax, blank, W);
    }
#undef ALN_ARGS
    S2T_LAUNCH_CHECK();
    return S2T_OK;
}
