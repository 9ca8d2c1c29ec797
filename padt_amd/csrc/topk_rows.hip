// generate(top_logprobs=k, output_patch_logprobs=True): the k best candidates of every step's processed fp32 score row with their log-probs,
// and the log-probs of the sample's own patch columns, inside the captured step — in place of keeping the (vocab + patches)-wide row.
//
// The row is the one the selection kernel read (after the logit mask, schedule, penalty, bans, the caller's processors and, under sampling,
// the warpers); it is 152 k columns for one batch and a step may have 8 rows only, so the work is split over a (chunk, row) grid:
//
//   stage 1  topk_chunk_kernel<VEC>   one 256-thread block per (TOPK_CHUNK columns, row): 16 values per thread in registers (four 16-byte
//            loads where the row start is 16-byte aligned, scalar loads otherwise), reduced to the chunk's maximum, Σ exp(v - max) over
//            its finite entries and its k best (value, column) pairs → workspace.
//   stage 2  topk_merge_kernel        one 256-thread block per row: folds the chunk (max, sum) pairs in a fixed order into the row's
//            log-sum-exp, selects the k best of the n_chunks * k candidates (staged in LDS), writes ids and v - max - log Σ at the device
//            step counter, gathers the sample's patch columns minus the same log-sum-exp, and writes the sentinels of finished rows.
//
// Selection is EXACT: a candidate is the 64-bit word (order-preserving image of the fp32 value) << 32 | ~column, so one unsigned max is
// "larger value, then lower column" — the rule of padt_greedy_step and torch.argmax (−0.0 is folded into +0.0 first: they compare equal
// there).  Words are unique per row, so "the best word below the last one I gave" enumerates a thread's values in order without a taken
// mask, the ids do not depend on the chunking, and every reduction runs in a fixed order: two launches agree bit for bit.  A NaN orders
// above +inf (torch.sort) and makes the row's log-probs NaN, as log_softmax does.
#include "block_reduce.h"
#include <math.h>

namespace {

constexpr int TOPK_CHUNK = 4096;             // columns per stage-1 block (ops.TOPK_ROWS_CHUNK): 16 per thread
constexpr int TOPK_THREADS = 256;
constexpr int TOPK_PER_THREAD = TOPK_CHUNK / TOPK_THREADS;
constexpr int TOPK_MAX_K = 32;
constexpr int TOPK_MAX_CHUNKS = 128;         // stage 2 stages n_chunks * k words in LDS: 32 KiB at the cap (rows of up to 524288 columns)
constexpr unsigned KEY_NEG_INF = 0x007fffffu;   // key of -inf: a key above it is a candidate

typedef unsigned long long u64;

// float_key (block_reduce.h) with a NaN above +inf and -0.0 folded into +0.0; key_float inverts it.  Written out: through float_key the compiler
// no longer folds `u | 0x80000000` into a source modifier, one more instruction per key (28.2 → 28.6 us for the launch pair at 64 rows, k = 5).
__device__ __forceinline__ unsigned key_of(float v) {
    if (v != v) return 0xffffffffu;
    unsigned u = v == 0.f ? 0u : __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ u64 word_of(unsigned key, int col) { return ((u64)key << 32) | (unsigned)~(unsigned)col; }

// Block-wide max of one word per thread (256 threads = 4 waves).  `red` holds 2 x 4 words used alternately by `round` parity, so one
// barrier per call is enough: a wave can only write a slot again after every wave has passed the barrier of the call in between.
__device__ __forceinline__ u64 block_max(u64 x, u64* red, int round) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const u64 y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    u64* slot = red + (round & 1) * 4;
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = x;
    __syncthreads();
    const u64 a = slot[0] > slot[1] ? slot[0] : slot[1], b = slot[2] > slot[3] ? slot[2] : slot[3];
    return a > b ? a : b;
}

// Block-wide sum in a fixed order: xor tree inside the wave, then waves 0..3 left to right.
__device__ __forceinline__ float block_sum(float x, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// Workspace of row b (u64 units): [n_chunks] (max, sum) float pairs, then [n_chunks][k] candidate words (0: no candidate).
template <bool VEC>
__global__ __launch_bounds__(TOPK_THREADS) void topk_chunk_kernel(const float* __restrict__ x, long ld, int n, int k, const int* __restrict__ unfinished,
                                                                  const int* __restrict__ step, int t_max, u64* __restrict__ ws, int n_chunks) {
    __shared__ u64 red[8];
    __shared__ float red_f[4];
    const int t = *step;
    const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (t < 0 || t >= t_max || !unfinished[b]) return;           // stage 2 does not read a finished row's workspace
    const float* row = x + (long)b * ld;
    const int col0 = c * TOPK_CHUNK;
    unsigned key[TOPK_PER_THREAD];
    // column of register i: VEC — float4 number (i / 4) * 256 + tid of the chunk, element i % 4; scalar — i * 256 + tid
    auto col_of = [&](int i) { return col0 + (VEC ? (((i >> 2) * TOPK_THREADS + tid) << 2) + (i & 3) : i * TOPK_THREADS + tid); };
    if (VEC) {
#pragma unroll
        for (int q = 0; q < TOPK_PER_THREAD / 4; ++q) {
            const int cq = col0 + ((q * TOPK_THREADS + tid) << 2);
            float v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            if (cq + 3 < n) {
                const float4 f = *reinterpret_cast<const float4*>(row + cq);
                v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (cq + e < n) v[e] = row[cq + e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) key[q * 4 + e] = key_of(v[e]);
        }
    } else {
#pragma unroll
        for (int i = 0; i < TOPK_PER_THREAD; ++i) {
            const int ci = col0 + i * TOPK_THREADS + tid;
            key[i] = key_of(ci < n ? row[ci] : -INFINITY);
        }
    }
    // a column at or past n was loaded as -inf: never a candidate, nothing in the sum
    u64 mine = 0;
#pragma unroll
    for (int i = 0; i < TOPK_PER_THREAD; ++i) {
        const u64 w = key[i] > KEY_NEG_INF ? word_of(key[i], col_of(i)) : 0;
        mine = w > mine ? w : mine;
    }
    u64* wrow = ws + (long)b * n_chunks * (1 + k);
    u64* cand = wrow + n_chunks + (long)c * k;
    u64 best = block_max(mine, red, 0);                          // round 0 is also the chunk's maximum
    const float m = best ? key_float((unsigned)(best >> 32)) : -INFINITY;
    float s = 0.f;
    if (best) {
#pragma unroll
        for (int i = 0; i < TOPK_PER_THREAD; ++i)
            if (key[i] > KEY_NEG_INF) s += __builtin_amdgcn_exp2f((key_float(key[i]) - m) * 1.44269504088896341f);
    }
    s = block_sum(s, red_f);
    if (tid == 0) {
        float2 ms; ms.x = m; ms.y = s;
        *reinterpret_cast<float2*>(wrow + c) = ms;
    }
    for (int j = 0; j < k; ++j) {
        if (j) best = block_max(mine, red, j);
        if (tid == 0) cand[j] = best;
        if (best == 0) {                                         // block-uniform: the chunk has fewer than k candidates
            if (tid == 0) for (int r = j + 1; r < k; ++r) cand[r] = 0;
            break;
        }
        if (mine == best) {                                      // one thread: its next value below the one just given
            u64 nxt = 0;
#pragma unroll
            for (int i = 0; i < TOPK_PER_THREAD; ++i) {
                const u64 w = key[i] > KEY_NEG_INF ? word_of(key[i], col_of(i)) : 0;
                nxt = (w < best && w > nxt) ? w : nxt;
            }
            mine = nxt;
        }
    }
}

__global__ __launch_bounds__(TOPK_THREADS) void topk_merge_kernel(const float* __restrict__ x, long ld, int n, int k, const int* __restrict__ unfinished,
                                                                  const int* __restrict__ step, int t_max, int* __restrict__ top_idx,
                                                                  float* __restrict__ top_val, const int* __restrict__ vrt_off, int vocab,
                                                                  float* __restrict__ patch_lp, int p_cap, const u64* __restrict__ ws, int n_chunks) {
    extern __shared__ u64 lds_cand[];                            // n_chunks * k words
    __shared__ u64 red[8];
    __shared__ float red_f[4];
    const int t = *step;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (t < 0 || t >= t_max) return;
    int* oi = top_idx ? top_idx + ((long)b * t_max + t) * k : nullptr;
    float* ov = top_val ? top_val + ((long)b * t_max + t) * k : nullptr;
    float* op = patch_lp ? patch_lp + ((long)b * t_max + t) * p_cap : nullptr;
    if (!unfinished[b]) {                                        // after the row's EOS: the sentinels in every slot
        if (oi) for (int j = tid; j < k; j += TOPK_THREADS) { oi[j] = -1; ov[j] = -INFINITY; }
        if (op) for (int j = tid; j < p_cap; j += TOPK_THREADS) op[j] = -INFINITY;
        return;
    }
    const u64* wrow = ws + (long)b * n_chunks * (1 + k);
    // the row's log-sum-exp from the chunk pairs: thread c holds chunk c (n_chunks <= 128 < 256)
    float m = -INFINITY, s = 0.f;
    if (tid < n_chunks) {
        const float2 ms = *reinterpret_cast<const float2*>(wrow + tid);
        m = ms.x; s = ms.y;
    }
    const u64 mw = block_max((u64)key_of(m), red, 0);
    const float M = key_float((unsigned)mw);
    float part = 0.f;
    if (tid < n_chunks && m != -INFINITY) part = s * __builtin_amdgcn_exp2f((m - M) * 1.44269504088896341f);
    const float S = block_sum(part, red_f);
    const bool any = M != -INFINITY;                             // false: every column is -inf, the row has no candidate
    const float logS = any ? logf(S) : 0.f;
    if (op) {
        const int p0 = vrt_off[b], np = vrt_off[b + 1] - p0;
        const float* row = x + (long)b * ld;
        for (int j = tid; j < p_cap; j += TOPK_THREADS) {
            const long col = (long)vocab + p0 + j;
            float lp = -INFINITY;
            if (any && j < np && col >= 0 && col < n) {
                const float v = row[col];
                lp = v == -INFINITY ? -INFINITY : (v - M) - logS;
            }
            op[j] = lp;
        }
    }
    if (k == 0) return;
    const int n_cand = n_chunks * k;
    const u64* cand = wrow + n_chunks;
    u64 mine = 0;
    for (int i = tid; i < n_cand; i += TOPK_THREADS) {
        const u64 w = cand[i];
        lds_cand[i] = w;
        mine = w > mine ? w : mine;
    }
    // a thread re-reads only the words it wrote itself: no barrier is needed before the rounds
    for (int j = 0; j < k; ++j) {
        const u64 best = block_max(mine, red, j + 1);
        if (best == 0) {                                         // fewer than k finite candidates: id -1, log-prob -inf in the rest
            for (int r = j + tid; r < k; r += TOPK_THREADS) { oi[r] = -1; ov[r] = -INFINITY; }
            break;
        }
        if (tid == 0) {
            oi[j] = (int)~(unsigned)best;
            ov[j] = (key_float((unsigned)(best >> 32)) - M) - logS;
        }
        if (mine == best) {
            u64 nxt = 0;
            for (int i = tid; i < n_cand; i += TOPK_THREADS) {
                const u64 w = lds_cand[i];
                nxt = (w < best && w > nxt) ? w : nxt;
            }
            mine = nxt;
        }
    }
}

inline long topk_chunks(long n_cols) { return (n_cols + TOPK_CHUNK - 1) / TOPK_CHUNK; }

}  // namespace

extern "C" long padt_topk_rows_chunk(void) { return TOPK_CHUNK; }

extern "C" long padt_topk_rows_workspace(long n_cols, long k, long batch) {
    if (n_cols <= 0 || k < 0 || k > TOPK_MAX_K || batch <= 0) return 0;
    return batch * topk_chunks(n_cols) * (1 + k) * (long)sizeof(u64);
}

extern "C" int padt_topk_logprob_rows_f32(void* stream, const void* rows_f32, long ld, long n_cols, long k, const int* unfinished, const int* step,
                                          long t_max, void* top_idx, void* top_val, const int* vrt_off, long vocab, void* patch_lp, long p_cap,
                                          void* workspace, long batch) {
    if (batch <= 0) return 0;
    if (k < 0 || k > TOPK_MAX_K) { padt_set_error("padt_topk_logprob_rows_f32: 0 <= k <= 32 required"); return -1; }
    if (rows_f32 == nullptr || ((size_t)rows_f32 & 3) || n_cols <= 0 || ld < n_cols || unfinished == nullptr || step == nullptr || t_max <= 0 ||
        t_max > 0x7fffffffL || workspace == nullptr || ((size_t)workspace & 7) || batch > 65535) {
        padt_set_error("padt_topk_logprob_rows_f32: score rows (ld >= n_cols), the unfinished flags, the step counter, a workspace of "
                       "padt_topk_rows_workspace bytes and batch <= 65535 are required");
        return -1;
    }
    if (topk_chunks(n_cols) > TOPK_MAX_CHUNKS) { padt_set_error("padt_topk_logprob_rows_f32: rows of at most 524288 columns"); return -1; }
    if ((k > 0) != (top_idx != nullptr) || (k > 0) != (top_val != nullptr)) {
        padt_set_error("padt_topk_logprob_rows_f32: top_idx and top_val [batch][t_max][k] are required with k > 0 and null with k == 0");
        return -1;
    }
    if (patch_lp != nullptr && (vrt_off == nullptr || p_cap <= 0 || p_cap > 0x7fffffffL || vocab < 0 || vocab > 0x7fffffffL)) {
        padt_set_error("padt_topk_logprob_rows_f32: patch_lp [batch][t_max][p_cap] needs vrt_off [batch + 1], vocab and p_cap > 0");
        return -1;
    }
    if (k == 0 && patch_lp == nullptr) { padt_set_error("padt_topk_logprob_rows_f32: k == 0 and no patch_lp: nothing to compute"); return -1; }
    const int nc = (int)topk_chunks(n_cols);
    const dim3 grid1((unsigned)nc, (unsigned)batch);
    const bool vec = (((size_t)rows_f32 & 15) == 0) && (ld & 3) == 0;       // every row (and chunk) start is 16-byte aligned
    if (vec)
        hipLaunchKernelGGL(topk_chunk_kernel<true>, grid1, dim3(TOPK_THREADS), 0, (hipStream_t)stream, (const float*)rows_f32, ld, (int)n_cols, (int)k,
                           unfinished, step, (int)t_max, (u64*)workspace, nc);
    else
        hipLaunchKernelGGL(topk_chunk_kernel<false>, grid1, dim3(TOPK_THREADS), 0, (hipStream_t)stream, (const float*)rows_f32, ld, (int)n_cols, (int)k,
                           unfinished, step, (int)t_max, (u64*)workspace, nc);
    PADT_CHECK_LAUNCH();
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)batch), dim3(TOPK_THREADS), (size_t)nc * k * sizeof(u64), (hipStream_t)stream,
                       (const float*)rows_f32, ld, (int)n_cols, (int)k, unfinished, step, (int)t_max, (int*)top_idx, (float*)top_val, vrt_off,
                       (int)vocab, (float*)patch_lp, (int)p_cap, (const u64*)workspace, nc);
    PADT_CHECK_LAUNCH();
    return 0;
}
