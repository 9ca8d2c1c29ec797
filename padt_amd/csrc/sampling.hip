// Token selection over fp32 score rows: the sampling branch of the decode loop (temperature / top-k / top-p and the Gumbel-max draw; HF's
// later warpers), the row arg-max of the hooked loop and the row log-probs.  Each kernel leaves one (value, index) partial per row in the
// layout padt_greedy_step (decode_step.hip) reads with nblk = 1.  Type-independent: compiled once.
//
// Sampling branch of the loop (padt.py:740-743: probs = softmax(next_token_scores); next = multinomial(probs, 1)) with HF's
// logits warpers (generation/logits_process.py: Temperature → TopK → TopP, the order _get_logits_processor builds at padt.py:570-580).
// One block per row over the fp32 logits the head kernel wrote (mask / repetition penalty / scripted mode already applied):
//   top-k: exact k-th largest by a 4-pass radix select on order-preserving keys; everything >= it stays (HF keeps ties);
//   top-p: the survivors STRICTLY above the k-th largest value (<= k - 1 <= 1023: top_p needs top_k) are sorted in LDS; rank r stays
//          iff the probability mass of the ranks before it is < top_p (= HF's "remove ascending-cumulative <= 1 - top_p", at least one
//          token kept).  The entries EQUAL to the k-th value (any number of them: one exact tie already makes k + 1 survivors) all carry
//          the same probability and come after every sorted rank: they are one block with a count, of which the lowest-index j stay,
//          j = the number of tied ranks whose mass-before is < top_p — the order (value descending, index ascending) of a full sort;
//   draw:  Gumbel-max — argmax((l - max)/T + g), g = -log(-log u), u from a counter-based hash of (seed, step, row, index) —
//          an exact multinomial draw from softmax(l/T) over the survivors without normalising or building a CDF.
// The draws cannot match torch.multinomial's (different generator); the DISTRIBUTION is what the tests check.
// gen->write_back: the row is then overwritten with the warped scores HF's samplers see (padt.py:717-720: the warpers are part of
// logits_processor, so `scores` and the stopping criteria get them): l / T (a true fp32 division, HF's TemperatureLogitsWarper) on the
// kept entries, -inf everywhere else in [0, n).
#include "block_reduce.h"
#include "gen_cfg.h"

namespace PADT_NS {

PADT_DEV unsigned hash32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
PADT_DEV float gumbel_noise(unsigned seed, unsigned step, unsigned row, unsigned idx) {
    unsigned x = hash32(idx * 0x9E3779B1u + seed);
    x = hash32(x ^ (row * 0x85EBCA77u + step * 0xC2B2AE3Du + 0x68bc21ebu));
    // 23 random bits: (x >> 9) + 0.5 is exact in fp32 (24 would round 2^24 - 0.5 up to 2^24 → u = 1 → g = +inf, a uniformly random
    // token once per 2^24 candidates: 0.9 % per step over a 152k-row table with top_k = 0) → u in [2^-24, 1 - 2^-24], g finite
    const float u = ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f);
    return -logf(-logf(u));
}

__global__ __launch_bounds__(1024) void sample_token_kernel(float* logits, long ld, int n, const GenCfg* __restrict__ g,
                                                            const int* __restrict__ step, float* __restrict__ out_val,
                                                            int* __restrict__ out_idx, int vocab, const int* __restrict__ vrt_off,
                                                            const int* __restrict__ row_base) {
    __shared__ unsigned hist[256];                                        // radix histogram; then the per-wave tie counts of the cut search
    __shared__ unsigned sel[2];                                           // chosen bin, remaining rank
    __shared__ float sval[1024];
    __shared__ int sidx[1024];
    __shared__ float red_v[1024];
    __shared__ int red_i[1024];
    __shared__ int cnt, n_tie, tie_keep, tie_last;                        // sorted ranks; tied entries, how many stay, index of the last kept
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = logits + (long)b * ld;
    const float T = g->temperature > 0.f ? g->temperature : 1.f;
    const int k = g->top_k;
    const float top_p = g->top_p;
    const unsigned seed = g->seed, st = step ? (unsigned)*step : 0u;
    // the generator's (row, index) counter in the numbering of the row's own batch (padt_sample_token_keyed): a batch of a merged decode
    // group draws what it draws alone; without row_base: (b, column)
    int rb = row_base ? row_base[b] : 0;
    rb = (rb < 0 || rb > b) ? 0 : rb;                                     // an index read from device memory: vrt_off[rb] stays inside [0, batch]
    const unsigned key_row = (unsigned)(b - rb);
    const int col0 = row_base ? vrt_off[rb] : 0;
    auto key_col = [&](int i) { return (unsigned)(i >= vocab && row_base ? i - col0 : i); };
    // ---- top-k threshold (key of the k-th largest entry), or keep everything finite
    unsigned thresh = float_key(-INFINITY) + 1u;                          // any finite value
    if (k > 0 && k < n) {
        unsigned prefix = 0u, mask = 0u, remaining = (unsigned)k;
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = pass * 8;
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            for (int i = tid; i < n; i += 1024) {
                const unsigned key = float_key(row[i]);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0u;
                int bin = 255;
                for (; bin > 0; --bin) {
                    if (cum + hist[bin] >= remaining) break;
                    cum += hist[bin];
                }
                sel[0] = (unsigned)bin;
                sel[1] = remaining - cum;
            }
            __syncthreads();
            prefix |= sel[0] << shift;
            mask |= 0xffu << shift;
            remaining = sel[1];
            __syncthreads();
        }
        if (prefix > thresh) thresh = prefix;                             // fewer than k finite entries: -inf stays out
    }
    // ---- row maximum over the survivors (for the exponentials)
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 1024) {
        const float v = row[i];
        if (float_key(v) >= thresh) mx = fmaxf(mx, v);
    }
    mx = block_max_lds<1024>(mx, red_v);
    __syncthreads();
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    const bool nucleus = top_p < 1.0f && k > 0 && k <= 1024;
    int n_keep = 0;                                                       // nucleus: kept sorted ranks (a prefix of the sort)
    if (nucleus) {
        // ---- nucleus over the top-k survivors: gather the entries above the threshold (< k <= 1024 of them; k >= n: n <= 1024), sort
        //      descending, prefix mass, Gumbel over the kept ranks; the entries at the threshold are one block (see above)
        if (tid == 0) { cnt = 0; n_tie = 0; }
        sval[tid] = -INFINITY;
        sidx[tid] = 0x7fffffff;
        __syncthreads();
        for (int i = tid; i < n; i += 1024) {
            const float v = row[i];
            const unsigned key = float_key(v);
            if (key > thresh) {
                const int slot = atomicAdd(&cnt, 1);
                if (slot < 1024) { sval[slot] = v; sidx[slot] = i; }
            } else if (key == thresh) {
                atomicAdd(&n_tie, 1);
            }
        }
        __syncthreads();
        for (int size = 2; size <= 1024; size <<= 1)                        // bitonic sort, descending by (value, then lower index first)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                const int j = tid ^ stride;
                if (j > tid) {
                    const bool desc = (tid & size) == 0;
                    const float a = sval[tid], c = sval[j];
                    const int ai = sidx[tid], ci = sidx[j];
                    const bool a_first = (a > c) || (a == c && ai < ci);
                    if (a_first != desc) { sval[tid] = c; sval[j] = a; sidx[tid] = ci; sidx[j] = ai; }
                }
                __syncthreads();
            }
        const float pv = sval[tid] > -INFINITY ? expf((sval[tid] - mx) / T) : 0.f;
        red_v[tid] = pv;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {                          // inclusive scan
            const float add = tid >= off ? red_v[tid - off] : 0.f;
            __syncthreads();
            red_v[tid] += add;
            __syncthreads();
        }
        const float S = red_v[1023];                                      // mass above the threshold (no tie: the total, bit for bit as before)
        const float tv = key_float(thresh);                               // the tied value (finite: thresh > key(-inf))
        const float et = n_tie > 0 ? expf((tv - mx) / T) : 0.f;           // mass of ONE tied entry
        const float total = S + (float)n_tie * et;
        const float before = (red_v[tid] - pv) / total;                   // probability mass of the ranks before this one
        const bool keep = sval[tid] > -INFINITY && (tid == 0 || before < top_p);
        n_keep = __syncthreads_count(keep);
        if (tid == 0) {
            // tied rank j (0-based, ascending index) has mass-before (S + j et) / total, non-decreasing in j: the kept ones are those below the
            // first j whose mass-before is >= top_p; none when a sorted rank was already cut, at least one when nothing lies above the threshold
            int lo = 0, hi = n_tie;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if ((S + (float)mid * et) / total < top_p) lo = mid + 1;
                else hi = mid;
            }
            if (n_keep < cnt) lo = 0;
            if (cnt == 0 && n_tie > 0 && lo == 0) lo = 1;
            tie_keep = lo;
            tie_last = lo == n_tie ? 0x7fffffff : -1;
        }
        __syncthreads();
        const int jk = tie_keep;
        if (jk > 0 && jk < n_tie) {
            // index of the jk-th tied entry: count the tied entries of consecutive 1024-column chunks (ballot per wave, 16 wave counts)
            int seen = 0;
            for (int c0 = 0; c0 < n && seen < jk; c0 += 1024) {
                const int i = c0 + tid;
                const bool t = i < n && float_key(row[i]) == thresh;
                const unsigned long long bal = __ballot(t);
                if (lane == 0) hist[wave] = (unsigned)__popcll(bal);
                __syncthreads();
                int pre = 0, tot = 0;
#pragma unroll
                for (int w = 0; w < 16; ++w) { pre += w < wave ? (int)hist[w] : 0; tot += (int)hist[w]; }
                if (t && seen + pre + __popcll(bal & ((1ull << lane) - 1ull)) == jk - 1) tie_last = i;
                seen += tot;
                __syncthreads();
            }
            __syncthreads();
        }
        if (keep) {
            best = (sval[tid] - mx) / T + gumbel_noise(seed, st, key_row, key_col(sidx[tid]));
            bidx = sidx[tid];
        }
        if (jk > 0) {
            const int last = tie_last;
            for (int i = tid; i < n && i <= last; i += 1024) {
                if (float_key(row[i]) == thresh) {
                    const float sc = (tv - mx) / T + gumbel_noise(seed, st, key_row, key_col(i));
                    if (argmax_less(best, bidx, sc, i)) { best = sc; bidx = i; }
                }
            }
        }
    } else {
        for (int i = tid; i < n; i += 1024) {
            const float v = row[i];
            if (float_key(v) >= thresh) {
                const float sc = (v - mx) / T + gumbel_noise(seed, st, key_row, key_col(i));
                if (argmax_less(best, bidx, sc, i)) { best = sc; bidx = i; }
            }
        }
    }
    __syncthreads();
    block_argmax_lds<1024>(best, bidx, red_v, red_i);
    if (tid == 0) { out_val[b] = red_v[0]; out_idx[b] = red_i[0]; }
    if (g->write_back) {                                                  // every read of the row is behind the barriers above
        const float lv = n_keep > 0 ? sval[n_keep - 1] : INFINITY;       // nucleus: last kept sorted rank (value, index)
        const int li = n_keep > 0 ? sidx[n_keep - 1] : -1;
        const int last = nucleus ? tie_last : 0x7fffffff;
        constexpr int WU = 8;                                             // loads in flight per thread before the stores
        for (int i0 = tid; i0 < n; i0 += WU * 1024) {
            float v[WU];
#pragma unroll
            for (int u = 0; u < WU; ++u) v[u] = i0 + u * 1024 < n ? row[i0 + u * 1024] : 0.f;
#pragma unroll
            for (int u = 0; u < WU; ++u) {
                const int i = i0 + u * 1024;
                const unsigned key = float_key(v[u]);
                const bool kept = !nucleus ? key >= thresh
                                : key > thresh ? (v[u] > lv || (v[u] == lv && i <= li)) : (key == thresh && i <= last);
                if (i < n) row[i] = kept ? v[u] / T : -INFINITY;
            }
        }
    }
}

// next token per row by multinomial sampling from the warped logits; writes one (value, index) "partial" per row in the layout
// padt_greedy_step reads with nblk = 1, so the bookkeeping kernel is shared with the greedy path.  With gen_cfg's write_back set the rows
// are overwritten with the warped scores (see sample_token_kernel).
extern "C" int padt_sample_token(void* stream, void* logits_f32, long ld_logits, long n_rows_table, const void* gen_cfg,
                                 const int* step, void* part_val, void* part_idx, long batch) {
    if (batch <= 0) return 0;
    if (gen_cfg == nullptr || n_rows_table <= 0 || n_rows_table > 0x7fffffffL) { padt_set_error("padt_sample_token: gen_cfg and a table size are required"); return -1; }
    hipLaunchKernelGGL(sample_token_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, (float*)logits_f32, ld_logits,
                       (int)n_rows_table, (const GenCfg*)gen_cfg, step, (float*)part_val, (int*)part_idx, 0, (const int*)nullptr,
                       (const int*)nullptr);
    PADT_CHECK_LAUNCH();
    return 0;
}

// padt_sample_token with the generator keyed like padt_warp_sample_rows_f32's: row_base[b] = the first row of b's own batch inside a merged
// decode group, vrt_off [batch + 1], vocab — the draw of row b, column c uses (b - row_base[b], c >= vocab ? c - vrt_off[row_base[b]] : c), the
// numbers the batch has alone.  row_base null: padt_sample_token.
extern "C" int padt_sample_token_keyed(void* stream, void* logits_f32, long ld_logits, long n_rows_table, const void* gen_cfg,
                                       const int* step, void* part_val, void* part_idx, long batch, long vocab, const int* vrt_off,
                                       const int* row_base) {
    if (batch <= 0) return 0;
    if (gen_cfg == nullptr || n_rows_table <= 0 || n_rows_table > 0x7fffffffL) { padt_set_error("padt_sample_token_keyed: gen_cfg and a table size are required"); return -1; }
    if (row_base != nullptr && (vrt_off == nullptr || vocab < 0 || vocab > n_rows_table)) {
        padt_set_error("padt_sample_token_keyed: row_base needs vrt_off and 0 <= vocab <= n_rows_table");
        return -1;
    }
    hipLaunchKernelGGL(sample_token_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, (float*)logits_f32, ld_logits,
                       (int)n_rows_table, (const GenCfg*)gen_cfg, step, (float*)part_val, (int*)part_idx, (int)vocab, vrt_off, row_base);
    PADT_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// HF's warpers AFTER top-p (generation/logits_process.py, the order _get_logits_processor builds: MinP → Typical → Epsilon → Eta, each with
// min_tokens_to_keep = 1) and the draw, over the fp32 rows sample_token_kernel left with write_back: l / T on the top-k / top-p survivors, -inf
// elsewhere.  One block per row, in place; every warper takes its softmax over the survivors of the stage before it (the finite entries):
//   min_p:    drop p_i < min_p · p_max  ⇔  v_i - max < log min_p  (no sum needed; the top entries always stay);
//   typical:  H = -Σ p log p, key_i = |-log p_i - H|; keep the keys <= the key of the first rank (ascending key) whose cumulative mass is
//             >= typical_p.  No sort: an MSB-first radix select over the bits of the non-negative fp32 key (order-preserving as unsigned), whose
//             256-bin histograms accumulate probability MASS — as 2^-48 fixed-point integers, so that the sums are exact, the four passes agree
//             with each other whatever order the LDS atomics arrive in, and a replay repeats bit for bit.  Four passes descend into the bin where
//             the cumulative mass crosses typical_p; entries with the cut's key all stay (HF removes `>` only);
//   epsilon:  drop p_i < ε unless the entry has the row's top score;
//   eta:      η = min(ε, sqrt(ε) · exp(-H)), drop p_i < η unless the entry has the row's top score.
// Sums (Σ e, Σ e·(v - max), e = expf(v - max)) are accumulated in fp64 in a fixed order (strided columns per thread, shuffles, 16 wave
// partials); thresholds are compared in fp64 on v - max, so a decision differs from an exact evaluation of the fp32 row only where it lies
// within fp32 rounding of its threshold.  A compare pass also accumulates the sums of what it keeps — the next stage's statistics; only the
// typical warper can remove the row's top entry, after which the maximum (and then the sums) are taken again.
// Passes: one over the row for the maximum and a survivor count per thread; when at most WARP_LIST_CAP entries survive (always under
// top-k <= 1024) a second copies them to LDS in a fixed order (by thread, then in the thread's sweep order) and every stage runs on that list,
// writing only its -inf into the row.  Otherwise min_p, when active, runs over the row in place, counts again and usually leaves few enough
// for the list; what still does not fit is warped by sweeps over the L2-resident row itself.  A thread owns the same columns in every sweep
// (16-byte loads when the row starts 16-byte aligned).  Columns >= n are never touched.
// Draw: Gumbel-max over the final survivors, argmax(v - max + g) with sample_token_kernel's counter hash of (seed, step, row, index) — an exact
// multinomial draw from softmax(row); ties → the lower index.  A row without a finite entry yields (-inf, sentinel index) as
// sample_token_kernel does, which padt_greedy_step turns into the pad token.
PADT_DEV float warp_block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();                                                      // `red` may still be read by a previous call
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    return m;
}
PADT_DEV void warp_block_sum2(double& a, double& c, double* red) {      // red: [2][16]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); c += __shfl_xor(c, o); }
    __syncthreads();
    if (lane == 0) { red[wave] = a; red[16 + wave] = c; }
    __syncthreads();
    double sa = 0.0, sc = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { sa += red[w]; sc += red[16 + w]; }
    a = sa; c = sc;
}
PADT_DEV unsigned typical_key(float v, float mx, double logS, double H) {  // bits of |-log p - H| >= 0: ascending as unsigned; NaN sorts last
    const double nlp = logS - ((double)v - (double)mx);
    return __builtin_bit_cast(unsigned, (float)fabs(nlp - H)) & 0x7fffffffu;
}

constexpr int WARP_LIST_CAP = 4096;                                       // survivors the LDS list holds (32 KiB)
constexpr int WARP_LOADS = 8;                                             // loads in flight per thread, scalar or 16-byte

// f(j, v) for this thread's finite elements of a list of m floats (elements tid, tid + 1024, ...), WARP_LOADS loads in flight; f may overwrite element j
template <class F>
PADT_DEV void warp_sweep_list(const float* lv, int m, int tid, F f) {
    for (int j0 = tid; j0 < m; j0 += WARP_LOADS * 1024) {
        float v[WARP_LOADS];
#pragma unroll
        for (int u = 0; u < WARP_LOADS; ++u) v[u] = j0 + u * 1024 < m ? lv[j0 + u * 1024] : -INFINITY;
#pragma unroll
        for (int u = 0; u < WARP_LOADS; ++u)
            if (j0 + u * 1024 < m && v[u] != -INFINITY) f(j0 + u * 1024, v[u]);
    }
}
// The same over the row in memory.  vec (the row starts 16-byte aligned): a thread owns the 4-column groups tid, tid + 1024, ... and loads each
// with one 16-byte load, the thread after the last whole group owns the up to 3 columns left; otherwise it owns the columns tid, tid + 1024, ...
// Either way a thread owns the same columns in every sweep of a launch and meets them in the same order.
template <class F>
PADT_DEV void warp_sweep_row(const float* row, int n, int tid, bool vec, F f) {
    if (!vec) { warp_sweep_list(row, n, tid, f); return; }
    const int nq = n >> 2;
    const f32x4* row4 = reinterpret_cast<const f32x4*>(row);
    for (int q0 = tid; q0 < nq; q0 += WARP_LOADS * 1024) {
        f32x4 v[WARP_LOADS];
#pragma unroll
        for (int u = 0; u < WARP_LOADS; ++u)
            v[u] = q0 + u * 1024 < nq ? row4[q0 + u * 1024] : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int u = 0; u < WARP_LOADS; ++u) {
            const int q = q0 + u * 1024;
            if (q < nq) {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (v[u][c] != -INFINITY) f(4 * q + c, v[u][c]);
            }
        }
    }
    if (tid == (nq & 1023))
        for (int j = 4 * nq; j < n; ++j) {
            const float v = row[j];
            if (v != -INFINITY) f(j, v);
        }
}
// exclusive prefix of `mine` over the block's threads (→ at) and the block's total; red: 16 ints
PADT_DEV void warp_block_scan(int mine, int& at, int& total, int* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) red[wave] = inc;
    __syncthreads();
    at = inc - mine;
    total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) { at += w < wave ? red[w] : 0; total += red[w]; }
}

__global__ __launch_bounds__(1024) void warp_sample_rows_kernel(float* rows, long ld, int n, const GenCfg* __restrict__ g,
                                                                const int* __restrict__ step, float* __restrict__ out_val,
                                                                int* __restrict__ out_idx, int vocab, const int* __restrict__ vrt_off,
                                                                const int* __restrict__ row_base) {
    __shared__ unsigned long long hist[256];                              // probability mass per radix bin, 2^-48 fixed point
    __shared__ unsigned long long wave_tot[4];
    __shared__ unsigned long long sel[2];                                 // chosen bin, mass still to cover inside it
    __shared__ double red_d[32];
    __shared__ float red_f[16];
    __shared__ int red_i[16];
    __shared__ float lv[WARP_LIST_CAP];                                   // the survivors' values and columns, when they fit
    __shared__ int li[WARP_LIST_CAP];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* row = rows + (long)b * ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const float min_p = g->min_p, typ = g->typical_p, eps = g->epsilon_cutoff, eta_eps = g->eta_cutoff;
    const unsigned seed = g->seed, st = step ? (unsigned)*step : 0u;
    // the generator's (row, index) counter in the numbering of the row's own batch: a batch of a merged decode group draws what it draws alone
    int rb = row_base ? row_base[b] : 0;
    rb = (rb < 0 || rb > b) ? 0 : rb;                                     // an index read from device memory: vrt_off[rb] stays inside [0, batch]
    const unsigned key_row = (unsigned)(b - rb);
    const int col0 = row_base ? vrt_off[rb] : 0;

    // ---- the maximum and this thread's survivor count, in one pass over the row
    float lm = -INFINITY;
    int mine = 0;
    warp_sweep_row(row, n, tid, vec, [&](int, float v) { lm = fmaxf(lm, v); ++mine; });
    float mx = warp_block_max(lm, red_f);
    if (mx == -INFINITY) {                                                // no candidate (uniform over the block)
        if (tid == 0) { out_val[b] = -INFINITY; out_idx[b] = 0x7fffffff; }
        return;
    }
    int at, total;
    warp_block_scan(mine, at, total, red_i);
    // survivors → LDS list in a fixed order (by thread, then in the thread's sweep order); called with total <= WARP_LIST_CAP, and `at` stays below total
    auto to_list = [&]() {
        warp_sweep_row(row, n, tid, vec, [&](int j, float v) {
            lv[at] = v; li[at] = j;
            ++at;
        });
        __syncthreads();
    };
    double S = 0.0, E = 0.0;                                              // Σ e and Σ e (v - mx) over the survivors, once have_sums
    bool have_sums = false;
    const bool min_p_on = min_p > 0.f && min_p <= 1.f;
    bool min_p_done = !min_p_on;
    bool compact = total <= WARP_LIST_CAP;
    if (compact) {
        to_list();
    } else if (min_p_on) {
        // too many for the list: min_p in place, with the sums of what stays and a new count — it usually leaves few enough
        const double thr = log((double)min_p);
        mine = 0;
        warp_sweep_row(row, n, tid, vec, [&](int j, float v) {
            if ((double)v - (double)mx < thr) { row[j] = -INFINITY; return; }
            const float d = v - mx, ex = expf(d);
            S += (double)ex;
            E += (double)ex * (double)d;
            ++mine;
        });
        warp_block_sum2(S, E, red_d);
        have_sums = min_p_done = true;
        warp_block_scan(mine, at, total, red_i);
        compact = total <= WARP_LIST_CAP;
        if (compact) to_list();
    }
    const int m = compact ? total : n;
    // f(j, v) over the survivors: list entries or columns; drop(j) removes one (a thread drops only what its own sweep handed it)
    auto sweep = [&](auto f) {
        if (compact) warp_sweep_list(lv, m, tid, f);
        else warp_sweep_row(row, n, tid, vec, f);
    };
    auto column = [&](int j) { return compact ? li[j] : j; };
    auto drop = [&](int j) {
        if (compact) { lv[j] = -INFINITY; row[li[j]] = -INFINITY; }
        else row[j] = -INFINITY;
    };
    auto sums = [&]() {
        double s = 0.0, e = 0.0;
        sweep([&](int, float v) {
            const float d = v - mx, ex = expf(d);
            s += (double)ex;
            e += (double)ex * (double)d;
        });
        warp_block_sum2(s, e, red_d);
        S = s; E = e; have_sums = true;
    };
    // drop (v - mx) < thr unless v is the row's top score; accumulates the sums of what stays
    auto threshold_stage = [&](double thr) {
        double s = 0.0, e = 0.0;
        sweep([&](int j, float v) {
            if ((double)v - (double)mx < thr && v != mx) { drop(j); return; }
            const float d = v - mx, ex = expf(d);
            s += (double)ex;
            e += (double)ex * (double)d;
        });
        warp_block_sum2(s, e, red_d);
        S = s; E = e; have_sums = true;
    };

    if (!min_p_done) threshold_stage(log((double)min_p));

    if (typ > 0.f && typ < 1.f) {
        if (!have_sums) sums();
        const double logS = log(S), H = logS - E / S;
        const float scale = (float)(281474976710656.0 / S);              // 2^48 / S: S >= 1 (the top entry adds 1), a mass is at most 2^48
        unsigned prefix = 0u, mask = 0u;
        unsigned long long remaining = 0ull;
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = pass * 8;
            __syncthreads();
            if (tid < 256) hist[tid] = 0ull;
            __syncthreads();
            sweep([&](int, float v) {
                const unsigned key = typical_key(v, mx, logS, H);
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], (unsigned long long)(expf(v - mx) * scale));
            });
            __syncthreads();
            // exclusive prefix over the 256 bins (threads 0..255: shuffles within a wave, 4 wave totals), ascending key
            const unsigned long long h = tid < 256 ? hist[tid] : 0ull;
            unsigned long long cum = h;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned long long t = __shfl_up(cum, o);
                if (lane >= o) cum += t;
            }
            if (tid < 256 && lane == 63) wave_tot[wave] = cum;
            if (tid == 0) { sel[0] = 255ull; sel[1] = 0ull; }             // unreachable target (a NaN row): the last bin
            __syncthreads();
            if (pass == 3) {                                              // the row's whole mass Q and the target ceil(typical_p · Q) in [1, Q]
                const unsigned long long Q = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
                unsigned long long tq = (unsigned long long)ceil((double)typ * (double)Q);
                tq = tq > Q ? Q : tq;
                remaining = tq < 1ull ? 1ull : tq;
            }
            if (tid < 256) {
                unsigned long long before = cum - h;
                for (int w = 0; w < wave; ++w) before += wave_tot[w];
                if (h > 0ull && before < remaining && remaining <= before + h) { sel[0] = (unsigned long long)tid; sel[1] = remaining - before; }
            }
            __syncthreads();
            prefix |= (unsigned)sel[0] << shift;
            mask |= 0xffu << shift;
            remaining = sel[1];
        }
        // keys above the cut go; the new maximum and the sums of what stays (relative to the old maximum)
        double s = 0.0, e = 0.0;
        float nm = -INFINITY;
        sweep([&](int j, float v) {
            if (typical_key(v, mx, logS, H) > prefix) { drop(j); return; }
            const float d = v - mx, ex = expf(d);
            s += (double)ex;
            e += (double)ex * (double)d;
            nm = fmaxf(nm, v);
        });
        warp_block_sum2(s, e, red_d);
        S = s; E = e;
        nm = warp_block_max(nm, red_f);
        if (nm != mx && nm > -INFINITY) { mx = nm; sums(); }              // the top entry was not typical: statistics relative to the new one
    }
    if (eps > 0.f && eps < 1.f) {
        if (!have_sums) sums();
        threshold_stage(log((double)eps) + log(S));
    }
    if (eta_eps > 0.f && eta_eps < 1.f) {
        if (!have_sums) sums();
        const double logS = log(S), H = logS - E / S;
        const double eta = fmin((double)eta_eps, sqrt((double)eta_eps) * exp(-H));
        threshold_stage(log(eta) + logS);
    }

    float best = -INFINITY;
    int bidx = 0x7fffffff;
    sweep([&](int j, float v) {
        const int i = column(j);
        const float sc = (v - mx) + gumbel_noise(seed, st, key_row, (unsigned)(i >= vocab ? i - col0 : i));
        if (sc > best || (sc == best && i < bidx)) { best = sc; bidx = i; }
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o);
        const int oi = __shfl_xor(bidx, o);
        if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
    }
    __syncthreads();
    if (lane == 0) { red_f[wave] = best; red_i[wave] = bidx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (red_f[w] > best || (red_f[w] == best && red_i[w] < bidx)) { best = red_f[w]; bidx = red_i[w]; }
        out_val[b] = best;
        out_idx[b] = bidx;
    }
}

// HF's MinP → Typical → Epsilon → Eta warpers and the multinomial draw over fp32 score rows that already hold the scores after temperature /
// top-k / top-p (padt_sample_token with gen_cfg's write_back): rows[b][0..n_cols) is warped in place (dropped columns become -inf, kept ones
// keep their bits) and one (value, index) partial per row is written in the layout padt_greedy_step reads with nblk = 1.  The four values are
// the GenCfg slots after `pad`, read from device memory.  row_base (nullable, with vrt_off [batch + 1] and vocab): row_base[b] = the first
// row of b's own batch inside a merged decode group — the draw is then keyed by (b - row_base[b], column in the batch's own numbering: a
// column >= vocab minus vrt_off[row_base[b]]), so a batch draws inside a group what it draws alone; null: (b, column).
extern "C" int padt_warp_sample_rows_f32(void* stream, void* rows_f32, long ld, long n_cols, const void* gen_cfg, const int* step,
                                         void* part_val, void* part_idx, long batch, long vocab, const int* vrt_off, const int* row_base) {
    if (batch <= 0) return 0;
    if (row_base != nullptr && (vrt_off == nullptr || vocab < 0 || vocab > n_cols)) {
        padt_set_error("padt_warp_sample_rows_f32: row_base needs vrt_off and 0 <= vocab <= n_cols");
        return -1;
    }
    if (rows_f32 == nullptr || gen_cfg == nullptr || n_cols <= 0 || n_cols > 0x7fffffffL || ld < n_cols || part_val == nullptr || part_idx == nullptr) {
        padt_set_error("padt_warp_sample_rows_f32: score rows (ld >= n_cols), gen_cfg and the partial buffers are required");
        return -1;
    }
    hipLaunchKernelGGL(warp_sample_rows_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, (float*)rows_f32, ld, (int)n_cols,
                       (const GenCfg*)gen_cfg, step, (float*)part_val, (int*)part_idx, (int)vocab, vrt_off, row_base);
    PADT_CHECK_LAUNCH();
    return 0;
}

// Arg-max of fp32 score rows (round 6: the selection of the HOOKED decode loop — caller-supplied `logits_processor`s of padt.py:717 have rewritten
// the step's score rows between the head kernel and the selection, so the head's fused arg-max partials no longer describe them): one block per
// row, ties → lowest index (torch.argmax, padt.py:745), one (value, index) partial per row in the layout padt_greedy_step reads with nblk = 1.
// The tree's comparator is argmax_less with torch's NaN rule: a NaN beats every number, two NaNs → the lower index.
PADT_DEV bool argmax_less_nan(float cv, int ci, float ov, int oi) {
    const bool o_nan = ov != ov, c_nan = cv != cv;
    return (o_nan && !c_nan) || (o_nan == c_nan && (ov > cv || ((ov == cv || o_nan) && oi < ci)));
}
__global__ __launch_bounds__(1024) void argmax_rows_f32_kernel(const float* __restrict__ x, long ld, int n, float* __restrict__ out_val, int* __restrict__ out_idx) {
    __shared__ float red_v[1024];
    __shared__ int red_i[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (long)b * ld;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = tid; i < n; i += 1024) {
        const float v = row[i];
        if (v > best || (v == best && i < bidx) || (v != v && best == best)) { best = v; bidx = i; }    // a NaN wins once (torch.argmax: NaN is the maximum)
    }
    block_argmax_lds<1024, argmax_less_nan>(best, bidx, red_v, red_i);
    if (tid == 0) { out_val[b] = red_v[0]; out_idx[b] = red_i[0] == 0x7fffffff ? 0 : red_i[0]; }
}

extern "C" int padt_argmax_rows_f32(void* stream, const void* scores_f32, long ld, long n_cols, void* part_val, void* part_idx, long batch) {
    if (batch <= 0) return 0;
    if (scores_f32 == nullptr || n_cols <= 0 || n_cols > 0x7fffffffL || part_val == nullptr || part_idx == nullptr) {
        padt_set_error("padt_argmax_rows_f32: score rows, a column count and the partial buffers are required");
        return -1;
    }
    hipLaunchKernelGGL(argmax_rows_f32_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, (const float*)scores_f32, ld, (int)n_cols,
                       (float*)part_val, (int*)part_idx);
    PADT_CHECK_LAUNCH();
    return 0;
}

// Token log-probs of the ROW path (generate(output_token_logprobs=True) under do_sample or with caller logits processors: the selection does
// not come from the head's partials): one block per fp32 score row as the selection kernel left it (under sampling the warped row:
// gen_cfg's write_back), between padt_sample_token / padt_argmax_rows_f32 and padt_greedy_step, which clears `unfinished`:
// logprobs[b][*step] = unfinished[b] ? row[tok] - max - log Σ exp(row - max) : 0 with tok = part_idx[b]; -inf when the row has no candidate
// or tok is not one.  Fixed order: strided columns per thread, LDS trees.
__global__ __launch_bounds__(1024) void token_logprob_rows_f32_kernel(const float* __restrict__ x, long ld, int n, const int* __restrict__ part_idx,
                                                                     const int* __restrict__ unfinished, const int* __restrict__ step,
                                                                     float* __restrict__ logprobs, int t_max) {
    __shared__ float red[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* row = x + (long)b * ld;
    float mx = -INFINITY;
    for (int i = tid; i < n; i += 1024) { const float v = row[i]; mx = (v > mx || v != v) ? v : mx; }     // a NaN stays: the result is NaN then
    const float M = block_tree_lds<1024>(mx, red, [](float c, float o) { return (o > c || o != o) ? o : c; });
    __syncthreads();
    float acc = 0.f;
    for (int i = tid; i < n; i += 1024) {
        const float v = row[i];
        acc += v == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((v - M) * 1.44269504088896341f);
    }
    block_sum_lds<1024>(acc, red);
    if (tid == 0) {
        const int t = *step;
        if (t >= 0 && t < t_max) {
            const int tok = part_idx[b];
            float lp = 0.f;
            if (unfinished[b]) {
                const float v = (tok >= 0 && tok < n) ? row[tok] : -INFINITY;
                lp = (v == -INFINITY || M == -INFINITY) ? -INFINITY : (v - M) - logf(red[0]);
            }
            logprobs[(long)b * t_max + t] = lp;
        }
    }
}

extern "C" int padt_token_logprob_rows_f32(void* stream, const void* rows_f32, long ld, long n_cols, const void* part_idx, const int* unfinished,
                                           const int* step, void* logprobs, long t_max, long batch) {
    if (batch <= 0) return 0;
    if (rows_f32 == nullptr || n_cols <= 0 || n_cols > 0x7fffffffL || ld < n_cols || part_idx == nullptr || unfinished == nullptr || step == nullptr ||
        logprobs == nullptr || t_max <= 0 || t_max > 0x7fffffffL) {
        padt_set_error("padt_token_logprob_rows_f32: score rows (ld >= n_cols), the selection, the unfinished flags, the step counter and logprobs [batch][t_max] are required");
        return -1;
    }
    hipLaunchKernelGGL(token_logprob_rows_f32_kernel, dim3((unsigned)batch), dim3(1024), 0, (hipStream_t)stream, (const float*)rows_f32, ld, (int)n_cols,
                       (const int*)part_idx, unfinished, step, (float*)logprobs, (int)t_max);
    PADT_CHECK_LAUNCH();
    return 0;
}

}  // namespace PADT_NS
