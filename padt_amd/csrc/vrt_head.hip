// VRT logit head with fused logit mask + arg-max, and the greedy-loop bookkeeping kernel.
//
// Reference (padt.py:292-301, 713-757): logits = hidden @ cat([embed_tokens|lm_head, prototypes]).T, masked_fill(-inf)
// outside [text vocab ∪ the sample's own patch rows], argmax of the last position in fp32, finished rows get pad,
// EOS clears `unfinished`.  Here the two tables are read through two base pointers (the 0.6 GB concatenation per forward
// never happens), only the last position is computed, and the logits never touch HBM unless a caller asks for them.
//
// vrt_head_kernel: block = 4 waves = 16 table rows, K interleaved over the waves (same weight-streaming scheme as the
// skinny GEMM), swapped MFMA so a lane owns 4 consecutive table rows of one sample; block-local (max, argmax) per
// sample goes to a partial buffer.  greedy_step_kernel: final reduction (ties → lowest index, as torch.argmax),
// pad/EOS bookkeeping, append to the token buffer, stash the step's last-layer hidden row for parseVRTintoCompletion
// (padt_processor.py:125), advance cache slots / rope positions / step counter — all on device, so a decode step is one
// replayable hipGraph.
#include "common.h"
#include <stdlib.h>
#include <cstdint>

extern "C" void padt_set_error(const char* msg);
extern "C" long padt_vrt_head_nblk(long vocab, long n_proto);

namespace PADT_NS {

// Generation-config slots kept in DEVICE memory so a captured decode graph does not bake them in
// (HF generation_config.json: repetition_penalty, eos_token_id list; padt.py:570-580,717,756).
struct GenCfg {
    float penalty;                     // RepetitionPenaltyLogitsProcessor: score<0 ? score*p : score/p on every id already in the row
    int eos[4];                        // up to 4 EOS ids, -1 = unused
    int do_sample;                     // 0 greedy (arg-max), 1 multinomial sampling (padt.py:740-743) by sample_token_kernel
    unsigned seed;                     // counter-based RNG key (the device step counter, row and table index are the counter)
    float temperature;                 // TemperatureLogitsWarper
    int top_k;                         // TopKLogitsWarper (0 = off)
    float top_p;                       // TopPLogitsWarper (1 = off)
    int write_back;                    // sample_token_kernel overwrites its input rows with the warped scores (l / T, -inf outside the kept set)
    int pad;
    // read by warp_sample_rows_kernel alone (every other kernel stops at `pad`): HF's warpers after top-p, each with its "off" value
    float min_p;                       // MinPLogitsWarper: active when 0 < min_p <= 1 (0 = off)
    float typical_p;                   // TypicalLogitsWarper: active when 0 < typical_p < 1 (1 = off)
    float epsilon_cutoff;              // EpsilonLogitsWarper: active when 0 < epsilon < 1 (0 = off)
    float eta_cutoff;                  // EtaLogitsWarper: active when 0 < epsilon < 1 (0 = off)
};

struct HeadArgs {
    const x16_t* h; long ldh;         // [B][D]
    const x16_t* E; int V;            // text rows
    const x16_t* proto; int NP;       // prototype rows
    const int* vrt_off;                // [B+1]
    const int* mode_table;             // [T] or null: 0 free, 1 text rows only, 2 own VRT rows only, 3 force EOS
    const int* step;                   // device step counter (index into mode_table) or null
    float* logits; long ldl;           // optional [B][V+NP]
    float* part_val; int* part_idx;    // [nblk][16*MT]
    int B, D, eos;
    const x16_t* Ep;                  // optional fragment-packed copy of E (PACKED kernels; h is then packed too)
    const GenCfg* gen;                 // optional generation config (repetition penalty) + per-sample seen-token bitmap
    const unsigned* seen; long seen_words;
    const unsigned* ban; long ban_words;   // optional per-sample bitmap of banned table rows (gen_rules_kernel): bit set → the logit is -inf
    float* part_sum;                   // LSE kernels: [nblk][B] Σ exp(v - block max) over the block's 16 masked logits (token log-probs)
    const int* forced; int t_forced;   // PROBE kernels: [B][t_forced] table columns the caller forces (generate(forced_tokens=)), < 0 = free step
    float* probe_val;                  // PROBE kernels: [B] the processed logit at forced[m][*step]
};

// PACKED: text rows come from a fragment-packed copy of the table ([V/16][D/32][64 lanes][8], ops.pack_weight — every wave
// load is 1 KiB contiguous) and the hidden rows from the 16-row fragment-packed activation layout; prototype rows (rebuilt
// per batch) stay row-major.  Waves take groups of U consecutive K-steps; wave w finishes (row block, sample block) pairs w, w + 4, ...
// NT: 16-row table blocks per thread block — they share every hidden-row fragment a wave loads (at 64 rows a wave loads 4 KiB of hidden
// fragments per K-step: with one table block per thread block that is 4 bytes of L2 traffic per byte of table, 2.5 GB per step; with NT = 4,
// 1:1).  The K-step → wave map and the cross-wave order are those of NT = 1: a logit's bits depend neither on NT nor on the row count.
// LSE (generate(output_token_logprobs=True)): the finishing wave also writes s = Σ exp(v - best) over the block's 16 masked / penalised /
// ban-filtered logits of a sample — greedy_step_kernel<true> folds the (best, s) pairs into log p(token) without any logit row in memory.
// exp is v_exp_f32 on (v - best)·log2e: the argument is <= 0, so nothing overflows however large the logits are; a block without an allowed
// row (best = -inf) yields s = 0.  MFMA order, cross-wave sum and the (best, idx) partials are those of LSE = false, bit for bit.
// PROBE (padt_vrt_head_probe, an LSE kernel plus one store): the lane that owns column forced[m][*step] of sample m also writes the value v it
// writes to `logits` — masked, penalised, ban-filtered — to probe_val[m]; a negative entry, or a step outside [0, t_forced), writes nothing.
template <int MT, int NT, bool PACKED, bool LSE = false, bool PROBE = false>
__global__ __launch_bounds__(256) void vrt_head_kernel(HeadArgs p) {
    extern __shared__ __attribute__((aligned(16))) float red_raw[];
    typedef float RedT[NT * MT][64][4];
    RedT* red = reinterpret_cast<RedT*>(red_raw);                 // [4 waves]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int NTOT = p.V + p.NP;
    const int nblk = (NTOT + 15) / 16;
    const x16_t* wrow[NT];
    const x16_t* wpk[NT];
    bool in_text[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int n0 = (blockIdx.x * NT + i) * 16;
        int n = n0 + frow;
        n = n < NTOT ? n : NTOT - 1;
        in_text[i] = PACKED && (n0 + 16 <= p.V);                  // whole block inside the packed text table
        wrow[i] = (n < p.V) ? p.E + (long)n * p.D : p.proto + (long)(n - p.V) * p.D;
        wpk[i] = PACKED ? p.Ep + (long)(min(n0, p.V - 16) >> 4) * (p.D >> 5) * 512 + lane * 8 : nullptr;
    }
    const x16_t* xrow[MT];
    bool xok[MT];
#pragma unroll
    for (int j = 0; j < MT; ++j) {
        const int m = j * 16 + frow;
        xok[j] = PACKED ? (j * 16 < p.B) : (m < p.B);             // packed: row blocks past the last valid row are not in the buffer
        xrow[j] = PACKED ? p.h + (long)j * 16 * p.ldh + lane * 8 : p.h + (long)(m < p.B ? m : 0) * p.ldh + fq * 8;
    }
    const int xstep = PACKED ? 512 : 32;
    f32x4 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nks = (p.D + 31) / 32;
    constexpr int U = 4;                                          // K-steps per wave group (fixes the summation order)
    constexpr int UH = (NT * MT > 8) ? 2 : 4;                     // K-steps loaded at a time (register budget); same MFMA order either way
    for (int g0 = wave; g0 * U < nks; g0 += 4) {
#pragma unroll
        for (int uh = 0; uh < U; uh += UH) {
            x16x8 wf[UH][NT], xf[UH][MT];
#pragma unroll
            for (int u = 0; u < UH; ++u) {
                const int ks = g0 * U + uh + u;
                const int k = ks * 32 + fq * 8;
                const bool kok = (ks < nks) && (k < p.D);
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    if (PACKED && in_text[i]) wf[u][i] = kok ? __builtin_nontemporal_load(reinterpret_cast<const x16x8*>(wpk[i] + (long)ks * 512)) : zero_frag();
                    else wf[u][i] = kok ? ld_frag(wrow[i] + k) : zero_frag();
                }
#pragma unroll
                for (int j = 0; j < MT; ++j) xf[u][j] = (kok && xok[j]) ? ld_frag(xrow[j] + (long)ks * xstep) : zero_frag();
            }
#pragma unroll
            for (int u = 0; u < UH; ++u)
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j) acc[i][j] = mfma16(wf[u][i], xf[u][j], acc[i][j]);
        }
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) *reinterpret_cast<f32x4*>(&red[wave][i * MT + j][lane][0]) = acc[i][j];
    __syncthreads();
    const int mode = (p.mode_table && p.step) ? p.mode_table[*p.step] : 0;
    const float pen = (p.gen && p.seen) ? p.gen->penalty : 1.0f;
    for (int q = wave; q < NT * MT; q += 4) {                     // (table block, sample block) pairs this wave finishes
        const int i = q / MT, j = q % MT;
        const int blk = blockIdx.x * NT + i;
        if (blk >= nblk) continue;
        const int n0 = blk * 16;
        f32x4 sum = *reinterpret_cast<f32x4*>(&red[0][q][lane][0]);
#pragma unroll
        for (int w = 1; w < 4; ++w) sum += *reinterpret_cast<f32x4*>(&red[w][q][lane][0]);
        const int m = j * 16 + frow;                              // sample
        float best = -INFINITY;
        int bidx = 0x7fffffff;
        int lo = 0, hi = 0;
        if (m < p.B) { lo = p.vrt_off[m]; hi = p.vrt_off[m + 1]; }
        int fcol = -1;                                            // PROBE: the column forced on sample m at this step
        if constexpr (PROBE) {
            const int st = *p.step;
            if (m < p.B && st >= 0 && st < p.t_forced) fcol = p.forced[(long)m * p.t_forced + st];
        }
        float vr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = n0 + fq * 4 + r;
            bool ok = (m < p.B) && (row < NTOT);
            if (ok) {
                if (row < p.V) ok = (mode == 0 || mode == 1 || (mode == 3 && row == p.eos));
                else { const int jv = row - p.V; ok = (jv >= lo && jv < hi) && (mode == 0 || mode == 2); }
            }
            if (p.ban && ok) ok = !((p.ban[(long)m * p.ban_words + (row >> 5)] >> (row & 31)) & 1u);   // a pure ban: the penalty no longer matters
            float sc = sum[r];
            if (pen != 1.0f && ok && ((p.seen[(long)m * p.seen_words + (row >> 5)] >> (row & 31)) & 1u)) sc = sc < 0.f ? sc * pen : sc / pen;
            const float v = ok ? sc : -INFINITY;
            if (p.logits && m < p.B && row < NTOT) p.logits[(long)m * p.ldl + row] = v;
            if constexpr (PROBE) {
                if (row == fcol && row < NTOT) p.probe_val[m] = v;   // fcol >= 0 only for m < B; one lane owns the column
            }
            if (v > best) { best = v; bidx = row; }               // rows ascend with r → first max wins
            vr[r] = v;
        }
        // combine the 4 lanes (fq = 0..3) that hold the same sample
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float ov = __shfl_xor(best, off, 64);
            const int oi = __shfl_xor(bidx, off, 64);
            if (ov > best || (ov == best && oi < bidx)) { best = ov; bidx = oi; }
        }
        if (fq == 0 && m < p.B) {
            p.part_val[(long)blk * p.B + m] = best;
            p.part_idx[(long)blk * p.B + m] = bidx;
        }
        if constexpr (LSE) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r)                           // a masked logit adds an exact 0 (and -inf - -inf never reaches the exp)
                s += vr[r] == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((vr[r] - best) * 1.44269504088896341f);
            s += __shfl_xor(s, 16, 64);                           // the same two steps that combined `best`: a fixed order
            s += __shfl_xor(s, 32, 64);
            if (fq == 0 && m < p.B) p.part_sum[(long)blk * p.B + m] = s;
        }
    }
}

#if !PADT_OP16_F16   // type-independent: compiled once
struct GreedyArgs {
    const float* part_val; const int* part_idx; int nblk;
    int B, D, eos, pad, T_max;
    int* unfinished;          // [B]
    long* tokens_out;         // [B][T_max]
    long* cur_tok;            // [B] token to feed to the next step
    int* step;                // device counter
    int* slot; int* lens;     // [B] KV append index / valid-key count for the NEXT step
    int* pos3;                // [3][B] rope positions for the NEXT step
    const x16_t* hidden;     // [B][D] last-layer hidden of this step (post final norm)
    x16_t* hidden_buf;       // [T_max][B][D]
    int advance;              // 1: bump slot/lens/pos (decode steps and after prefill)
    const GenCfg* gen;        // optional: extra EOS ids
    unsigned* seen; long seen_words;   // optional: bitmap of ids present in each row (repetition penalty), updated here
    const float* part_sum;    // LP: [nblk][B] Σ exp(v - block max) of the LSE head kernels
    float* logprobs;          // LP: [B][T_max] log-prob of the token each step selected
    const int* forced; int t_forced;   // FORCED: [B][t_forced] the caller's tokens (table columns; < 0 = free step), read at *step
    const float* probe;       // FORCED + LP: [B] the processed logit of the forced column (padt_vrt_head_probe)
    int n_cols;               // FORCED: table columns; an entry outside [0, n_cols) is a free step
};

// LP (padt_greedy_step_lp): next to the arg-max, S = Σ_blk part_sum · exp(part_val - M) with M the global max — the row's Σ exp(logit - M) —
// in a fixed order (the arg-max's strided block → thread map and LDS tree; an all-masked block adds an exact 0).  The selection IS the arg-max,
// so log p(token) = -log S.  Rows finished on entry hold 0 (a completion's log-prob is then the row sum), a row without any candidate -inf.
// FORCED (padt_forced_step): an unfinished row whose entry forced[b][*step] is a table column takes it as its token whatever the scores say, a
// -inf column included (the "no candidate → pad" branch is for free rows); with LP its log-prob is (probe - M) - log S, -inf for a -inf column —
// when the forced column is the arg-max, probe == M, the difference is an exact 0 and the bits are those of the free step.
template <bool LP, bool FORCED = false>
__global__ __launch_bounds__(256) void greedy_step_kernel(GreedyArgs p) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float ss[LP ? 256 : 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = tid; i < p.nblk; i += 256) {
        const float v = p.part_val[(long)i * p.B + b];
        const int ix = p.part_idx[(long)i * p.B + b];
        if (v > best || (v == best && ix < bidx)) { best = v; bidx = ix; }
    }
    sv[tid] = best; si[tid] = bidx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            const float ov = sv[tid + s]; const int oi = si[tid + s];
            if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
        }
        __syncthreads();
    }
    if constexpr (LP) {
        const float M = sv[0];
        float acc = 0.f;
        for (int i = tid; i < p.nblk; i += 256) {
            const float s = p.part_sum[(long)i * p.B + b];
            const float v = p.part_val[(long)i * p.B + b];
            acc += (s == 0.f || v == -INFINITY) ? 0.f : s * __builtin_amdgcn_exp2f((v - M) * 1.44269504088896341f);
        }
        ss[tid] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) ss[tid] += ss[tid + s];
            __syncthreads();
        }
    }
    const int step = *p.step;
    if (step < p.T_max) {
        const x16_t* h = p.hidden + (long)b * p.D;
        x16_t* hb = p.hidden_buf + ((long)step * p.B + b) * p.D;
        for (int c = tid * 8; c < p.D; c += 256 * 8) *reinterpret_cast<u32x4*>(hb + c) = *reinterpret_cast<const u32x4*>(h + c);
    }
    __syncthreads();
    if (tid == 0) {
        const int unf = p.unfinished[b];
        long next = unf ? (long)si[0] : (long)p.pad;                 // padt.py:749
        // a row whose logits are all NaN (an fp16 operand overflowed upstream: the range guard flags the batch, padt_check_finite) has no
        // arg-max — bidx is still the sentinel; continue with the pad token so that every later index stays inside its table
        const bool no_choice = si[0] == 0x7fffffff || next < 0 || (p.seen && (next >> 5) >= p.seen_words);
        if (no_choice) next = (long)p.pad;
        bool is_forced = false;
        if constexpr (FORCED) {
            if (unf && step >= 0 && step < p.t_forced) {
                const int f = p.forced[(long)b * p.t_forced + step];
                if (f >= 0 && f < p.n_cols) { is_forced = true; next = (long)f; }
            }
        }
        if (step < p.T_max) p.tokens_out[(long)b * p.T_max + step] = next;
        if constexpr (LP) {
            float lp = !unf ? 0.f : no_choice ? -INFINITY : 0.f - logf(ss[0]);
            if constexpr (FORCED) {
                if (is_forced) { const float pr = p.probe[b]; lp = pr == -INFINITY ? -INFINITY : (pr - sv[0]) - logf(ss[0]); }
            }
            if (step >= 0 && step < p.T_max) p.logprobs[(long)b * p.T_max + step] = lp;
        }
        p.cur_tok[b] = next;
        bool is_eos = next == p.eos;
        if (p.gen) {
#pragma unroll
            for (int k = 0; k < 4; ++k) is_eos = is_eos || (p.gen->eos[k] >= 0 && next == (long)p.gen->eos[k]);
        }
        p.unfinished[b] = unf & (is_eos ? 0 : 1);                    // padt.py:756
        if (p.seen) p.seen[(long)b * p.seen_words + (next >> 5)] |= 1u << (next & 31);   // the row now contains `next`
        if (p.advance) {
            p.slot[b] += 1; p.lens[b] += 1;
            p.pos3[b] += 1; p.pos3[p.B + b] += 1; p.pos3[2 * p.B + b] += 1;
        }
    }
}

// one-thread kernel: bump the step counter after all samples' greedy_step blocks ran
__global__ void step_inc_kernel(int* step) { *step += 1; }

extern "C" long padt_vrt_head_nblk(long vocab, long n_proto) { return (vocab + n_proto + 15) / 16; }

// ---------------------------------------------------------------------------------------------------------------------
// HF's pure-ban logits processors (generation/logits_process.py: SuppressTokens, SuppressTokensAtBegin, NoBadWords = SequenceBias with
// -inf, NoRepeatNGram) as ONE per-step bitmap the head tests next to the logit mask.  One block per session row rebuilds the row of `ban`
// from scratch — zero, barrier, OR in — so no bit outlives the step it applies to.  The row's history is what HF's processors see as
// input_ids: h[i] = i < L ? hist[row][i] (the caller's padded prompt row, padding included) : tokens[row][i - L], cur = L + *step ids.
// Rule table (DEVICE memory like GenCfg, nothing baked into a captured graph; packed by ops.gen_rules_tensor, at most GEN_RULES_MAX ints):
//   [0] n-gram size n (0 = off)  [1] n_static  [2] n_begin  [3] n_words  [4 ..) static ids | begin ids | word offsets | words (m, id[m])
//   static ids (suppress_tokens and 1-token bad words): always;  begin ids: only at *step == 0;
//   word of m > 1 ids: its last id when cur >= m and the last m - 1 history ids equal its first m - 1 (SequenceBiasLogitsProcessor skips a
//   sequence LONGER than the input: cur >= m, not m - 1);
//   n-gram: when cur + 1 >= n, for every i in [0, cur - n] with h[i .. i + n - 2] == the last n - 1 history ids: h[i + n - 1] (n = 1: every id
//   of the history).  Finished rows are treated like live ones, as in HF.
constexpr int GEN_RULES_MAX = 4096;
struct RulesArgs {
    const int* rules; const int* hist; long ld_hist; const int* hist_len; const long* tokens; long ld_tok; const int* step;
    unsigned* ban; long ban_words; int n_cols;
};

__global__ __launch_bounds__(256) void gen_rules_kernel(RulesArgs p) {
    const int row = blockIdx.x, tid = threadIdx.x;
    unsigned* out = p.ban + (long)row * p.ban_words;
    for (long w = tid; w < p.ban_words; w += 256) out[w] = 0u;
    __syncthreads();
    const int* r = p.rules;
    int t = *p.step;
    t = t < 0 ? 0 : (t > (int)p.ld_tok ? (int)p.ld_tok : t);
    int L = p.hist_len[row];
    L = L < 0 ? 0 : (L > (int)p.ld_hist ? (int)p.ld_hist : L);
    const int cur = L + t;
    const int* hrow = p.hist + (long)row * p.ld_hist;
    const long* trow = p.tokens + (long)row * p.ld_tok;
    auto h = [&](int i) -> int { return i < L ? hrow[i] : (int)trow[i - L]; };
    auto set = [&](int id) { if (id >= 0 && id < p.n_cols) atomicOr(&out[id >> 5], 1u << (id & 31)); };
    const int n = r[0], ns = r[1], nb = r[2], nw = r[3];
    if (n < 0 || ns < 0 || nb < 0 || nw < 0 || 4L + ns + nb + nw > GEN_RULES_MAX) return;      // not a table ops.gen_rules_tensor packed
    for (int i = tid; i < ns; i += 256) set(r[4 + i]);
    if (t == 0)
        for (int i = tid; i < nb; i += 256) set(r[4 + ns + i]);
    for (int w = tid; w < nw; w += 256) {
        const int o = r[4 + ns + nb + w];
        if (o < 0 || o >= GEN_RULES_MAX) continue;
        const int m = r[o];
        if (m < 2 || o + m >= GEN_RULES_MAX || cur < m) continue;
        bool eq = true;
        for (int k = 0; k < m - 1 && eq; ++k) eq = h(cur - (m - 1) + k) == r[o + 1 + k];
        if (eq) set(r[o + m]);
    }
    if (n > 0 && cur + 1 >= n)
        for (int i = tid; i <= cur - n; i += 256) {
            bool eq = true;
            for (int k = 0; k < n - 1 && eq; ++k) eq = h(i + k) == h(cur - (n - 1) + k);
            if (eq) set(h(i + n - 1));
        }
}

extern "C" int padt_gen_rules(void* stream, const int* rules, const int* hist, long ld_hist, const int* hist_len, const long* tokens,
                              long ld_tokens, const int* step, void* ban, long ban_words, long n_cols, long batch) {
    if (batch <= 0) return 0;
    if (!rules || !hist || !hist_len || !tokens || !step || !ban || ld_hist <= 0 || ld_tokens <= 0 || ld_hist + ld_tokens > 0x7fffffffL) {
        padt_set_error("padt_gen_rules: rule table, history, token buffer, step counter and ban bitmap are required"); return -1;
    }
    if (n_cols <= 0 || n_cols > ban_words * 32) { padt_set_error("padt_gen_rules: ban bitmap narrower than the table"); return -1; }
    RulesArgs a{rules, hist, ld_hist, hist_len, tokens, ld_tokens, step, (unsigned*)ban, ban_words, (int)n_cols};
    hipLaunchKernelGGL(gen_rules_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}
#endif

template <int MT, int NT, bool PACKED, bool LSE, bool PROBE>
static void launch_head(const HeadArgs& a, int nblk, hipStream_t s) {
    constexpr int lds = 4 * NT * MT * 64 * 16;
    if constexpr (lds > 64 * 1024) {
        static PerDeviceOnce once;
        once.run([] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vrt_head_kernel<MT, NT, PACKED, LSE, PROBE>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    }
    hipLaunchKernelGGL((vrt_head_kernel<MT, NT, PACKED, LSE, PROBE>), dim3((nblk + NT - 1) / NT), dim3(256), lds, s, a);
}

template <bool LSE, bool PROBE = false>
static void dispatch_head(const HeadArgs& a, int nblk, hipStream_t s) {
    if (a.Ep) {                                                 // NT = 4 table blocks per thread block (2 at 128 rows): profiles/r03_head_nt_ab.log
        if (a.B <= 16) launch_head<1, 4, true, LSE, PROBE>(a, nblk, s);
        else if (a.B <= 32) launch_head<2, 4, true, LSE, PROBE>(a, nblk, s);
        else if (a.B <= 64) launch_head<4, 4, true, LSE, PROBE>(a, nblk, s);
        else launch_head<8, 2, true, LSE, PROBE>(a, nblk, s);
    } else if (a.B <= 16) launch_head<1, 1, false, LSE, PROBE>(a, nblk, s);
    else if (a.B <= 32) launch_head<2, 1, false, LSE, PROBE>(a, nblk, s);
    else if (a.B <= 64) launch_head<4, 1, false, LSE, PROBE>(a, nblk, s);
    else launch_head<8, 1, false, LSE, PROBE>(a, nblk, s);
}

static int vrt_head_impl(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                         const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                         const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                         long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                         const void* seen, long seen_words, const void* ban, long ban_words, void* part_sum = nullptr,
                         const int* forced = nullptr, long t_forced = 0, void* probe_val = nullptr) {
    if (batch <= 0) return 0;
    if (batch > 128 || (D & 7) || (ldh & 7)) { padt_set_error("padt_vrt_head: batch <= 128, D % 8 == 0 required"); return -1; }
    if (embed_table_packed && ((D & 31) || (vocab & 15) || ((uintptr_t)embed_table_packed & 15) || ((uintptr_t)hidden & 15))) {
        padt_set_error("padt_vrt_head: the packed path needs D % 32 == 0, vocab % 16 == 0 and 16-byte aligned pointers");
        return -1;
    }
    HeadArgs a{(const x16_t*)hidden, ldh, (const x16_t*)embed_table, (int)vocab, (const x16_t*)proto, (int)n_proto,
               vrt_off, mode_table, step, (float*)logits_f32, ld_logits, (float*)part_val, (int*)part_idx, (int)batch,
               (int)D, eos, (const x16_t*)embed_table_packed, (const GenCfg*)gen_cfg, (const unsigned*)seen, seen_words,
               (const unsigned*)ban, ban_words, (float*)part_sum, forced, (int)t_forced, (float*)probe_val};
    if (seen && seen_words * 32 < vocab + n_proto) { padt_set_error("padt_vrt_head: seen bitmap narrower than the table"); return -1; }
    if (ban && ban_words * 32 < vocab + n_proto) { padt_set_error("padt_vrt_head_ban: ban bitmap narrower than the table"); return -1; }
    const int nblk = (int)padt_vrt_head_nblk(vocab, n_proto);
    hipStream_t s = (hipStream_t)stream;
    if (forced) dispatch_head<true, true>(a, nblk, s);
    else if (part_sum) dispatch_head<true>(a, nblk, s);
    else dispatch_head<false>(a, nblk, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

extern "C" int PADT_TWIN(padt_vrt_head)(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                             const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                             const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                             long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                             const void* seen, long seen_words) {
    return vrt_head_impl(stream, hidden, ldh, embed_table, vocab, proto, n_proto, vrt_off, mode_table, step, logits_f32, ld_logits, part_val,
                         part_idx, batch, D, eos, embed_table_packed, gen_cfg, seen, seen_words, nullptr, 0);
}

// padt_vrt_head with a ban bitmap [batch][ban_words] (padt_gen_rules): a set bit makes the written logit and the partial -inf, like a row
// outside the logit mask.  A row whose every column is banned has no arg-max: padt_greedy_step's sentinel branch then emits pad.
extern "C" int PADT_TWIN(padt_vrt_head_ban)(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                             const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                             const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                             long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                             const void* seen, long seen_words, const void* ban, long ban_words) {
    return vrt_head_impl(stream, hidden, ldh, embed_table, vocab, proto, n_proto, vrt_off, mode_table, step, logits_f32, ld_logits, part_val,
                         part_idx, batch, D, eos, embed_table_packed, gen_cfg, seen, seen_words, ban, ban_words);
}

// padt_vrt_head_ban that also writes part_sum[blk * batch + b] = Σ exp(v - part_val) over block blk's 16 masked logits of sample b (the LSE
// kernels): with padt_greedy_step_lp, the log-prob of every selected token without a logit row in memory.  Tokens, partials and any written
// logits are those of padt_vrt_head_ban, bit for bit.
extern "C" int PADT_TWIN(padt_vrt_head_lse)(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                             const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                             const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                             long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                             const void* seen, long seen_words, const void* ban, long ban_words, void* part_sum) {
    if (batch > 0 && part_sum == nullptr) { padt_set_error("padt_vrt_head_lse: part_sum is required"); return -1; }
    return vrt_head_impl(stream, hidden, ldh, embed_table, vocab, proto, n_proto, vrt_off, mode_table, step, logits_f32, ld_logits, part_val,
                         part_idx, batch, D, eos, embed_table_packed, gen_cfg, seen, seen_words, ban, ban_words, part_sum);
}

// padt_vrt_head_lse that also writes probe_val[b] = the processed logit (what `logits` gets: masked, penalised, ban-filtered) of column
// forced[b][*step] of the int32 table forced [batch][t_forced] — generate(forced_tokens=): with padt_forced_step, the log-prob of a token the
// caller chose.  A negative entry, or *step outside [0, t_forced), writes nothing; entries must be < vocab + n_proto.  Partials, part_sum and any
// written logits are those of padt_vrt_head_lse, bit for bit.
extern "C" int PADT_TWIN(padt_vrt_head_probe)(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                             const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                             const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                             long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                             const void* seen, long seen_words, const void* ban, long ban_words, void* part_sum,
                             const int* forced, long t_forced, void* probe_val) {
    if (batch <= 0) return 0;
    if (part_sum == nullptr || forced == nullptr || probe_val == nullptr || step == nullptr || t_forced <= 0 || t_forced > 0x7fffffffL) {
        padt_set_error("padt_vrt_head_probe: part_sum, the step counter, the forced table [batch][t_forced] and probe_val are required"); return -1;
    }
    return vrt_head_impl(stream, hidden, ldh, embed_table, vocab, proto, n_proto, vrt_off, mode_table, step, logits_f32, ld_logits, part_val,
                         part_idx, batch, D, eos, embed_table_packed, gen_cfg, seen, seen_words, ban, ban_words, part_sum, forced, t_forced,
                         probe_val);
}

#if !PADT_OP16_F16   // type-independent: compiled once
extern "C" int padt_greedy_step(void* stream, const void* part_val, const void* part_idx, long nblk, long batch, long D,
                                int eos, int pad, long t_max, int* unfinished, long* tokens_out, long* cur_tok,
                                int* step, int* slot, int* lens, int* pos3, const void* hidden, void* hidden_buf,
                                int advance, const void* gen_cfg, void* seen, long seen_words) {
    if (batch <= 0) return 0;
    if (D & 7) { padt_set_error("padt_greedy_step: D % 8 == 0 required"); return -1; }
    GreedyArgs a{(const float*)part_val, (const int*)part_idx, (int)nblk, (int)batch, (int)D, eos, pad, (int)t_max,
                 unfinished, tokens_out, cur_tok, step, slot, lens, pos3, (const x16_t*)hidden, (x16_t*)hidden_buf,
                 advance, (const GenCfg*)gen_cfg, (unsigned*)seen, seen_words, nullptr, nullptr};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(greedy_step_kernel<false>, dim3((unsigned)batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// padt_greedy_step over the partials of padt_vrt_head_lse: also logprobs[b][*step] = log softmax(step's masked row)[selected token] — 0 for
// a row already finished on entry, -inf where the sentinel branch emits pad (no candidate) — nothing once *step >= t_max.
extern "C" int padt_greedy_step_lp(void* stream, const void* part_val, const void* part_idx, long nblk, long batch, long D,
                                   int eos, int pad, long t_max, int* unfinished, long* tokens_out, long* cur_tok,
                                   int* step, int* slot, int* lens, int* pos3, const void* hidden, void* hidden_buf,
                                   int advance, const void* gen_cfg, void* seen, long seen_words, const void* part_sum, void* logprobs) {
    if (batch <= 0) return 0;
    if (D & 7) { padt_set_error("padt_greedy_step_lp: D % 8 == 0 required"); return -1; }
    if (part_sum == nullptr || logprobs == nullptr) { padt_set_error("padt_greedy_step_lp: part_sum and logprobs are required"); return -1; }
    GreedyArgs a{(const float*)part_val, (const int*)part_idx, (int)nblk, (int)batch, (int)D, eos, pad, (int)t_max,
                 unfinished, tokens_out, cur_tok, step, slot, lens, pos3, (const x16_t*)hidden, (x16_t*)hidden_buf,
                 advance, (const GenCfg*)gen_cfg, (unsigned*)seen, seen_words, (const float*)part_sum, (float*)logprobs};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(greedy_step_kernel<true>, dim3((unsigned)batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// padt_greedy_step / padt_greedy_step_lp with a table of tokens the caller forces (generate(forced_tokens=)): forced int32 [batch][t_forced] in
// table columns.  After the arg-max (and the LSE fold), an unfinished row b with 0 <= forced[b][*step] < n_cols and 0 <= *step < t_forced takes
// that column as its token — appended, fed to the next step, entered in `seen`, checked against the EOS ids — even where its score is -inf; every
// other row is the free step.  part_sum / logprobs / probe_val (padt_vrt_head_probe's; all three or none): logprobs[b][*step] =
// probe == -inf ? -inf : (probe - max) - log Σ for a forced row, padt_greedy_step_lp's value elsewhere.
extern "C" int padt_forced_step(void* stream, const void* part_val, const void* part_idx, long nblk, long batch, long D,
                                int eos, int pad, long t_max, int* unfinished, long* tokens_out, long* cur_tok,
                                int* step, int* slot, int* lens, int* pos3, const void* hidden, void* hidden_buf,
                                int advance, const void* gen_cfg, void* seen, long seen_words, const void* part_sum, void* logprobs,
                                const int* forced, long t_forced, const void* probe_val, long n_cols) {
    if (batch <= 0) return 0;
    if (D & 7) { padt_set_error("padt_forced_step: D % 8 == 0 required"); return -1; }
    if (forced == nullptr || t_forced <= 0 || t_forced > 0x7fffffffL || n_cols <= 0 || n_cols > 0x7fffffffL || step == nullptr) {
        padt_set_error("padt_forced_step: the forced table [batch][t_forced], the step counter and the table's column count are required"); return -1;
    }
    const bool lp = part_sum != nullptr || logprobs != nullptr || probe_val != nullptr;
    if (lp && (part_sum == nullptr || logprobs == nullptr || probe_val == nullptr)) {
        padt_set_error("padt_forced_step: part_sum, logprobs and probe_val go together"); return -1;
    }
    if (seen && seen_words * 32 < n_cols) { padt_set_error("padt_forced_step: seen bitmap narrower than the table"); return -1; }
    GreedyArgs a{(const float*)part_val, (const int*)part_idx, (int)nblk, (int)batch, (int)D, eos, pad, (int)t_max,
                 unfinished, tokens_out, cur_tok, step, slot, lens, pos3, (const x16_t*)hidden, (x16_t*)hidden_buf,
                 advance, (const GenCfg*)gen_cfg, (unsigned*)seen, seen_words, (const float*)part_sum, (float*)logprobs,
                 forced, (int)t_forced, (const float*)probe_val, (int)n_cols};
    hipStream_t s = (hipStream_t)stream;
    if (lp) hipLaunchKernelGGL((greedy_step_kernel<true, true>), dim3((unsigned)batch), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((greedy_step_kernel<false, true>), dim3((unsigned)batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// Row path of generate(forced_tokens=) (the token comes from padt_sample_token / padt_warp_sample_rows_f32 / padt_argmax_rows_f32, not from the
// head's partials): part_idx[b] = forced[b][*step] for every unfinished row whose entry is a table column, so that padt_token_logprob_rows_f32
// scores the forced column; free and finished rows keep their draw / arg-max.
__global__ void forced_override_kernel(int* __restrict__ part_idx, const int* __restrict__ forced, int t_forced, const int* __restrict__ step,
                                       const int* __restrict__ unfinished, int n_cols, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    const int st = *step;
    if (b >= B || st < 0 || st >= t_forced || !unfinished[b]) return;
    const int f = forced[(long)b * t_forced + st];
    if (f >= 0 && f < n_cols) part_idx[b] = f;
}

extern "C" int padt_forced_override(void* stream, void* part_idx, const int* forced, long t_forced, const int* step, const int* unfinished,
                                    long n_cols, long batch) {
    if (batch <= 0) return 0;
    if (part_idx == nullptr || forced == nullptr || step == nullptr || unfinished == nullptr || t_forced <= 0 || t_forced > 0x7fffffffL ||
        n_cols <= 0 || n_cols > 0x7fffffffL || batch > 0x7fffffffL) {
        padt_set_error("padt_forced_override: the selection, the forced table [batch][t_forced], the step counter, the unfinished flags and the "
                       "table's column count are required"); return -1;
    }
    hipLaunchKernelGGL(forced_override_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (int*)part_idx, forced,
                       (int)t_forced, step, unfinished, (int)n_cols, (int)batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
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
PADT_DEV unsigned float_key(float f) {                                    // order-preserving float → uint
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PADT_DEV float key_float(unsigned k) {                                    // inverse of float_key
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(1024) void sample_token_kernel(float* logits, long ld, int n, const GenCfg* __restrict__ g,
                                                            const int* __restrict__ step, float* __restrict__ out_val,
                                                            int* __restrict__ out_idx) {
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
    red_v[tid] = mx;
    __syncthreads();
    for (int s2 = 512; s2 > 0; s2 >>= 1) {
        if (tid < s2) red_v[tid] = fmaxf(red_v[tid], red_v[tid + s2]);
        __syncthreads();
    }
    mx = red_v[0];
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
            best = (sval[tid] - mx) / T + gumbel_noise(seed, st, (unsigned)b, (unsigned)sidx[tid]);
            bidx = sidx[tid];
        }
        if (jk > 0) {
            const int last = tie_last;
            for (int i = tid; i < n && i <= last; i += 1024) {
                if (float_key(row[i]) == thresh) {
                    const float sc = (tv - mx) / T + gumbel_noise(seed, st, (unsigned)b, (unsigned)i);
                    if (sc > best || (sc == best && i < bidx)) { best = sc; bidx = i; }
                }
            }
        }
    } else {
        for (int i = tid; i < n; i += 1024) {
            const float v = row[i];
            if (float_key(v) >= thresh) {
                const float sc = (v - mx) / T + gumbel_noise(seed, st, (unsigned)b, (unsigned)i);
                if (sc > best || (sc == best && i < bidx)) { best = sc; bidx = i; }
            }
        }
    }
    __syncthreads();
    red_v[tid] = best;
    red_i[tid] = bidx;
    __syncthreads();
    for (int s2 = 512; s2 > 0; s2 >>= 1) {
        if (tid < s2) {
            const float ov = red_v[tid + s2];
            const int oi = red_i[tid + s2];
            if (ov > red_v[tid] || (ov == red_v[tid] && oi < red_i[tid])) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
    }
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
                       (int)n_rows_table, (const GenCfg*)gen_cfg, step, (float*)part_val, (int*)part_idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// Arg-max of fp32 score rows (round 6: the selection of the HOOKED decode loop — caller-supplied `logits_processor`s of padt.py:717 have rewritten
// the step's score rows between the head kernel and the selection, so the head's fused arg-max partials no longer describe them): one block per
// row, ties → lowest index (torch.argmax, padt.py:745), one (value, index) partial per row in the layout padt_greedy_step reads with nblk = 1.
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
    red_v[tid] = best;
    red_i[tid] = bidx;
    __syncthreads();
    for (int s2 = 512; s2 > 0; s2 >>= 1) {
        if (tid < s2) {
            const float ov = red_v[tid + s2], cv = red_v[tid];
            const int oi = red_i[tid + s2], ci = red_i[tid];
            const bool o_nan = ov != ov, c_nan = cv != cv;
            const bool take = (o_nan && !c_nan) || (o_nan == c_nan && (ov > cv || ((ov == cv || o_nan) && oi < ci)));
            if (take) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
    }
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
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
    red[tid] = mx;
    __syncthreads();
    for (int s2 = 512; s2 > 0; s2 >>= 1) {
        if (tid < s2) { const float o = red[tid + s2], c = red[tid]; red[tid] = (o > c || o != o) ? o : c; }
        __syncthreads();
    }
    const float M = red[0];
    __syncthreads();
    float acc = 0.f;
    for (int i = tid; i < n; i += 1024) {
        const float v = row[i];
        acc += v == -INFINITY ? 0.f : __builtin_amdgcn_exp2f((v - M) * 1.44269504088896341f);
    }
    red[tid] = acc;
    __syncthreads();
    for (int s2 = 512; s2 > 0; s2 >>= 1) {
        if (tid < s2) red[tid] += red[tid + s2];
        __syncthreads();
    }
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
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// What generate()'s synchronising half needs from the device, in ONE launch and ONE small D2H copy (round 6: replaces a torch.cat of flag
// tensors, `unfinished.any()` per chunk and isin / argmax / max over the token ring — seven ATen reduce launches and three host syncs per
// batch): out = [err, any(unfinished), nf_rows[n_rows], nf_batch[n_batch], first_eos[n_rows]] with first_eos[r] = the first step t < done whose
// token is one of the EOS ids (config eos or gen->eos[0..3]), -1 if none — the reference stops right after the step in which the last
// sequence finished (padt.py:756-757), so a batch's length is max over its rows of first_eos + 1.
struct CollectArgs {
    const int* err; const int* unfinished; const int* nf_rows; const int* nf_batch; int n_rows, n_batch;
    const long* tokens; int T_max, done, eos; const GenCfg* gen; int* out;
};
__global__ __launch_bounds__(256) void collect_summary_kernel(CollectArgs p) {
    const int tid = threadIdx.x;
    int unf = 0;
    for (int r = tid; r < p.n_rows; r += 256) {
        unf |= p.unfinished[r];
        p.out[2 + r] = p.nf_rows[r];
        int first = -1;
        const long* row = p.tokens + (long)r * p.T_max;
        for (int t = 0; t < p.done && first < 0; ++t) {
            const long tok = row[t];
            bool is_eos = tok == (long)p.eos;
            if (p.gen) {
#pragma unroll
                for (int k = 0; k < 4; ++k) is_eos = is_eos || (p.gen->eos[k] >= 0 && tok == (long)p.gen->eos[k]);
            }
            if (is_eos) first = t;
        }
        p.out[2 + p.n_rows + p.n_batch + r] = first;
    }
    for (int b = tid; b < p.n_batch; b += 256) p.out[2 + p.n_rows + b] = p.nf_batch[b];
    const int any = __syncthreads_or(unf);
    if (tid == 0) { p.out[0] = p.err ? *p.err : 0; p.out[1] = any ? 1 : 0; }
}

extern "C" int padt_collect_summary(void* stream, const int* err, const int* unfinished, const int* nf_rows, const int* nf_batch, long n_rows,
                                    long n_batch, const long* tokens, long t_max, long done, int eos, const void* gen_cfg, int* out) {
    if (n_rows <= 0 || n_batch < 0 || done < 0 || done > t_max || out == nullptr) { padt_set_error("padt_collect_summary: bad arguments"); return -1; }
    CollectArgs a{err, unfinished, nf_rows, nf_batch, (int)n_rows, (int)n_batch, tokens, (int)t_max, (int)done, eos, (const GenCfg*)gen_cfg, out};
    hipLaunchKernelGGL(collect_summary_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// sequences[b] = [input_ids[b] (L) | tokens[row0 + b][0 .. n_steps)] with the session-global VRT ids of a merged decode group shifted back to
// the batch's own (id >= vocab → id - proto_row0): the `torch.cat([input_ids, next_tokens])` of padt.py:751 for one batch of the group.
__global__ void assemble_sequences_kernel(const long* __restrict__ ids, long ld_ids, int L, const long* __restrict__ tokens, long T_max,
                                          int n_steps, long vocab, long proto_row0, long* __restrict__ out, int B) {
    const int W = L + n_steps;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * W; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / W), c = (int)(i % W);
        long v;
        if (c < L) v = ids[(long)b * ld_ids + c];
        else {
            v = tokens[(long)b * T_max + (c - L)];
            if (v >= vocab) v -= proto_row0;
        }
        out[i] = v;
    }
}

extern "C" int padt_assemble_sequences(void* stream, const long* input_ids, long ld_ids, long L, const long* tokens, long t_max, long n_steps,
                                       long vocab, long proto_row0, long* out, long batch) {
    if (batch <= 0 || L + n_steps <= 0) return 0;
    if (n_steps < 0 || n_steps > t_max || L < 0) { padt_set_error("padt_assemble_sequences: bad arguments"); return -1; }
    const long n = batch * (L + n_steps);
    long blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(assemble_sequences_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, input_ids, ld_ids, (int)L, tokens, t_max,
                       (int)n_steps, vocab, proto_row0, out, (int)batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// past_logit_mask (padt.py:196-201, returned at :794): mask[b][c] = c < vocab || vrt_off[b] <= c - vocab + off0 < vrt_off[b + 1] — one byte per
// table column; vrt_off are the session's prototype row offsets of the batch's rows, off0 = the batch's first prototype row in the session.
__global__ void logit_mask_kernel(const int* __restrict__ vrt_off, long vocab, long table_rows, long off0, unsigned char* __restrict__ out, int B) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < (long)B * table_rows; i += (long)gridDim.x * blockDim.x) {
        const int b = (int)(i / table_rows);
        const long c = i % table_rows;
        out[i] = (c < vocab || (c - vocab + off0 >= vrt_off[b] && c - vocab + off0 < vrt_off[b + 1])) ? 1 : 0;
    }
}

extern "C" int padt_logit_mask(void* stream, const int* vrt_off, long vocab, long table_rows, long proto_row0, void* out_u8, long batch) {
    if (batch <= 0 || table_rows <= 0) return 0;
    const long n = batch * table_rows;
    long blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(logit_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, vrt_off, vocab, table_rows, proto_row0,
                       (unsigned char*)out_u8, (int)batch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// output_scores=True (padt.py:719-720: `scores += (next_token_scores,)`): dst[*step][0..n) = src[0..n) — the masked / penalised fp32 logit rows
// the head kernel just wrote, filed under the DEVICE step counter so the copy can sit inside the captured decode graph.
__global__ void stash_step_f32_kernel(const float* __restrict__ src, long n, const int* __restrict__ step, long t_max, float* __restrict__ dst) {
    const long s = *step;
    if (s < 0 || s >= t_max) return;
    float* d = dst + s * n;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
        reinterpret_cast<f32x4*>(d)[i] = reinterpret_cast<const f32x4*>(src)[i];
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) d[n4 * 4 + threadIdx.x] = src[n4 * 4 + threadIdx.x];
}

extern "C" int padt_stash_step_f32(void* stream, const void* src_f32, long n, const int* step, long t_max, void* dst_f32) {
    if (n <= 0) return 0;
    if (((size_t)src_f32 | (size_t)dst_f32) & 15 || (n & 3)) { padt_set_error("padt_stash_step_f32: 16-byte aligned buffers and n % 4 == 0 required"); return -1; }
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(stash_step_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)src_f32, n, step, t_max, (float*)dst_f32);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}

// seen[row[i]] |= bit(ids[i]) for every prompt token (ids already global in the session's table); ids outside the table are
// ignored (the range assert of padt.py:203 is reported by the embedding kernel).
__global__ void seen_init_kernel(const long* __restrict__ ids, const int* __restrict__ rows, long n, unsigned* seen, long words) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long id = ids[i];
        if (id >= 0 && id < words * 32) atomicOr(&seen[(long)rows[i] * words + (id >> 5)], 1u << (id & 31));
    }
}

extern "C" int padt_seen_init(void* stream, const long* ids, const int* rows, long n, void* seen, long seen_words) {
    if (n <= 0) return 0;
    long blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(seen_init_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ids, rows, n, (unsigned*)seen, seen_words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { padt_set_error(hipGetErrorString(e)); return -2; }
    return 0;
}
#endif

}  // namespace PADT_NS
