// VRT logit head with fused logit mask + arg-max partials.
//
// Reference (padt.py:292-301, 713-757): logits = hidden @ cat([embed_tokens|lm_head, prototypes]).T, masked_fill(-inf)
// outside [text vocab ∪ the sample's own patch rows], argmax of the last position in fp32.  Here the two tables are read through two base
// pointers (the 0.6 GB concatenation per forward never happens), only the last position is computed, and the logits never touch HBM unless
// a caller asks for them.
//
// vrt_head_kernel: block = 4 waves = 16 table rows, K interleaved over the waves (same weight-streaming scheme as the
// skinny GEMM), swapped MFMA so a lane owns 4 consecutive table rows of one sample; block-local (max, argmax) per
// sample goes to a partial buffer, which greedy_step_kernel (decode_step.hip) reduces.  This is the only file of the token selection that
// depends on the 16-bit operand type: the step bookkeeping (decode_step.hip), the sampling kernels (sampling.hip) and the ban bitmaps
// (gen_rules.hip, token_automaton.hip) are compiled once.
#include "gen_cfg.h"
#include <stdlib.h>
#include <cstdint>

extern "C" long padt_vrt_head_nblk(long vocab, long n_proto);

namespace PADT_NS {

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
    const float* bias;                 // optional [V + NP] additive bias over the table columns (generate(logit_bias=, patch_bias=)): logit + bias[row]
    const float* decay; int t_decay;   // optional [t_decay] a[t] of generate(exponential_decay_length_penalty=), read at *step: 0 = no change
};

// HF's ExponentialDecayLengthPenalty on one EOS column: v + |v| * a, the product and the sum rounded separately as HF's two tensor ops are (a
// contraction into one FMA would change the last bit).  -inf stays -inf (HF: NaN).
PADT_DEV float eos_decay(float v, float a) {
#pragma clang fp contract(off)
    const float pen = fabsf(v) * a;
    return v == -INFINITY ? v : v + pen;
}

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
// EDIT (padt_vrt_head_bias with a bias vector and / or a decay table; every other launch is EDIT = false and compiles to the code it was
// before the flag existed — whether two runtime null tests would have cost the plain step anything was not settled, profiles/score_bias.md §2): HF's
// processor order — the bias is added to the raw logit BEFORE the repetition penalty (SequenceBias comes first), the mask / schedule / ban
// filter follows, and a surviving EOS column (the config's id or one of gen's) becomes v + |v| * decay[*step] LAST
// (ExponentialDecayLengthPenalty).  Every consumer — the written row, the arg-max and LSE partials, the probe value — sees the edited value.
template <int MT, int NT, bool PACKED, bool LSE = false, bool PROBE = false, bool EDIT = false>
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
    float dec = 0.f;                                              // EDIT: this step's a[t]; 0 (before `start`, past the table, no table): no edit
    int dcol[5] = {-1, -1, -1, -1, -1};                           // ... and the columns it edits, read once: the config's EOS id and gen's list
    if constexpr (EDIT) {
        if (p.decay) { const int st = *p.step; if (st >= 0 && st < p.t_decay) dec = p.decay[st]; }
        if (dec != 0.f) {
            dcol[0] = p.eos;
            if (p.gen) {
#pragma unroll
                for (int k = 0; k < 4; ++k) dcol[1 + k] = p.gen->eos[k];
            }
        }
    }
    for (int q = wave; q < NT * MT; q += 4) {                     // (table block, sample block) pairs this wave finishes
        const int i = q / MT, j = q % MT;
        const int blk = blockIdx.x * NT + i;
        if (blk >= nblk) continue;
        const int n0 = blk * 16;
        float bv[4] = {0.f, 0.f, 0.f, 0.f};                       // EDIT: the lane's four bias values, asked for before the LDS reads below
        if constexpr (EDIT) {
            if (p.bias) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int row = n0 + fq * 4 + r; if (row < NTOT) bv[r] = p.bias[row]; }
            }
        }
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
            if constexpr (EDIT) {
                if (p.bias) sc += bv[r];
            }
            if (pen != 1.0f && ok && ((p.seen[(long)m * p.seen_words + (row >> 5)] >> (row & 31)) & 1u)) sc = sc < 0.f ? sc * pen : sc / pen;
            float v = ok ? sc : -INFINITY;
            if constexpr (EDIT) {
                if (dec != 0.f && row < p.V && (row == dcol[0] || row == dcol[1] || row == dcol[2] || row == dcol[3] || row == dcol[4])) v = eos_decay(v, dec);
            }
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

template <int MT, int NT, bool PACKED, bool LSE, bool PROBE, bool EDIT>
static void launch_head(const HeadArgs& a, int nblk, hipStream_t s) {
    constexpr int lds = 4 * NT * MT * 64 * 16;
    if constexpr (lds > 64 * 1024) {
        static PerDeviceOnce once;
        once.run([] { (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&vrt_head_kernel<MT, NT, PACKED, LSE, PROBE, EDIT>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, lds); });
    }
    hipLaunchKernelGGL((vrt_head_kernel<MT, NT, PACKED, LSE, PROBE, EDIT>), dim3((nblk + NT - 1) / NT), dim3(256), lds, s, a);
}

template <bool LSE, bool PROBE = false, bool EDIT = false>
static void dispatch_head(const HeadArgs& a, int nblk, hipStream_t s) {
    if (a.Ep) {                                                 // NT = 4 table blocks per thread block (2 at 128 rows): profiles/r03_head_nt_ab.log
        if (a.B <= 16) launch_head<1, 4, true, LSE, PROBE, EDIT>(a, nblk, s);
        else if (a.B <= 32) launch_head<2, 4, true, LSE, PROBE, EDIT>(a, nblk, s);
        else if (a.B <= 64) launch_head<4, 4, true, LSE, PROBE, EDIT>(a, nblk, s);
        else launch_head<8, 2, true, LSE, PROBE, EDIT>(a, nblk, s);
    } else if (a.B <= 16) launch_head<1, 1, false, LSE, PROBE, EDIT>(a, nblk, s);
    else if (a.B <= 32) launch_head<2, 1, false, LSE, PROBE, EDIT>(a, nblk, s);
    else if (a.B <= 64) launch_head<4, 1, false, LSE, PROBE, EDIT>(a, nblk, s);
    else launch_head<8, 1, false, LSE, PROBE, EDIT>(a, nblk, s);
}

static int vrt_head_impl(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                         const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                         const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                         long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                         const void* seen, long seen_words, const void* ban, long ban_words, void* part_sum = nullptr,
                         const int* forced = nullptr, long t_forced = 0, void* probe_val = nullptr, const void* bias = nullptr,
                         const void* decay = nullptr, long t_decay = 0) {
    if (batch <= 0) return 0;
    if (batch > 128 || (D & 7) || (ldh & 7)) { padt_set_error("padt_vrt_head: batch <= 128, D % 8 == 0 required"); return -1; }
    if (embed_table_packed && ((D & 31) || (vocab & 15) || ((uintptr_t)embed_table_packed & 15) || ((uintptr_t)hidden & 15))) {
        padt_set_error("padt_vrt_head: the packed path needs D % 32 == 0, vocab % 16 == 0 and 16-byte aligned pointers");
        return -1;
    }
    HeadArgs a{(const x16_t*)hidden, ldh, (const x16_t*)embed_table, (int)vocab, (const x16_t*)proto, (int)n_proto,
               vrt_off, mode_table, step, (float*)logits_f32, ld_logits, (float*)part_val, (int*)part_idx, (int)batch,
               (int)D, eos, (const x16_t*)embed_table_packed, (const GenCfg*)gen_cfg, (const unsigned*)seen, seen_words,
               (const unsigned*)ban, ban_words, (float*)part_sum, forced, (int)t_forced, (float*)probe_val, (const float*)bias,
               (const float*)decay, (int)t_decay};
    if (seen && seen_words * 32 < vocab + n_proto) { padt_set_error("padt_vrt_head: seen bitmap narrower than the table"); return -1; }
    if (ban && ban_words * 32 < vocab + n_proto) { padt_set_error("padt_vrt_head_ban: ban bitmap narrower than the table"); return -1; }
    const int nblk = (int)padt_vrt_head_nblk(vocab, n_proto);
    hipStream_t s = (hipStream_t)stream;
    if (bias || decay) {                                        // the EDIT instantiations: the only launches that read the two pointers
        if (forced) dispatch_head<true, true, true>(a, nblk, s);
        else if (part_sum) dispatch_head<true, false, true>(a, nblk, s);
        else dispatch_head<false, false, true>(a, nblk, s);
    } else if (forced) dispatch_head<true, true>(a, nblk, s);
    else if (part_sum) dispatch_head<true>(a, nblk, s);
    else dispatch_head<false>(a, nblk, s);
    PADT_CHECK_LAUNCH();
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

// Every head above with an additive score bias and / or the exponential length decay (generate(logit_bias=, patch_bias=,
// exponential_decay_length_penalty=)); bias fp32 [vocab + n_proto] or null, decay fp32 [t_decay] or null (then t_decay is ignored), read at *step.
// The head is chosen as the other entry points choose it: forced != null → the probe head (part_sum, probe_val and t_forced required), else
// part_sum != null → the LSE head, else the plain head; ban is optional in all three.  bias = decay = null is that head, bit for bit.
extern "C" int PADT_TWIN(padt_vrt_head_bias)(void* stream, const void* hidden, long ldh, const void* embed_table, long vocab,
                             const void* proto, long n_proto, const int* vrt_off, const int* mode_table,
                             const int* step, void* logits_f32, long ld_logits, void* part_val, void* part_idx,
                             long batch, long D, int eos, const void* embed_table_packed, const void* gen_cfg,
                             const void* seen, long seen_words, const void* ban, long ban_words, void* part_sum,
                             const int* forced, long t_forced, void* probe_val, const void* bias, const void* decay, long t_decay) {
    if (batch <= 0) return 0;
    if (forced && (part_sum == nullptr || probe_val == nullptr || step == nullptr || t_forced <= 0 || t_forced > 0x7fffffffL)) {
        padt_set_error("padt_vrt_head_bias: a forced table needs part_sum, the step counter, t_forced > 0 and probe_val"); return -1;
    }
    if (decay && (step == nullptr || t_decay <= 0 || t_decay > 0x7fffffffL)) {
        padt_set_error("padt_vrt_head_bias: the decay table needs the step counter and 0 < t_decay < 2^31"); return -1;
    }
    return vrt_head_impl(stream, hidden, ldh, embed_table, vocab, proto, n_proto, vrt_off, mode_table, step, logits_f32, ld_logits, part_val,
                         part_idx, batch, D, eos, embed_table_packed, gen_cfg, seen, seen_words, ban, ban_words, part_sum,
                         forced, forced ? t_forced : 0, forced ? probe_val : nullptr, bias, decay, decay ? t_decay : 0);
}

}  // namespace PADT_NS

#if !PADT_OP16_F16   // type-independent: compiled once
extern "C" long padt_vrt_head_nblk(long vocab, long n_proto) { return (vocab + n_proto + 15) / 16; }
#endif
