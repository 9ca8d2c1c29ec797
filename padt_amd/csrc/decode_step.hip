// The bookkeeping of a decode step, on the device so that a step is one replayable hipGraph.  Type-independent (hidden rows are copied as
// 16-bit words): compiled once.
//
// greedy_step_kernel: final reduction of the head's block partials (vrt_head.hip; or one partial per row from sampling.hip) — ties →
// lowest index, as torch.argmax —, pad/EOS bookkeeping (padt.py:749-757), append to the token buffer, stash the step's last-layer hidden row
// for parseVRTintoCompletion (padt_processor.py:125), advance cache slots / rope positions / step counter.  Around it: the forced-token
// override of the row path, the seen-bitmap init, and what generate() reads back or assembles after the loop (collect summary, sequences,
// logit mask, score stash).
#include "block_reduce.h"
#include "gen_cfg.h"

namespace PADT_NS {

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
        if (argmax_less(best, bidx, v, ix)) { best = v; bidx = ix; }
    }
    block_argmax_lds<256>(best, bidx, sv, si);
    if constexpr (LP) {
        const float M = sv[0];
        float acc = 0.f;
        for (int i = tid; i < p.nblk; i += 256) {
            const float s = p.part_sum[(long)i * p.B + b];
            const float v = p.part_val[(long)i * p.B + b];
            acc += (s == 0.f || v == -INFINITY) ? 0.f : s * __builtin_amdgcn_exp2f((v - M) * 1.44269504088896341f);
        }
        block_sum_lds<256>(acc, ss);
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
        // ... and so has a row whose best value is -inf (padt_argmax_rows_f32 reports column 0 for it, torch.argmax's answer: every column
        // was banned by a caller's processor on the hooked loop) — the head's and the samplers' partials carry the sentinel there already
        const bool no_choice = si[0] == 0x7fffffff || sv[0] == -INFINITY || next < 0 || (p.seen && (next >> 5) >= p.seen_words);
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
        p.unfinished[b] = unf & (gen_is_eos(p.gen, next, p.eos) ? 0 : 1);   // padt.py:756
        if (p.seen) p.seen[(long)b * p.seen_words + (next >> 5)] |= 1u << (next & 31);   // the row now contains `next`
        if (p.advance) {
            p.slot[b] += 1; p.lens[b] += 1;
            p.pos3[b] += 1; p.pos3[p.B + b] += 1; p.pos3[2 * p.B + b] += 1;
        }
    }
}

// one-thread kernel: bump the step counter after all samples' greedy_step blocks ran
__global__ void step_inc_kernel(int* step) { *step += 1; }

// The argument block of the three step entry points, built once; the slots an entry point does not have stay null / 0.
static GreedyArgs step_args(const void* part_val, const void* part_idx, long nblk, long batch, long D, int eos, int pad, long t_max,
                            int* unfinished, long* tokens_out, long* cur_tok, int* step, int* slot, int* lens, int* pos3, const void* hidden,
                            void* hidden_buf, int advance, const void* gen_cfg, void* seen, long seen_words, const void* part_sum = nullptr,
                            void* logprobs = nullptr, const int* forced = nullptr, long t_forced = 0, const void* probe_val = nullptr,
                            long n_cols = 0) {
    return GreedyArgs{(const float*)part_val, (const int*)part_idx, (int)nblk, (int)batch, (int)D, eos, pad, (int)t_max,
                      unfinished, tokens_out, cur_tok, step, slot, lens, pos3, (const x16_t*)hidden, (x16_t*)hidden_buf,
                      advance, (const GenCfg*)gen_cfg, (unsigned*)seen, seen_words, (const float*)part_sum, (float*)logprobs,
                      forced, (int)t_forced, (const float*)probe_val, (int)n_cols};
}

// one block per row, then the step counter
static int launch_step(const GreedyArgs& a, bool lp, bool forced, hipStream_t s) {
    const dim3 grid((unsigned)a.B), block(256);
    if (forced) {
        if (lp) hipLaunchKernelGGL((greedy_step_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((greedy_step_kernel<false, true>), grid, block, 0, s, a);
    } else if (lp) hipLaunchKernelGGL(greedy_step_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(greedy_step_kernel<false>, grid, block, 0, s, a);
    hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, a.step);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_greedy_step(void* stream, const void* part_val, const void* part_idx, long nblk, long batch, long D,
                                int eos, int pad, long t_max, int* unfinished, long* tokens_out, long* cur_tok,
                                int* step, int* slot, int* lens, int* pos3, const void* hidden, void* hidden_buf,
                                int advance, const void* gen_cfg, void* seen, long seen_words) {
    if (batch <= 0) return 0;
    if (D & 7) { padt_set_error("padt_greedy_step: D % 8 == 0 required"); return -1; }
    return launch_step(step_args(part_val, part_idx, nblk, batch, D, eos, pad, t_max, unfinished, tokens_out, cur_tok, step, slot, lens, pos3,
                                 hidden, hidden_buf, advance, gen_cfg, seen, seen_words), false, false, (hipStream_t)stream);
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
    return launch_step(step_args(part_val, part_idx, nblk, batch, D, eos, pad, t_max, unfinished, tokens_out, cur_tok, step, slot, lens, pos3,
                                 hidden, hidden_buf, advance, gen_cfg, seen, seen_words, part_sum, logprobs), true, false, (hipStream_t)stream);
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
    return launch_step(step_args(part_val, part_idx, nblk, batch, D, eos, pad, t_max, unfinished, tokens_out, cur_tok, step, slot, lens, pos3,
                                 hidden, hidden_buf, advance, gen_cfg, seen, seen_words, part_sum, logprobs, forced, t_forced, probe_val, n_cols),
                       lp, true, (hipStream_t)stream);
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
    PADT_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// What generate()'s synchronising half needs from the device, in ONE launch and ONE small D2H copy (round 6: replaces a torch.cat of flag
// tensors, `unfinished.any()` per chunk and isin / argmax / max over the token ring — seven ATen reduce launches and three host syncs per
// batch): out = [err, any(unfinished), nf_rows[n_rows], nf_batch[n_batch], first_eos[n_rows]] with first_eos[r] = the first step t < done whose
// token is one of the EOS ids (config eos or gen->eos[0..3]), -1 if none — the reference stops right after the step in which the last
// sequence finished (padt.py:756-757), so a batch's length is max over its rows of first_eos + 1.
// STOP (padt_collect_summary_stop; generate(stop_sequences=, min_tokens=, max_tokens=)): behind that record, what padt_stop_match recorded per
// row — finish_step[n_rows], finish_reason[n_rows], stop_index[n_rows] — so that a row ended by anything but an EOS id has an end too.
struct CollectArgs {
    const int* err; const int* unfinished; const int* nf_rows; const int* nf_batch; int n_rows, n_batch;
    const long* tokens; int T_max, done, eos; const GenCfg* gen; int* out;
    const int* finish_step; const int* finish_reason; const int* stop_index;      // STOP
};
template <bool STOP>
__global__ __launch_bounds__(256) void collect_summary_kernel(CollectArgs p) {
    const int tid = threadIdx.x;
    int unf = 0;
    for (int r = tid; r < p.n_rows; r += 256) {
        unf |= p.unfinished[r];
        p.out[2 + r] = p.nf_rows[r];
        int first = -1;
        const long* row = p.tokens + (long)r * p.T_max;
        for (int t = 0; t < p.done && first < 0; ++t) {
            if (gen_is_eos(p.gen, row[t], p.eos)) first = t;
        }
        p.out[2 + p.n_rows + p.n_batch + r] = first;
        if constexpr (STOP) {
            int* tail = p.out + 2 + 2 * p.n_rows + p.n_batch;
            tail[r] = p.finish_step[r];
            tail[p.n_rows + r] = p.finish_reason[r];
            tail[2 * p.n_rows + r] = p.stop_index[r];
        }
    }
    for (int b = tid; b < p.n_batch; b += 256) p.out[2 + p.n_rows + b] = p.nf_batch[b];
    const int any = __syncthreads_or(unf);
    if (tid == 0) { p.out[0] = p.err ? *p.err : 0; p.out[1] = any ? 1 : 0; }
}

extern "C" int padt_collect_summary(void* stream, const int* err, const int* unfinished, const int* nf_rows, const int* nf_batch, long n_rows,
                                    long n_batch, const long* tokens, long t_max, long done, int eos, const void* gen_cfg, int* out) {
    if (n_rows <= 0 || n_batch < 0 || done < 0 || done > t_max || out == nullptr) { padt_set_error("padt_collect_summary: bad arguments"); return -1; }
    CollectArgs a{err, unfinished, nf_rows, nf_batch, (int)n_rows, (int)n_batch, tokens, (int)t_max, (int)done, eos, (const GenCfg*)gen_cfg, out,
                  nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(collect_summary_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}

// padt_collect_summary with the rows' finish records behind its record: out holds 2 + 5 n_rows + n_batch int32.
extern "C" int padt_collect_summary_stop(void* stream, const int* err, const int* unfinished, const int* nf_rows, const int* nf_batch,
                                         long n_rows, long n_batch, const long* tokens, long t_max, long done, int eos, const void* gen_cfg,
                                         const int* finish_step, const int* finish_reason, const int* stop_index, int* out) {
    if (n_rows <= 0 || n_batch < 0 || done < 0 || done > t_max || out == nullptr || !finish_step || !finish_reason || !stop_index) {
        padt_set_error("padt_collect_summary_stop: bad arguments"); return -1;
    }
    CollectArgs a{err, unfinished, nf_rows, nf_batch, (int)n_rows, (int)n_batch, tokens, (int)t_max, (int)done, eos, (const GenCfg*)gen_cfg, out,
                  finish_step, finish_reason, stop_index};
    hipLaunchKernelGGL(collect_summary_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
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
    PADT_CHECK_LAUNCH();
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
    PADT_CHECK_LAUNCH();
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
    PADT_CHECK_LAUNCH();
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
    PADT_CHECK_LAUNCH();
    return 0;
}

}  // namespace PADT_NS
