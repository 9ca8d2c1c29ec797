// Beam search inside the decode step (generate(beam_width=K)): the K best hypotheses of every sample are kept, scored and reordered on the
// device, so that a beam step stays one replayable hipGraph.  Type-independent (hidden rows and cache words move as raw bits): compiled once.
//
// beam_step_kernel     one block per sample, in the place of greedy_step_kernel: merges the K live rows' `keep` best (log-prob, column) pairs
//                      (padt_topk_logprob_rows_f32's output of this step), selects the next live beams, files finished hypotheses in the
//                      sample's store, decides whether the sample is done — generation.beam_step is the specification, applied bit for bit —
//                      and does greedy_step_kernel's chores for the sample's K rows.
// beam_cand_lp_kernel  (output_token_logprobs) the log-prob REPORTED for each of a row's candidates: (score - M) - log S with M and S folded
//                      from the LSE head's block partials exactly as padt_greedy_step_lp folds them, so that a hypothesis' token_logprobs are
//                      the bits the greedy call and score_completions report for the same row; the search itself adds the top-k kernel's values.
// beam_reorder_kernel  makes the packed KV caches of every layer follow the beams: child row c of a sample gets the generated slots of row
//                      perm[c], in place.
// beam_finalize_kernel once per call, one block per returned hypothesis: back-trace through the steps' records, tokens / log-probs / score /
//                      length, and the hypothesis's hidden rows gathered from hidden_buf.
#include "block_reduce.h"
#include "gen_cfg.h"

namespace PADT_NS {

constexpr int BEAM_MAX_K = 8;        // generation.BEAM_MAX_WIDTH
constexpr int BEAM_MAX_KEEP = 32;    // ops.TOPK_ROWS_MAX_K
constexpr int BEAM_CFG_MAGIC = 0x424d3031;

// The beam config in DEVICE memory (ops.beam_cfg_tensor): one captured graph per width serves every early-stopping mode and call length.
struct BeamCfg {
    int magic, K, keep;
    int early;        // generation.BEAM_EARLY: 0 False, 1 True, 2 "never"
    int t_last;       // the call's last step, max_new_tokens - 1: every candidate of that step is finishing
    int never_max;    // early == "never" and length penalty > 0: the heuristic divides by len_table[t_last]
    int pad0, pad1;
};
static_assert(sizeof(BeamCfg) == 32, "BeamCfg is 8 ints (ops.BEAM_CFG_INTS)");

struct BeamStepArgs {
    const int* top_idx; const float* top_val;      // [B * K][t_top][keep]: read at *step
    const float* rep_lp;                           // optional [B * K][keep]: the log-prob recorded for a candidate (null: its top_val)
    int t_top, keep, B, K, D, T_max;
    const BeamCfg* cfg; const float* len_table;    // [T_max]
    const GenCfg* gen; int eos, pad;
    long vocab, n_cols; const int* vrt_off;        // [B * K + 1]
    // per sample: live scores, the finished store, its flags
    float* live; float* st_score; float* st_lp; int* st_end; int* st_parent; int* st_tok; int* sent;      // [B][K]
    int* flags;                                    // [B][2] = (open: the early-stop heuristic is not satisfied yet, done)
    // per step and row: what the back-trace reads
    int* beam_tok; int* beam_parent; float* beam_lp;       // [T_max][B * K]
    int* perm;                                     // [B * K]: this step's parent of every row (identity for a done sample): beam_reorder_kernel's input
    long* cur_tok; int* unfinished; int* step; int* slot; int* lens; int* pos3;
    const x16_t* hidden; x16_t* hidden_buf;        // [B * K][D], [T_max][B * K][D]
    int advance; int* err;
};

// candidate a orders before candidate b: value descending, then lower beam, then lower rank (a total order: no two share beam and rank)
PADT_DEV bool beam_before(float va, int ka, float vb, int kb) { return va > vb || (va == vb && ka < kb); }

__global__ __launch_bounds__(256) void beam_step_kernel(BeamStepArgs p) {
    __shared__ float cv[BEAM_MAX_K * BEAM_MAX_KEEP];      // value of candidate (beam, rank), -inf: no candidate
    __shared__ float sv[BEAM_MAX_KEEP]; __shared__ int sk[BEAM_MAX_KEEP];      // the step's candidates in order: value, beam * keep + rank
    __shared__ int n_cand;
    const int b = blockIdx.x, tid = threadIdx.x, K = p.K, keep = p.keep;
    const int step = *p.step;
    const int row0 = b * K;
    // greedy_step's first chore: the step's hidden rows of the sample's K rows
    if (step >= 0 && step < p.T_max) {
        const int per_row = p.D / 8;
        for (int i = tid; i < K * per_row; i += 256) {
            const int r = i / per_row, c = (i - r * per_row) * 8;
            *reinterpret_cast<u32x4*>(p.hidden_buf + ((long)step * p.B * K + row0 + r) * p.D + c) =
                *reinterpret_cast<const u32x4*>(p.hidden + (long)(row0 + r) * p.D + c);
        }
    }
    const bool cfg_ok = p.cfg->magic == BEAM_CFG_MAGIC && p.cfg->K == K && p.cfg->keep == keep;
    const bool active = cfg_ok && step >= 0 && step < p.T_max && step < p.t_top && p.flags[2 * b + 1] == 0;
    if (tid == 0) n_cand = 0;
    // 1. the accumulated values; 2. their order
    const int n_all = K * keep;
    float v = -INFINITY;
    if (active && tid < n_all) {
        const int beam = tid / keep, r = tid - beam * keep;
        const long at = ((long)(row0 + beam) * p.t_top + step) * keep + r;
        const float lv = p.live[row0 + beam], lp = p.top_val[at];
        const int col = p.top_idx[at];
        if (lv != -INFINITY && col >= 0 && lp == lp && lp != -INFINITY) v = lv + lp;
        if (!(v == v)) v = -INFINITY;
    }
    if (tid < BEAM_MAX_K * BEAM_MAX_KEEP) cv[tid] = v;
    __syncthreads();
    if (active && tid < n_all && v != -INFINITY) {
        int rank = 0;
        for (int j = 0; j < n_all; ++j) rank += beam_before(cv[j], j, v, tid) ? 1 : 0;
        if (rank < keep) { sv[rank] = v; sk[rank] = tid; atomicAdd(&n_cand, 1); }      // LDS counter; every slot below it is written exactly once
    }
    __syncthreads();
    // 3.-7. one thread walks the <= 32 candidates; it is also the ONE thread that writes the sample's child rows
    if (tid == 0) {
        int tok[BEAM_MAX_K], par[BEAM_MAX_K]; float lps[BEAM_MAX_K], nl[BEAM_MAX_K];
        long feed[BEAM_MAX_K];
#pragma unroll
        for (int c = 0; c < BEAM_MAX_K; ++c) { tok[c] = p.pad; par[c] = c; lps[c] = 0.f; nl[c] = -INFINITY; feed[c] = p.pad; }
        bool done = !cfg_ok || p.flags[2 * b + 1] != 0;
        if (!cfg_ok && p.err) *p.err = 1;
        if (active) {
            const int n = n_cand < keep ? n_cand : keep;
            const float div_t = p.len_table[step];
            bool open = p.flags[2 * b] != 0;
            bool full = true;
            for (int c = 0; c < K; ++c) full = full && p.sent[row0 + c] != 0;
            const bool merge = open && !(p.cfg->early == 1 && full);
            bool all_fin = true;
            int n_live = 0;
            for (int i = 0; i < n; ++i) {
                const int beam = sk[i] / keep, r = sk[i] - beam * keep;
                const long at = ((long)(row0 + beam) * p.t_top + step) * keep + r;
                const int col = p.top_idx[at];
                const float lp = p.rep_lp ? p.rep_lp[(long)(row0 + beam) * keep + r] : p.top_val[at];
                // the column as a patch-local token: text ids as they are, row (row0 + beam)'s own patch j as vocab + j
                int local = col;
                bool bad = (long)col >= p.n_cols;
                if ((long)col >= p.vocab) {
                    const int j = col - (int)p.vocab - p.vrt_off[row0 + beam];
                    bad = bad || j < 0 || j >= p.vrt_off[row0 + beam + 1] - p.vrt_off[row0 + beam];
                    local = (int)p.vocab + j;
                }
                if (bad) { if (p.err) *p.err = 1; continue; }      // a column outside the row's table: reported, never followed
                const bool fin = gen_is_eos(p.gen, (long)col, p.eos) || step >= p.cfg->t_last;
                all_fin = all_fin && fin;
                if (!fin) {
                    if (n_live < K) { tok[n_live] = local; par[n_live] = beam; lps[n_live] = lp; nl[n_live] = sv[i]; feed[n_live] = col; ++n_live; }
                } else if (merge && i < K) {
                    // insert behind every entry whose score is >= the new one (old entries first at equal scores; new ones arrive in order)
                    const float sc = sv[i] / div_t;
                    if (sc == sc) {
                        int at_s = K;
                        while (at_s > 0 && !(p.st_score[row0 + at_s - 1] >= sc)) --at_s;
                        if (at_s < K) {
                            for (int c = K - 1; c > at_s; --c) {
                                p.st_score[row0 + c] = p.st_score[row0 + c - 1]; p.st_lp[row0 + c] = p.st_lp[row0 + c - 1];
                                p.st_end[row0 + c] = p.st_end[row0 + c - 1]; p.st_parent[row0 + c] = p.st_parent[row0 + c - 1];
                                p.st_tok[row0 + c] = p.st_tok[row0 + c - 1]; p.sent[row0 + c] = p.sent[row0 + c - 1];
                            }
                            p.st_score[row0 + at_s] = sc; p.st_lp[row0 + at_s] = lp; p.st_end[row0 + at_s] = step;
                            p.st_parent[row0 + at_s] = beam; p.st_tok[row0 + at_s] = local; p.sent[row0 + at_s] = 1;
                        }
                    }
                }
            }
            // 6. can a running beam still beat the worst finished hypothesis?
            full = true;
            float worst = INFINITY;
            for (int c = 0; c < K; ++c) { full = full && p.sent[row0 + c] != 0; worst = fminf(worst, p.st_score[row0 + c]); }
            if (!full) worst = -INFINITY;
            const int t_h = p.cfg->never_max ? p.cfg->t_last : step;
            const float best = nl[0] / p.len_table[t_h < p.T_max ? (t_h < 0 ? 0 : t_h) : p.T_max - 1];
            open = open && best > worst;
            // 7.
            done = !(open && !(p.cfg->early == 1 && full) && !all_fin);
            p.flags[2 * b] = open ? 1 : 0;
            p.flags[2 * b + 1] = done ? 1 : 0;
            for (int c = 0; c < K; ++c) p.live[row0 + c] = nl[c];
        }
        if (step >= 0 && step < p.T_max) {                 // the step's records; a done sample files pad rows that continue themselves
            for (int c = 0; c < K; ++c) {
                const long o = (long)step * p.B * K + row0 + c;
                p.beam_tok[o] = tok[c]; p.beam_parent[o] = par[c]; p.beam_lp[o] = lps[c];
            }
        }
        for (int c = 0; c < K; ++c) {
            const int row = row0 + c;
            p.perm[row] = par[c];
            p.cur_tok[row] = feed[c];
            if (done) p.unfinished[row] = 0;
            if (p.advance) {
                p.slot[row] += 1; p.lens[row] += 1;
                p.pos3[row] += 1; p.pos3[p.B * K + row] += 1; p.pos3[2 * p.B * K + row] += 1;
            }
        }
    }
}

__global__ void beam_step_inc_kernel(int* step) { *step += 1; }

// One block per row, before beam_step_kernel: the fold of greedy_step_kernel<LP> — the strided block → thread map, the LDS trees — then one
// thread per candidate.
__global__ __launch_bounds__(256) void beam_cand_lp_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                           const float* __restrict__ part_sum, int nblk, int R, const float* __restrict__ rows,
                                                           long ld, long n_cols, const int* __restrict__ top_idx, int t_top, int keep,
                                                           const int* __restrict__ step, float* __restrict__ out) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float ss[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = -INFINITY;
    int bidx = 0x7fffffff;
    for (int i = tid; i < nblk; i += 256) {
        const float v = part_val[(long)i * R + b];
        const int ix = part_idx[(long)i * R + b];
        if (argmax_less(best, bidx, v, ix)) { best = v; bidx = ix; }
    }
    block_argmax_lds<256>(best, bidx, sv, si);
    const float M = sv[0];
    float acc = 0.f;
    for (int i = tid; i < nblk; i += 256) {
        const float s = part_sum[(long)i * R + b];
        const float v = part_val[(long)i * R + b];
        acc += (s == 0.f || v == -INFINITY) ? 0.f : s * __builtin_amdgcn_exp2f((v - M) * 1.44269504088896341f);
    }
    block_sum_lds<256>(acc, ss);
    const int t = *step;
    if (tid < keep) {
        float lp = -INFINITY;
        if (t >= 0 && t < t_top && M != -INFINITY) {
            const int col = top_idx[((long)b * t_top + t) * keep + tid];
            if (col >= 0 && (long)col < n_cols) {
                const float v = rows[(long)b * ld + col];
                lp = v == -INFINITY ? -INFINITY : (v - M) - logf(ss[0]);
            }
        }
        out[(long)b * keep + tid] = lp;
    }
}

extern "C" int padt_beam_cand_lp(void* stream, const void* part_val, const int* part_idx, const void* part_sum, long nblk, long rows,
                                 const void* rows_f32, long ld, long n_cols, const int* top_idx, long t_top, long keep, const int* step,
                                 void* out) {
    if (rows <= 0) return 0;
    if (!part_val || !part_idx || !part_sum || !rows_f32 || !top_idx || !step || !out || nblk <= 0 || nblk > 0x7fffffffL || rows > 0x7fffffffL ||
        keep < 1 || keep > BEAM_MAX_KEEP || t_top <= 0 || t_top > 0x7fffffffL || n_cols <= 0 || n_cols > ld) {
        padt_set_error("padt_beam_cand_lp: the head's partials, the score rows, the candidates [rows][t_top][keep <= 32] and the output are required"); return -1;
    }
    hipLaunchKernelGGL(beam_cand_lp_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const float*)part_val, part_idx,
                       (const float*)part_sum, (int)nblk, (int)rows, (const float*)rows_f32, ld, n_cols, top_idx, (int)t_top, (int)keep, step,
                       (float*)out);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_beam_step(void* stream, const int* top_idx, const void* top_val, long t_top, long keep, long batch, long K, long D,
                              long t_max, const int* beam_cfg, const void* len_table, const void* gen_cfg, int eos, int pad, long vocab,
                              long n_cols, const int* vrt_off, void* live, void* st_score, void* st_lp, int* st_end, int* st_parent,
                              int* st_tok, int* sent, int* flags, int* beam_tok, int* beam_parent, void* beam_lp, int* perm, long* cur_tok,
                              int* unfinished, int* step, int* slot, int* lens, int* pos3, const void* hidden, void* hidden_buf, int advance,
                              int* err, const void* rep_lp) {
    if (batch <= 0) return 0;
    if (K < 1 || K > BEAM_MAX_K || keep < 1 || keep > BEAM_MAX_KEEP || K * keep > 256) {
        padt_set_error("padt_beam_step: 1 <= K <= 8 and 1 <= keep <= 32 are required"); return -1;
    }
    if (D & 7) { padt_set_error("padt_beam_step: D % 8 == 0 required"); return -1; }
    if (batch * K > 0x7fffffffL || t_max <= 0 || t_max > 0x7fffffffL || t_top <= 0 || t_top > 0x7fffffffL || n_cols <= 0 || n_cols > 0x7fffffffL ||
        vocab < 0 || vocab > n_cols) {
        padt_set_error("padt_beam_step: bad sizes"); return -1;
    }
    if (!top_idx || !top_val || !beam_cfg || !len_table || !vrt_off || !live || !st_score || !st_lp || !st_end || !st_parent || !st_tok || !sent ||
        !flags || !beam_tok || !beam_parent || !beam_lp || !perm || !cur_tok || !unfinished || !step || !slot || !lens || !pos3 || !hidden ||
        !hidden_buf) {
        padt_set_error("padt_beam_step: a required buffer is null"); return -1;
    }
    BeamStepArgs a{top_idx, (const float*)top_val, (const float*)rep_lp, (int)t_top, (int)keep, (int)batch, (int)K, (int)D, (int)t_max, (const BeamCfg*)beam_cfg,
                   (const float*)len_table, (const GenCfg*)gen_cfg, eos, pad, vocab, n_cols, vrt_off, (float*)live, (float*)st_score, (float*)st_lp,
                   st_end, st_parent, st_tok, sent, flags, beam_tok, beam_parent, (float*)beam_lp, perm, cur_tok, unfinished, step, slot, lens, pos3,
                   (const x16_t*)hidden, (x16_t*)hidden_buf, advance, err};
    hipLaunchKernelGGL(beam_step_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(beam_step_inc_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step);
    PADT_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The KV caches follow the beams.  After beam_step_kernel: row c of a sample continues the hypothesis of row perm[c], so the generated slots
// [p0, slot) of c must hold what perm[c]'s held.  The packed images are moved by their own tiles, whose inner order the kernel never needs:
//   K image   [Hkv][S / 16][head_dim * 16 values]: a 16-slot tile is head_dim * 32 contiguous bytes
//   V^T image [Hkv][head_dim / 16][S / 32][512 values]: a 32-slot tile is head_dim / 16 segments of 1 KiB, s_max * 32 bytes apart
// Every thread owns 16-byte word offsets of one tile: it loads that word from all K rows of the sample into registers, then stores to every
// child whose parent is another row.  No other thread touches that offset in any row of the sample, so the permutation is in place: no
// barrier, no scratch, no atomics.  Grid x covers the tiles a call of t_max steps can reach from p0; blocks past the live range exit.
struct BeamReorderArgs {
    void* const* images;           // [n_layers][2] device pointers: K image, V^T image
    const int* perm; const int* p0; const int* slot;       // [B * K]: parent, first generated slot, slots in use (after the step's advance)
    int K, Hkv, hd, s_max;
};

__global__ __launch_bounds__(256) void beam_reorder_kernel(BeamReorderArgs p) {
    const int K = p.K, b = blockIdx.y / p.Hkv, head = blockIdx.y - b * p.Hkv;
    const int layer = blockIdx.z >> 1, is_v = blockIdx.z & 1;
    const int row0 = b * K;
    int par[BEAM_MAX_K];
    bool ident = true;
#pragma unroll
    for (int c = 0; c < BEAM_MAX_K; ++c) {
        int q = c < K ? p.perm[row0 + c] : c;
        if (q < 0 || q >= K) q = c;                        // never a row outside the sample
        par[c] = q;
        ident = ident && q == c;
    }
    if (ident) return;                                     // a done sample, or every beam continues itself
    const int lo = p.p0[row0];
    int hi = p.slot[row0];
    if (hi > p.s_max) hi = p.s_max;
    if (lo < 0 || lo >= hi) return;
    const int tile_slots = is_v ? 32 : 16;
    const int tile = lo / tile_slots + blockIdx.x;
    if ((long)tile * tile_slots >= hi) return;
    char* base = (char*)p.images[2 * layer + is_v];
    const long row_bytes = (long)p.Hkv * p.s_max * p.hd * 2;
    const int words = p.hd * tile_slots * 2 / 16;          // 16-byte words of the tile: 256 (K), 512 (V^T) at head_dim 128
    for (int w = threadIdx.x; w < words; w += 256) {
        long off;
        if (!is_v) off = ((long)head * (p.s_max / 16) + tile) * (p.hd * 32L) + (long)w * 16;
        else {
            const int seg = w >> 6, in = w & 63;           // 64 words per 1 KiB segment
            off = (((long)head * (p.hd / 16) + seg) * (p.s_max / 32) + tile) * 1024L + (long)in * 16;
        }
        u32x4 reg[BEAM_MAX_K];
#pragma unroll
        for (int c = 0; c < BEAM_MAX_K; ++c)
            if (c < K) reg[c] = *reinterpret_cast<const u32x4*>(base + (long)(row0 + c) * row_bytes + off);
#pragma unroll
        for (int c = 0; c < BEAM_MAX_K; ++c) {
            if (c < K && par[c] != c) {
                u32x4 v = reg[0];
#pragma unroll
                for (int j = 1; j < BEAM_MAX_K; ++j) v = (j < K && par[c] == j) ? reg[j] : v;
                *reinterpret_cast<u32x4*>(base + (long)(row0 + c) * row_bytes + off) = v;
            }
        }
    }
}

extern "C" int padt_beam_reorder_kv(void* stream, const void* images, long n_layers, const int* perm, const int* p0, const int* slot, long batch,
                                    long K, long n_kv_heads, long head_dim, long s_max, long t_max) {
    if (batch <= 0 || n_layers <= 0) return 0;
    if (K < 1 || K > BEAM_MAX_K) { padt_set_error("padt_beam_reorder_kv: 1 <= K <= 8 is required"); return -1; }
    if (head_dim != 128 || s_max <= 0 || (s_max & 31)) {
        padt_set_error("padt_beam_reorder_kv: the packed cache images (head_dim 128, s_max % 32 == 0) are required"); return -1;
    }
    if (!images || !perm || !p0 || !slot || t_max <= 0 || n_kv_heads <= 0 || batch * n_kv_heads > 65535 || 2 * n_layers > 65535 ||
        batch * K > 0x7fffffffL || batch * K * n_kv_heads * s_max * head_dim * 2 > 0x7fffffffffffL) {
        padt_set_error("padt_beam_reorder_kv: bad arguments"); return -1;
    }
    BeamReorderArgs a{(void* const*)images, perm, p0, slot, (int)K, (int)n_kv_heads, (int)head_dim, (int)s_max};
    const unsigned tiles = (unsigned)((t_max + 15) / 16 + 1);          // 16-slot tiles a range of t_max slots can intersect from any p0
    hipLaunchKernelGGL(beam_reorder_kernel, dim3(tiles, (unsigned)(batch * n_kv_heads), (unsigned)(2 * n_layers)), dim3(256), 0,
                       (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// generation.beam_backtrace on the device: block i = sample b's r-th best store entry (i = b * n_best + r).  One thread walks the parents back
// and writes the hypothesis's tokens (pad behind its end; a patch-local VRT id vocab + j becomes vocab + out_off[i] + j, the returned row's
// own range), log-probs (0 behind the end), score, length and src_row[i][t] = the beam whose hidden row produced token t; then the block
// gathers those rows from hidden_buf with 16-byte copies into out_hidden [T_max][B * n_best][D] (rows behind the end are not written).
struct BeamFinalArgs {
    const float* st_score; const float* st_lp; const int* st_end; const int* st_parent; const int* st_tok;     // [B][K]
    const int* beam_tok; const int* beam_parent; const float* beam_lp;      // [T_max][B * K]
    int B, K, n_best, D, T_max, pad; long vocab; const int* out_off;       // [B * n_best]
    const x16_t* hidden_buf; x16_t* out_hidden;
    long* tokens; float* logprobs; float* scores; int* lengths; int* src_row;      // [B * n_best][T_max] x2, [B * n_best] x2, [B * n_best][T_max]
};

__global__ __launch_bounds__(256) void beam_finalize_kernel(BeamFinalArgs p) {
    __shared__ int s_len;
    const int i = blockIdx.x, b = i / p.n_best, r = i - b * p.n_best, tid = threadIdx.x;
    const int rows = p.B * p.K, e = b * p.K + r;
    if (tid == 0) {
        int end = p.st_end[e];
        if (end >= p.T_max) end = -1;
        int beam = p.st_parent[e];
        if (end >= 0 && (beam < 0 || beam >= p.K)) end = -1;
        long* tk = p.tokens + (long)i * p.T_max;
        float* lp = p.logprobs + (long)i * p.T_max;
        int* sr = p.src_row + (long)i * p.T_max;
        for (int t = end + 1; t < p.T_max; ++t) { tk[t] = p.pad; lp[t] = 0.f; sr[t] = -1; }
        auto renum = [&](int tok) { return (long)tok >= p.vocab ? (long)tok + p.out_off[i] : (long)tok; };
        if (end >= 0) {
            tk[end] = renum(p.st_tok[e]); lp[end] = p.st_lp[e]; sr[end] = beam;
            for (int t = end - 1; t >= 0; --t) {
                const long o = (long)t * rows + b * p.K + beam;
                tk[t] = renum(p.beam_tok[o]); lp[t] = p.beam_lp[o];
                int q = p.beam_parent[o];
                if (q < 0 || q >= p.K) q = beam;           // never a row outside the sample
                beam = q;
                sr[t] = beam;
            }
        }
        p.scores[i] = end >= 0 ? p.st_score[e] : -INFINITY;
        p.lengths[i] = end + 1;
        s_len = end + 1;
    }
    __syncthreads();                                        // src_row's global writes of thread 0 are visible to the block behind the barrier
    const int n = s_len, per_row = p.D / 8;
    const int* sr = p.src_row + (long)i * p.T_max;
    for (long w = tid; w < (long)n * per_row; w += 256) {
        const int t = (int)(w / per_row), c = (int)(w - (long)t * per_row) * 8;
        *reinterpret_cast<u32x4*>(p.out_hidden + ((long)t * p.B * p.n_best + i) * p.D + c) =
            *reinterpret_cast<const u32x4*>(p.hidden_buf + ((long)t * rows + b * p.K + sr[t]) * p.D + c);
    }
}

extern "C" int padt_beam_finalize(void* stream, const void* st_score, const void* st_lp, const int* st_end, const int* st_parent,
                                  const int* st_tok, const int* beam_tok, const int* beam_parent, const void* beam_lp, long batch, long K,
                                  long n_best, long D, long t_max, int pad, long vocab, const int* out_off, const void* hidden_buf,
                                  void* out_hidden, long* tokens, void* logprobs, void* scores, int* lengths, int* src_row) {
    if (batch <= 0) return 0;
    if (K < 1 || K > BEAM_MAX_K || n_best < 1 || n_best > K) { padt_set_error("padt_beam_finalize: 1 <= n_best <= K <= 8 is required"); return -1; }
    if (D & 7) { padt_set_error("padt_beam_finalize: D % 8 == 0 required"); return -1; }
    if (t_max <= 0 || t_max > 0x7fffffffL || batch * K > 0x7fffffffL) { padt_set_error("padt_beam_finalize: bad sizes"); return -1; }
    if (!st_score || !st_lp || !st_end || !st_parent || !st_tok || !beam_tok || !beam_parent || !beam_lp || !out_off || !hidden_buf || !out_hidden ||
        !tokens || !logprobs || !scores || !lengths || !src_row) {
        padt_set_error("padt_beam_finalize: a required buffer is null"); return -1;
    }
    BeamFinalArgs a{(const float*)st_score, (const float*)st_lp, st_end, st_parent, st_tok, beam_tok, beam_parent, (const float*)beam_lp, (int)batch,
                    (int)K, (int)n_best, (int)D, (int)t_max, pad, vocab, out_off, (const x16_t*)hidden_buf, (x16_t*)out_hidden, tokens,
                    (float*)logprobs, (float*)scores, lengths, src_row};
    hipLaunchKernelGGL(beam_finalize_kernel, dim3((unsigned)(batch * n_best)), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}

}  // namespace PADT_NS
