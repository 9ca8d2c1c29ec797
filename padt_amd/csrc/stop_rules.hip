// generate(stop_sequences=, min_tokens=, max_tokens=): how a row ENDS, decided on the device inside the decode step.  Type-independent:
// compiled once.  Two kernels around the unchanged head and bookkeeping kernels; what they record is read back by padt_collect_summary_stop
// (decode_step.hip).
//
// stop_ban_kernel (before the head): min_tokens as a pure ban — HF's MinNewTokensLengthLogitsProcessor(prompt_len, n, eos_ids).  One block
// per row writes ban_out[row] from scratch: the incoming bitmap of padt_gen_rules / padt_token_automaton when there is one, else zeros;
// while *step < min_tokens[row] the bits of the config EOS id and of gen->eos[0..3] are added.  An id outside [0, n_cols) sets nothing.
//
// stop_match_kernel (after padt_greedy_step and its step-counter bump): with n = *step tokens in the row, for every row without a recorded
// finish (finish_reason[row] == 0), in this order:
//   1. tokens[row][n - 1] is an EOS id                                                  → reason 1 (eos)
//   2. n >= min_tokens[row] and sequence i's m ids equal tokens[row][n - m .. n), m <= n → reason 2 (stop), the lowest such i
//   3. n >= max_tokens[row]                                                             → reason 3 (length)
// A finish clears unfinished[row] and writes finish_step[row] = n - 1, finish_reason[row] and stop_index[row] (i, or -1).  A row with a
// recorded finish is never touched again: its pad tokens cannot complete a sequence.  Nothing happens unless 1 <= n <= ld_tokens.
// Packed sequences (DEVICE memory, nothing baked into a captured graph; packed by generation.stop_table):
//   [0] magic  [1] n sequences <= 32  [2 .. 34) their lengths (1 .. 32)  [34 + 32 i ..) sequence i's ids.  A table that is not what the
//   packer writes makes the kernel return before its first write; a length outside 1 .. 32 never matches.
#include "gen_cfg.h"

namespace {

constexpr int SR_MAGIC = 0x53523031;         // ops.STOP_RULES_MAGIC
constexpr int SR_MAX_SEQS = 32;              // ops.STOP_RULES_MAX_SEQS
constexpr int SR_MAX_LEN = 32;               // ops.STOP_RULES_MAX_LEN
constexpr int SR_INTS = 2 + SR_MAX_SEQS + SR_MAX_SEQS * SR_MAX_LEN;      // ops.STOP_RULES_INTS
constexpr int SR_EOS = 1, SR_STOP = 2, SR_LENGTH = 3;

struct StopBanArgs {
    const GenCfg* gen; int eos; const int* step; const int* min_tokens; const unsigned* ban_in; unsigned* ban_out; long ban_words; int n_cols;
};

__global__ __launch_bounds__(256) void stop_ban_kernel(StopBanArgs p) {
    const int row = blockIdx.x, tid = threadIdx.x;
    unsigned* out = p.ban_out + (long)row * p.ban_words;
    const unsigned* in = p.ban_in ? p.ban_in + (long)row * p.ban_words : nullptr;
    for (long w = tid; w < p.ban_words; w += 256) out[w] = in ? in[w] : 0u;
    __syncthreads();
    if (tid < 5 && *p.step < p.min_tokens[row]) {
        const int e = tid == 4 ? p.eos : p.gen->eos[tid];
        if (e >= 0 && e < p.n_cols) atomicOr(&out[e >> 5], 1u << (e & 31));
    }
}

struct StopMatchArgs {
    const int* table; const GenCfg* gen; int eos; const long* tokens; long ld_tok; const int* step; const int* min_tokens;
    const int* max_tokens; int* unfinished; int* finish_step; int* finish_reason; int* stop_index;
};

__global__ __launch_bounds__(64) void stop_match_kernel(StopMatchArgs p) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int n = *p.step;
    if (n < 1 || (long)n > p.ld_tok) return;
    if (p.finish_reason[row] != 0) return;
    const int* tb = p.table;
    int n_seq = tb[1];
    if (tb[0] != SR_MAGIC || n_seq < 0 || n_seq > SR_MAX_SEQS) return;                  // not a table generation.stop_table packed
    const long* trow = p.tokens + (long)row * p.ld_tok;
    __shared__ int best;
    if (tid == 0) best = 0x7fffffff;
    __syncthreads();
    if (tid < n_seq && n >= p.min_tokens[row]) {
        const int m = tb[2 + tid];
        if (m >= 1 && m <= SR_MAX_LEN && m <= n) {
            const int* ids = tb + 2 + SR_MAX_SEQS + tid * SR_MAX_LEN;
            bool eq = true;
            for (int k = 0; k < m && eq; ++k) eq = trow[n - m + k] == (long)ids[k];
            if (eq) atomicMin(&best, tid);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int reason = 0, index = -1;
        if (gen_is_eos(p.gen, trow[n - 1], p.eos)) reason = SR_EOS;
        else if (best < SR_MAX_SEQS) { reason = SR_STOP; index = best; }
        else if (n >= p.max_tokens[row]) reason = SR_LENGTH;
        if (reason != 0) {
            p.unfinished[row] = 0;
            p.finish_step[row] = n - 1;
            p.stop_index[row] = index;
            p.finish_reason[row] = reason;
        }
    }
}

}  // namespace

extern "C" int padt_stop_ban(void* stream, const void* gen_cfg, int eos, const int* step, const int* min_tokens, const void* ban_in,
                             void* ban_out, long ban_words, long n_cols, long batch) {
    if (batch <= 0) return 0;
    if (!gen_cfg || !step || !min_tokens || !ban_out || ban_words <= 0) {
        padt_set_error("padt_stop_ban: generation config, step counter, min_tokens and the output bitmap are required"); return -1;
    }
    if (n_cols <= 0 || n_cols > ban_words * 32 || n_cols > 0x7fffffffL) { padt_set_error("padt_stop_ban: 0 < n_cols <= 32 * ban_words is required"); return -1; }
    if (ban_in == ban_out) { padt_set_error("padt_stop_ban: the incoming bitmap and the output bitmap must be two buffers"); return -1; }
    StopBanArgs a{(const GenCfg*)gen_cfg, eos, step, min_tokens, (const unsigned*)ban_in, (unsigned*)ban_out, ban_words, (int)n_cols};
    hipLaunchKernelGGL(stop_ban_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_stop_match(void* stream, const int* table, long table_ints, const void* gen_cfg, int eos, const long* tokens,
                               long ld_tokens, const int* step, const int* min_tokens, const int* max_tokens, int* unfinished,
                               int* finish_step, int* finish_reason, int* stop_index, long batch) {
    if (batch <= 0) return 0;
    if (!table || !gen_cfg || !tokens || !step || !min_tokens || !max_tokens || !unfinished || !finish_step || !finish_reason || !stop_index) {
        padt_set_error("padt_stop_match: sequence table, generation config, token buffer, step counter, min_tokens, max_tokens, stop state and "
                       "the three finish arrays are required"); return -1;
    }
    if (table_ints < SR_INTS) { padt_set_error("padt_stop_match: the packed sequence table holds 2 + 32 + 32 * 32 ints"); return -1; }
    if (ld_tokens <= 0 || ld_tokens > 0x7fffffffL) { padt_set_error("padt_stop_match: 0 < ld_tokens < 2^31 is required"); return -1; }
    StopMatchArgs a{table, (const GenCfg*)gen_cfg, eos, tokens, ld_tokens, step, min_tokens, max_tokens, unfinished, finish_step,
                    finish_reason, stop_index};
    hipLaunchKernelGGL(stop_match_kernel, dim3((unsigned)batch), dim3(64), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}
