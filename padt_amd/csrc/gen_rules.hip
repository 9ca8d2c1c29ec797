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
//   of the history).  Finished rows are treated like live ones, as in HF.  Type-independent: compiled once.
#include "gen_cfg.h"

namespace PADT_NS {

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
    PADT_CHECK_LAUNCH();
    return 0;
}

}  // namespace PADT_NS
