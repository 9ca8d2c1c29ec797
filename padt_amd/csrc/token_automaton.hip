// generate(token_automaton=A): which table columns a row may emit next, given what it emitted so far, as the step's ban bitmap for
// padt_vrt_head_ban — derived from the state of a token automaton instead of from n-grams (gen_rules_kernel).  Type-independent: compiled once.
//
// Packed automaton (DEVICE memory, nothing baked into a captured graph; packed by ops.token_automaton_tensor, checked by the header below):
//   [0] magic  [1] S states  [2] E edges  [3] start state   [4 .. 4 + S] edge offsets off[0 .. S] (off[s] .. off[s + 1] are state s' edges)
//   [5 + S ..) E edges as (key, next state) pairs, sorted by key within a state: the three classes first (EOS = -3, TEXT = -2, VRT = -1),
//   then the explicit text ids ascending.  S <= 4096, E <= 32768.
// A token matches an explicit id before a class.  VRT: the row's own patch columns vocab + vrt_off[row] .. vocab + vrt_off[row + 1] - 1;
// EOS: one of the GenCfg EOS ids; TEXT: a text id that is none of them.
// Per row a (state, valid_for_step) pair: at step t a state valid for t is kept (a repeated launch changes nothing), one valid for t - 1
// advances by tokens[row][t - 1] (binary search over the explicit edges, then the class tests), anything else is rebuilt from the start
// state over tokens[row][0 .. t).  A token without an edge takes the row to the off-automaton state (-1), which it never leaves.
// Bitmap of an unfinished row: every column of [0, n_cols) banned except the keys of the state's edges — the two range classes through
// word-wise stores with exact partial first / last words, the EOS ids carved out of the TEXT range unless the state has an EOS edge,
// explicit ids and EOS ids through single-bit atomics.  An empty allowed set (the off-automaton state, a state without edges, a VRT-only
// state of a row without patches) allows the EOS ids and nothing else.  A finished row keeps its state and bans nothing of its own.
// rules_ban (optional): padt_gen_rules' bitmap of the same step, OR-ed in at the end — the head reads ONE bitmap, the union; the row is
// rebuilt from scratch by every launch, so no bit outlives its step.  Bits past n_cols in the last word are zero (the rules' bits aside).
// A table that is not what the packer writes makes the kernel return before its first write; a state whose offsets or successor leave
// the table counts as off-automaton.  Every store lands in the row's own ban_words words or its own state pair.
#include "gen_cfg.h"

namespace {

constexpr int TA_MAGIC = 0x54413031;         // ops.TOKEN_AUTOMATON_MAGIC
constexpr int TA_MAX_STATES = 4096;          // ops.TOKEN_AUTOMATON_MAX_STATES
constexpr int TA_MAX_EDGES = 32768;          // ops.TOKEN_AUTOMATON_MAX_EDGES
constexpr int TA_KEY_EOS = -3, TA_KEY_TEXT = -2, TA_KEY_VRT = -1;
constexpr int TA_OFF = -1;                   // the off-automaton state

struct AutomatonArgs {
    const int* table; long table_ints; const GenCfg* gen; const int* vrt_off; const long* tokens; long ld_tok; const int* step;
    const int* unfinished; int* state; unsigned* ban; long ban_words; const unsigned* rules_ban; int n_cols; int vocab;
};

struct Tab { const int* off; const int* edge; int S, E; };

// what the state's edge list says: the successors of the three classes (-2: no such edge) and the explicit edges [xlo, xhi)
struct StateInfo { int nx_eos, nx_text, nx_vrt, xlo, xhi; bool ok; };

__device__ StateInfo state_info(const Tab& T, int s) {
    StateInfo r{-2, -2, -2, 0, 0, false};
    if (s < 0 || s >= T.S) return r;
    const int lo = T.off[s], hi = T.off[s + 1];
    if (lo < 0 || hi < lo || hi > T.E) return r;
    int e = lo;
    for (; e < hi; ++e) {
        const int k = T.edge[2 * e];
        if (k >= 0) break;
        if (k == TA_KEY_EOS) r.nx_eos = T.edge[2 * e + 1];
        else if (k == TA_KEY_TEXT) r.nx_text = T.edge[2 * e + 1];
        else if (k == TA_KEY_VRT) r.nx_vrt = T.edge[2 * e + 1];
    }
    r.xlo = e; r.xhi = hi; r.ok = true;
    return r;
}

__device__ int next_state(const Tab& T, int s, long tok, long v_lo, long v_hi, int vocab, const GenCfg* g) {
    const StateInfo si = state_info(T, s);
    if (!si.ok) return TA_OFF;
    int nx = -2;
    if (tok >= 0 && tok < (long)vocab) {
        int lo = si.xlo, hi = si.xhi;                        // the first explicit edge whose key is >= tok
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((long)T.edge[2 * mid] < tok) lo = mid + 1; else hi = mid;
        }
        if (lo < si.xhi && (long)T.edge[2 * lo] == tok) nx = T.edge[2 * lo + 1];
    }
    if (nx == -2) {
        if (tok >= v_lo && tok < v_hi) nx = si.nx_vrt;
        // the listed ids alone, not gen_is_eos: the EOS class is what the bitmap below carves out of TEXT, and that is the GenCfg list
        else if (tok >= 0 && tok < (long)vocab) nx = gen_eos_listed(g, tok) ? si.nx_eos : si.nx_text;
    }
    return (nx >= 0 && nx < T.S) ? nx : TA_OFF;
}

// the bits of word w that lie in columns [a, b)
__device__ __forceinline__ unsigned range_bits(long w, long a, long b) {
    const long base = w * 32;
    const long lo = a > base ? a - base : 0, hi = (b - base) < 32 ? (b - base) : 32;
    if (hi <= lo) return 0u;
    const unsigned upto_hi = hi == 32 ? 0xffffffffu : ((1u << hi) - 1u);
    return upto_hi & ~((1u << lo) - 1u);
}

__global__ __launch_bounds__(256) void token_automaton_kernel(AutomatonArgs p) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int* tb = p.table;
    const int S = tb[1], E = tb[2], start = tb[3];
    if (tb[0] != TA_MAGIC || S < 1 || S > TA_MAX_STATES || E < 0 || E > TA_MAX_EDGES || start < 0 || start >= S
        || 5L + S + 2L * E > p.table_ints) return;                       // not a table ops.token_automaton_tensor packed
    const Tab T{tb + 4, tb + 5 + S, S, E};
    int t = *p.step;
    t = t < 0 ? 0 : (t > (int)p.ld_tok ? (int)p.ld_tok : t);
    const bool live = p.unfinished[row] != 0;
    // the row's own patch columns, clamped into [vocab, n_cols)
    long v_lo = (long)p.vocab + p.vrt_off[row], v_hi = (long)p.vocab + p.vrt_off[row + 1];
    v_lo = v_lo < p.vocab ? p.vocab : (v_lo > p.n_cols ? p.n_cols : v_lo);
    v_hi = v_hi < v_lo ? v_lo : (v_hi > p.n_cols ? p.n_cols : v_hi);

    __shared__ int sh[5];                                                // text, vrt, eos class, explicit edges [xlo, xhi)
    if (tid == 0) {
        int s = p.state[2 * row];
        if (live) {
            const int valid = p.state[2 * row + 1];
            const long* trow = p.tokens + (long)row * p.ld_tok;
            if (valid != t) {
                if (t >= 1 && valid == t - 1) s = next_state(T, s, trow[t - 1], v_lo, v_hi, p.vocab, p.gen);
                else {
                    s = start;
                    for (int i = 0; i < t; ++i) s = next_state(T, s, trow[i], v_lo, v_hi, p.vocab, p.gen);
                }
                p.state[2 * row] = s;
                p.state[2 * row + 1] = t;
            }
        }
        const StateInfo si = state_info(T, s);
        bool text = si.ok && si.nx_text != -2, vrt = si.ok && si.nx_vrt != -2 && v_hi > v_lo, eosc = si.ok && si.nx_eos != -2;
        int xlo = si.ok ? si.xlo : 0, xhi = si.ok ? si.xhi : 0;
        if (!text && !vrt && !eosc && xhi <= xlo) eosc = true;           // empty allowed set: the EOS ids and nothing else
        sh[0] = text; sh[1] = vrt; sh[2] = eosc; sh[3] = xlo; sh[4] = xhi;
    }
    __syncthreads();
    const bool text = sh[0] != 0, vrt = sh[1] != 0, eosc = sh[2] != 0;
    const int xlo = sh[3], xhi = sh[4];
    unsigned* out = p.ban + (long)row * p.ban_words;
    for (long w = tid; w < p.ban_words; w += 256) {
        unsigned m = 0u;
        if (live) {
            m = range_bits(w, 0, p.n_cols);
            if (text) m &= ~range_bits(w, 0, p.vocab);
            if (vrt) m &= ~range_bits(w, v_lo, v_hi);
        }
        out[w] = m;
    }
    __syncthreads();
    if (live) {
        if (text && !eosc && tid < 4) {                                  // TEXT is every text id that is no EOS id
            const int e = p.gen->eos[tid];
            if (e >= 0 && e < p.vocab && e < p.n_cols) atomicOr(&out[e >> 5], 1u << (e & 31));
        }
        __syncthreads();
        for (int i = xlo + tid; i < xhi; i += 256) {                     // explicit ids win over the carve-out
            const int id = T.edge[2 * i];
            if (id >= 0 && id < p.vocab && id < p.n_cols) atomicAnd(&out[id >> 5], ~(1u << (id & 31)));
        }
        if (eosc && tid < 4) {
            const int e = p.gen->eos[tid];
            if (e >= 0 && e < p.n_cols) atomicAnd(&out[e >> 5], ~(1u << (e & 31)));
        }
    }
    if (p.rules_ban) {
        __syncthreads();
        const unsigned* rb = p.rules_ban + (long)row * p.ban_words;
        for (long w = tid; w < p.ban_words; w += 256) out[w] |= rb[w];
    }
}

}  // namespace

extern "C" int padt_token_automaton(void* stream, const int* table, long table_ints, const void* gen_cfg, const int* vrt_off,
                                    const long* tokens, long ld_tokens, const int* step, const int* unfinished, int* state, void* ban,
                                    long ban_words, const void* rules_ban, long n_cols, long vocab, long batch) {
    if (batch <= 0) return 0;
    if (!table || !gen_cfg || !vrt_off || !tokens || !step || !unfinished || !state || !ban || table_ints < 5 || ld_tokens <= 0
        || ld_tokens > 0x7fffffffL) {
        padt_set_error("padt_token_automaton: automaton table, generation config, patch offsets, token buffer, step counter, stop state, "
                       "state pairs and ban bitmap are required");
        return -1;
    }
    if (vocab <= 0 || n_cols < vocab || n_cols > ban_words * 32 || n_cols > 0x7fffffffL) {
        padt_set_error("padt_token_automaton: 0 < vocab <= n_cols <= 32 * ban_words is required");
        return -1;
    }
    if (rules_ban == ban) { padt_set_error("padt_token_automaton: the rules' bitmap and the output bitmap must be two buffers"); return -1; }
    AutomatonArgs a{table, table_ints, (const GenCfg*)gen_cfg, vrt_off, tokens, ld_tokens, step, unfinished, state, (unsigned*)ban,
                    ban_words, (const unsigned*)rules_ban, (int)n_cols, (int)vocab};
    hipLaunchKernelGGL(token_automaton_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}
