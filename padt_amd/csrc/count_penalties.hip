// generate(frequency_penalty=, presence_penalty=, patch_suppression=): the per-row COUNTS the head's edit reads (vrt_head.hip, the COUNTS
// kernels), kept on the device inside the decode step.  Type-independent: compiled once.  One kernel behind the bookkeeping kernel
// (padt_greedy_step / padt_forced_step and its step-counter bump), in front of padt_stop_match.
//
// count_update_kernel: with n = *step tokens in row b and tok = tokens[b][n - 1], for every row whose unfinished[b] the bookkeeping kernel left
// set (a row it finished in this very step — an EOS id — or earlier writes nothing: nothing is selected from such a row again, and its pad
// tokens are not generated tokens):
//   1. tok a text id (0 <= tok < vocab): cnt_text[b][tok] += 1;  tok one of the row's own patch columns (vrt_off[b] <= tok - vocab <
//      vrt_off[b + 1]): cnt_patch[tok - vocab] += 1.  A VRT id outside the row's own range counts nowhere.
//   2. tok is not a VRT id, tokens[b][n - 2] is one, and radius[b] >= 0: the run of VRT tokens that ends at n - 2 has just been COMPLETED.
//      Walking back over it, every token on one of the row's own patches (y, x) of the row-major merged grid (hp, wp) = grid[b] adds 1 to
//      near[] on the window max(|y' - y|, |x' - x|) <= radius[b], clipped at the grid's border — one token after the other with a block
//      barrier between them, thread i of the first (2 r + 1)^2 owning one cell of the window, so no two threads ever touch one element.
// The tables are uint16 and SATURATE at 65535 (half of what int32 would make the head read; a row cannot emit 65535 tokens before any
// session's token buffer ends, so saturation is a guard and not a behaviour).  Nothing is written unless 1 <= n <= ld_tokens, and nothing to
// near[] unless 0 <= radius[b] <= 7 and hp * wp is the row's patch count (the host checks both at launch; the kernel does not trust them).
#include "common.h"

namespace {

constexpr int CP_MAX_RADIUS = 7;             // ops.COUNT_MAX_RADIUS: (2 * 7 + 1)^2 = 225 window cells <= the block's 256 threads
constexpr unsigned CP_SAT = 65535u;

struct CountArgs {
    const long* tokens; long ld_tok; const int* step; const int* unfinished; const int* vrt_off; const int* grid; const int* radius;
    unsigned short* cnt_text; long ld_cnt; int V; unsigned short* cnt_patch; unsigned short* near; int NP;
};

__device__ __forceinline__ void sat_inc(unsigned short* p) {
    const unsigned v = *p;
    if (v < CP_SAT) *p = (unsigned short)(v + 1u);
}

__global__ __launch_bounds__(256) void count_update_kernel(CountArgs p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = *p.step;
    if (n < 1 || (long)n > p.ld_tok) return;
    if (p.unfinished[b] == 0) return;
    const long* trow = p.tokens + (long)b * p.ld_tok;
    const long tok = trow[n - 1];
    int lo = p.vrt_off[b], hi = p.vrt_off[b + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > p.NP ? p.NP : hi;
    if (tid == 0) {
        if (tok >= 0 && tok < (long)p.V) sat_inc(p.cnt_text + (long)b * p.ld_cnt + tok);
        else if (tok >= (long)p.V && tok - p.V >= (long)lo && tok - p.V < (long)hi) sat_inc(p.cnt_patch + (tok - p.V));
    }
    const int r = p.radius[b];
    if (tok >= (long)p.V || n < 2 || r < 0 || r > CP_MAX_RADIUS) return;        // the run, if any, is still open — or suppression is off
    const int hp = p.grid[2 * b], wp = p.grid[2 * b + 1];
    if (hp <= 0 || wp <= 0 || (long)hp * wp != (long)(hi - lo)) return;
    const int w = 2 * r + 1;
    const int dy = tid / w - r, dx = tid % w - r;
    for (int k = n - 2; k >= 0; --k) {                                           // uniform: every thread reads the same tokens
        const long t = trow[k];
        if (t < (long)p.V) break;
        const long jv = t - p.V;
        if (jv >= (long)lo && jv < (long)hi && tid < w * w) {
            const int j = (int)jv - lo;
            const int yy = j / wp + dy, xx = j % wp + dx;
            if (yy >= 0 && yy < hp && xx >= 0 && xx < wp) sat_inc(p.near + lo + yy * wp + xx);
        }
        __syncthreads();                                                         // the next token's windows may overlap this one's
    }
}

}  // namespace

extern "C" int padt_count_update(void* stream, const long* tokens, long ld_tokens, const int* step, const int* unfinished, const int* vrt_off,
                                 const int* grid, const int* radius, void* cnt_text, long ld_cnt, long vocab, void* cnt_patch, void* near,
                                 long n_proto, long batch) {
    if (batch <= 0) return 0;
    if (!tokens || !step || !unfinished || !vrt_off || !grid || !radius || !cnt_text || !cnt_patch || !near) {
        padt_set_error("padt_count_update: token buffer, step counter, stop state, vrt_off, the grids, the radii and the three count tables are "
                       "required"); return -1;
    }
    if (ld_tokens <= 0 || ld_tokens > 0x7fffffffL) { padt_set_error("padt_count_update: 0 < ld_tokens < 2^31 is required"); return -1; }
    if (vocab <= 0 || vocab > 0x7fffffffL || ld_cnt < vocab || n_proto < 0 || n_proto > 0x7fffffffL) {
        padt_set_error("padt_count_update: 0 < vocab <= ld_cnt and 0 <= n_proto < 2^31 are required"); return -1;
    }
    CountArgs a{tokens, ld_tokens, step, unfinished, vrt_off, grid, radius, (unsigned short*)cnt_text, ld_cnt, (int)vocab,
                (unsigned short*)cnt_patch, (unsigned short*)near, (int)n_proto};
    hipLaunchKernelGGL(count_update_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}
