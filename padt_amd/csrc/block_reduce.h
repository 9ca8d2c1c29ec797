// Block-wide reductions of the token-selection kernels, in ONE fixed order each, so that a kernel's result does not depend on which file
// spells the loop: the halving LDS tree (s = N/2 … 1: red[tid] = op(red[tid], red[tid + s])) over one value per thread of an N-thread block.
// The strided per-thread accumulation in front of a tree stays in the kernel.  The shuffle-then-wave-partials reductions of
// warp_sample_rows_kernel (sampling.hip) and of topk_rows.hip pair their operands in another order and are not these.
#pragma once
#include "common.h"

PADT_DEV unsigned float_key(float f) {                                    // order-preserving float → uint
    const unsigned u = __builtin_bit_cast(unsigned, f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
PADT_DEV float key_float(unsigned k) {                                    // inverse of float_key
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// red[0] = op over the block's values, every thread gets it; op(a, b) is called with a = red[tid], b = red[tid + s].  No barrier after the
// last read: a caller that writes `red` again puts one in front.
template <int N, class Op>
PADT_DEV float block_tree_lds(float v, float* red, Op op) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] = op(red[tid], red[tid + s]);
        __syncthreads();
    }
    return red[0];
}
template <int N> PADT_DEV float block_max_lds(float v, float* red) { return block_tree_lds<N>(v, red, [](float a, float b) { return fmaxf(a, b); }); }
template <int N> PADT_DEV float block_sum_lds(float v, float* red) { return block_tree_lds<N>(v, red, [](float a, float b) { return a + b; }); }

// (ov, oi) beats (v, i) in an arg-max: the larger value, ties → the lower index (torch.argmax).  The maximum of (value, −index) pairs is
// associative and commutative: any tree gives the same pair.
PADT_DEV bool argmax_less(float v, int i, float ov, int oi) { return ov > v || (ov == v && oi < i); }

// (red_v[0], red_i[0]) = the block's best (value, index) pair under LESS
template <int N, bool (*LESS)(float, int, float, int) = argmax_less>
PADT_DEV void block_argmax_lds(float best, int bidx, float* red_v, int* red_i) {
    const int tid = threadIdx.x;
    red_v[tid] = best;
    red_i[tid] = bidx;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const float ov = red_v[tid + s];
            const int oi = red_i[tid + s];
            if (LESS(red_v[tid], red_i[tid], ov, oi)) { red_v[tid] = ov; red_i[tid] = oi; }
        }
        __syncthreads();
    }
}
