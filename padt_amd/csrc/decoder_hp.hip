// Split-precision ("hp") kernels of the PaDT decoder for gfx950.
//
// Why: the north star asks for box coordinates / mask logits within 1e-3 of the reference's fp32 CPU path.  With bf16
// activation storage between kernels every tensor on the decoder's query path (residual stream, norm outputs, q/k/v,
// attention output, MLP hidden, head inputs) costs 1–2.5e-3 on the boxes BY ITSELF at the real 98 M-parameter shape
// (tests/study_decoder_precision.py), so the decoder keeps
//   * fp32 residual streams (query, memory) and fp32 q / k / v / attention math, and
//   * every GEMM A operand as a bf16 (hi, lo) PAIR: hi = bf16(x), lo = bf16(x - hi) — 16 mantissa bits — stored side by
//     side as [hi(K) | lo(K)] per row, multiplied against the weight image [W | W] (weights.py): the MFMA GEMM kernels run
//     unchanged at K' = 2K and accumulate hi·W + lo·W in fp32.  Weights are bf16 in the reference's GPU path too.
// The decoder is ≈3 % of a step's kernel time, so doubling its MFMA work is cheap; the LLM / ViT stay plain bf16.
//
// Kernels here: norm_split (RMSNorm / add / gather / GELU → fp32 or split rows), rope_half_f32 (in place), two fp32
// varlen attention kernels (few queries x many keys: query→image; many queries x few keys: image→query) writing split
// rows, mask_scatter_f32.  Replaces padt_decoder.py:20-60 (attention), 71-74 / 95-128 (norms), 241-274 (mask head tail).
#include "common.h"
#include <cstdint>

namespace {

PADT_DEV void unpack4h(u32x2 v, float* f) { unpack4x(v, f); }   // this file is compiled for X = bf16 only (the (hi, lo) pairs)

// 4 consecutive columns c..c+3 of one row → hi at [(c / chunk) * 2 * chunk + c % chunk], lo `chunk` elements further
PADT_DEV void split_store4(x16_t* y, long row_off, int c, int chunk, const float* v) {
    x16_t* dst = y + row_off + (long)(c / chunk) * 2 * chunk + (c % chunk);
    const u32x2 hi = u32x2{pack2x(v[0], v[1]), pack2x(v[2], v[3])};
    float h[4];
    unpack4h(hi, h);
    *reinterpret_cast<u32x2*>(dst) = hi;
    *reinterpret_cast<u32x2*>(dst + chunk) = u32x2{pack2x(v[0] - h[0], v[1] - h[1]), pack2x(v[2] - h[2], v[3] - h[3])};
}

enum { OUT_NONE = 0, OUT_F32 = 1, OUT_SPLIT = 2 };

struct NormSplitArgs {
    const void* x; long ldx; int x_f32;          // input rows, bf16 or fp32
    const int* idx;                              // optional row gather: x row of output row r = idx[r]
    const float* a; long lda; int a_div;         // optional pre-norm add: x + a[r / a_div]   (padt_decoder.py:220)
    const x16_t* w; float eps; int act;         // RMSNorm weight (null: no normalisation); act 1 = exact-erf GELU after it
    const float* pos; long ld_pos; long pos_rows;  // optional post-norm add for the SECOND output: y + pos[r % pos_rows]
    void* y0; long ld_y0; int y0_mode;           // first output:  y
    void* y1; long ld_y1; int y1_mode;           // second output: y + pos
    int rows, D, chunk;
};

// one wave per row, 4 columns per lane per step; two passes over the (L2-resident) row
__global__ __launch_bounds__(256) void norm_split_kernel(NormSplitArgs p) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= p.rows) return;
    const long sr = p.idx ? p.idx[row] : row;
    const float* ar = p.a ? p.a + (long)(row / p.a_div) * p.lda : nullptr;
    auto load4 = [&](int c, float* f) {
        if (p.x_f32) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(p.x) + sr * p.ldx + c);
            f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
        } else {
            unpack4h(*reinterpret_cast<const u32x2*>(reinterpret_cast<const x16_t*>(p.x) + sr * p.ldx + c), f);
        }
        if (ar) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(ar + c);
            f[0] += g[0]; f[1] += g[1]; f[2] += g[2]; f[3] += g[3];
        }
    };
    float rstd = 1.f;
    if (p.w) {
        float ss = 0.f;
        for (int c = lane * 4; c < p.D; c += 256) {
            float f[4];
            load4(c, f);
            ss += f[0] * f[0] + f[1] * f[1] + f[2] * f[2] + f[3] * f[3];
        }
        ss = wave_sum(ss);
        rstd = rsqrtf(ss / (float)p.D + p.eps);
    }
    const float* pr = p.pos ? p.pos + (long)(row % p.pos_rows) * p.ld_pos : nullptr;
    for (int c = lane * 4; c < p.D; c += 256) {
        float f[4];
        load4(c, f);
        if (p.w) {
            float wv[4];
            unpack4h(*reinterpret_cast<const u32x2*>(p.w + c), wv);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f[i] = f[i] * rstd * wv[i];
                if (p.act == 1) f[i] = gelu_erf(f[i]);
            }
        }
        if (p.y0_mode == OUT_F32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y0) + (long)row * p.ld_y0 + c) = f32x4{f[0], f[1], f[2], f[3]};
        else if (p.y0_mode == OUT_SPLIT) split_store4(reinterpret_cast<x16_t*>(p.y0), (long)row * p.ld_y0, c, p.chunk, f);
        if (p.y1_mode != OUT_NONE) {
            if (pr) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(pr + c);
                f[0] += g[0]; f[1] += g[1]; f[2] += g[2]; f[3] += g[3];
            }
            if (p.y1_mode == OUT_F32) *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.y1) + (long)row * p.ld_y1 + c) = f32x4{f[0], f[1], f[2], f[3]};
            else split_store4(reinterpret_cast<x16_t*>(p.y1), (long)row * p.ld_y1, c, p.chunk, f);
        }
    }
}

// SwiGLU of fp32 rows [gate(I) | up(I)] → split rows [hi(I) | lo(I)] of silu(gate) * up (HF:85-96, 545-553 at fp32-class precision: the
// "reference" precision mode of ViT / LLM, padt_amd/reference.py); exact expf and an IEEE division, one rounding pair per element.
__global__ __launch_bounds__(256) void swiglu_split_kernel(const float* __restrict__ gu, long ld_gu, int I, x16_t* __restrict__ y, long ld_y, long rows) {
    const long total = rows * (I / 4);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / (I / 4);
        const int c = (int)(i % (I / 4)) * 4;
        const f32x4 g = *reinterpret_cast<const f32x4*>(gu + r * ld_gu + c);
        const f32x4 u = *reinterpret_cast<const f32x4*>(gu + r * ld_gu + I + c);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = g[e] / (1.0f + expf(-g[e])) * u[e];
        split_store4(y, r * ld_y, c, I, v);
    }
}

// LayerNorm (with bias) of fp32 rows → fp32 rows: the prototype projection's vis_norm (padt.py:187-191) in the reference precision mode.
// One wave per row; mean and variance as torch.nn.functional.layer_norm defines them (biased variance, eps inside the root).
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, long ldx, const x16_t* __restrict__ w, const x16_t* __restrict__ b,
                                                            float eps, float* __restrict__ y, long ldy, int rows, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + (long)row * ldx;
    float s = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        s += v[0] + v[1] + v[2] + v[3];
    }
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) q += (v[e] - mean) * (v[e] - mean);
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    for (int c = lane * 4; c < D; c += 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(xr + c);
        float wv[4], bv[4];
        unpack4h(*reinterpret_cast<const u32x2*>(w + c), wv);
        unpack4h(*reinterpret_cast<const u32x2*>(b + c), bv);
        *reinterpret_cast<f32x4*>(y + (long)row * ldy + c) = f32x4{(v[0] - mean) * rstd * wv[0] + bv[0], (v[1] - mean) * rstd * wv[1] + bv[1],
                                                                   (v[2] - mean) * rstd * wv[2] + bv[2], (v[3] - mean) * rstd * wv[3] + bv[3]};
    }
}

// rotate-half rotary in place on fp32 rows: nh heads of width D per token, pairs (d, d + D/2); tables fp32 [T][ld_cs]
__global__ __launch_bounds__(256) void rope_half_f32_kernel(float* __restrict__ x, long ldx, const float* __restrict__ cs,
                                                            const float* __restrict__ sn, long ld_cs, long T, int nh, int D) {
    const int half = D >> 1;
    const long total = T * nh * half;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int d = (int)(i % half);
        const long th = i / half;
        const int h = (int)(th % nh);
        const long t = th / nh;
        float* q = x + t * ldx + (long)h * D;
        const float c = cs[t * ld_cs + d], s = sn[t * ld_cs + d];
        const float x1 = q[d], x2 = q[d + half];
        q[d] = rope_lo(x1, x2, c, s);
        q[d + half] = rope_hi(x1, x2, c, s);
    }
}

struct AttnF32Args {
    const float* q; long ldq;
    const float* k; long ldk;
    const float* v; long ldv;
    x16_t* out; long ldo; int chunk;             // split rows: element (t, h*D + d)
    const int* cu_q; const int* cu_k;
    float scale;
    // round 5 (the reference-precision LLM, padt_amd/reference.py): GQA — q head h reads kv head h / kv_group —, a causal mask aligned
    // bottom-right (key j of a segment is visible to its query i iff j <= i + nk - nq: the prompt pass), and an optional per-segment key
    // COUNT for segments that sit at fixed strides with room to grow (the fp32 KV cache of the decode steps: keys [cu_k[s], cu_k[s] + len_k[s]))
    int kv_group; int causal; const int* len_k;
};

// ---- few queries per segment (<= QB per block; more → blockIdx.y chunks), any number of keys: self-attention of the object
// queries and query→image cross-attention (8 x 2116 per object and head).  Thread j owns key j of a KC-key chunk for the
// score pass (K row in registers, q rows broadcast from LDS); the softmax runs one wave per query over the chunk's scores in
// LDS (online across chunks); P·V runs with one thread per (key partition, d) and o[q] in registers.
constexpr int QB = 16, KC = 256;

template <int D>
__global__ __launch_bounds__(256) void attn_f32_qfew_kernel(AttnF32Args p) {
    constexpr int PARTS = 256 / D;
    static_assert(D % 4 == 0 && D <= 128 && PARTS * QB * D <= QB * KC, "partial-sum buffer aliases the score tile");
    __shared__ __attribute__((aligned(16))) float qs[QB][D];
    __shared__ __attribute__((aligned(16))) float sc[QB][KC];
    __shared__ float m_s[QB], l_s[QB], al_s[QB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = blockIdx.z, h = blockIdx.x;
    const int q0 = p.cu_q[seg] + blockIdx.y * QB, q_end = p.cu_q[seg + 1];
    if (q0 >= q_end) return;
    const int nq = (q_end - q0) < QB ? (q_end - q0) : QB;
    const int k0 = p.cu_k[seg], nk = p.len_k ? p.len_k[seg] : p.cu_k[seg + 1] - k0;
    const int hk = h / p.kv_group;
    // causal: query row q0 + qi is position (q0 + qi - q_begin) of its segment and sees keys 0 .. position + shift
    const int shift = p.causal ? nk - (q_end - p.cu_q[seg]) + (q0 - p.cu_q[seg]) : nk;     // + qi → last visible key of query qi
    for (int i = tid; i < QB * D; i += 256) {
        const int qi = i / D, d = i % D;
        qs[qi][d] = qi < nq ? p.q[(long)(q0 + qi) * p.ldq + (long)h * D + d] * p.scale : 0.f;
    }
    if (tid < QB) { m_s[tid] = -INFINITY; l_s[tid] = 0.f; al_s[tid] = 0.f; }
    const int part = tid / D, d = tid % D;
    const bool active = part < PARTS;
    float o[QB];
#pragma unroll
    for (int qi = 0; qi < QB; ++qi) o[qi] = 0.f;

    for (int kc = 0; kc < nk; kc += KC) {
        const int n = (nk - kc) < KC ? (nk - kc) : KC;
        __syncthreads();                                          // qs / state ready; previous chunk's P·V done with sc
        if (tid < n) {
            const float* kr = p.k + (long)(k0 + kc + tid) * p.ldk + (long)hk * D;
            float kreg[D];
#pragma unroll
            for (int c = 0; c < D; c += 4) {
                const f32x4 t4 = *reinterpret_cast<const f32x4*>(kr + c);
                kreg[c] = t4[0]; kreg[c + 1] = t4[1]; kreg[c + 2] = t4[2]; kreg[c + 3] = t4[3];
            }
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) {
                if (qi < nq) {
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < D; ++c) s += qs[qi][c] * kreg[c];
                    sc[qi][tid] = (p.causal && kc + tid > shift + qi) ? -INFINITY : s;      // exp(-inf - m) = 0: the key is not there
                }
            }
        }
        __syncthreads();
        for (int qi = wave; qi < nq; qi += 4) {                   // one wave per query: chunk max, exp, sum
            float mx = -INFINITY;
            for (int j = lane; j < n; j += 64) mx = fmaxf(mx, sc[qi][j]);
            mx = wave_max(mx);
            const float m_old = m_s[qi];
            const float m_new = fmaxf(m_old, mx);
            const float alpha = expf(m_old - m_new);              // first chunk: exp(-inf) = 0
            float sum = 0.f;
            for (int j = lane; j < n; j += 64) {
                const float pj = expf(sc[qi][j] - m_new);
                sc[qi][j] = pj;
                sum += pj;
            }
            sum = wave_sum(sum);
            if (lane == 0) { m_s[qi] = m_new; l_s[qi] = l_s[qi] * alpha + sum; al_s[qi] = alpha; }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int qi = 0; qi < QB; ++qi) if (qi < nq) o[qi] *= al_s[qi];
            const float* vb = p.v + (long)(k0 + kc) * p.ldv + (long)hk * D + d;
            int j = part;
            for (; j + 3 * PARTS < n; j += 4 * PARTS) {           // 4 independent V loads in flight
                const float v0 = vb[(long)j * p.ldv], v1 = vb[(long)(j + PARTS) * p.ldv];
                const float v2 = vb[(long)(j + 2 * PARTS) * p.ldv], v3 = vb[(long)(j + 3 * PARTS) * p.ldv];
#pragma unroll
                for (int qi = 0; qi < QB; ++qi)
                    if (qi < nq) o[qi] += sc[qi][j] * v0 + sc[qi][j + PARTS] * v1 + sc[qi][j + 2 * PARTS] * v2 + sc[qi][j + 3 * PARTS] * v3;
            }
            for (; j < n; j += PARTS) {
                const float v0 = vb[(long)j * p.ldv];
#pragma unroll
                for (int qi = 0; qi < QB; ++qi) if (qi < nq) o[qi] += sc[qi][j] * v0;
            }
        }
    }
    __syncthreads();
    float* red = &sc[0][0];                                       // [PARTS][QB][D] partial sums
    if (active) {
#pragma unroll
        for (int qi = 0; qi < QB; ++qi) if (qi < nq) red[(part * QB + qi) * D + d] = o[qi];
    }
    __syncthreads();
    for (int i = tid; i < nq * (D / 4); i += 256) {
        const int qi = i / (D / 4), c = (i % (D / 4)) * 4;
        const float inv = l_s[qi] > 0.f ? 1.f / l_s[qi] : 0.f;   // a segment without keys yields zero rows (as attn_varlen_kernel), not NaN
        float v4[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float s = 0.f;
#pragma unroll
            for (int pp = 0; pp < PARTS; ++pp) s += red[(pp * QB + qi) * D + c + e];
            v4[e] = s * inv;
        }
        split_store4(p.out, (long)(q0 + qi) * p.ldo, h * D + c, p.chunk, v4);
    }
}

// ---- many queries, few keys per segment: image→query cross-attention (2116 image rows x 3 + n_vrt object queries).  One
// thread per (query row, head): scores against the key chunk in LDS (broadcast reads), online softmax across chunks of KB keys,
// o[D] in registers.
constexpr int KB = 32;

template <int D>
__global__ __launch_bounds__(256) void attn_f32_kfew_kernel(AttnF32Args p) {
    __shared__ __attribute__((aligned(16))) float ks[KB][D];
    __shared__ __attribute__((aligned(16))) float vs[KB][D];
    __shared__ float ps[KB][256];
    const int tid = threadIdx.x;
    const int seg = blockIdx.z, h = blockIdx.y;
    const int q_begin = p.cu_q[seg], q_end = p.cu_q[seg + 1];
    if (q_begin + (int)blockIdx.x * 256 >= q_end) return;
    const int row = q_begin + blockIdx.x * 256 + tid;
    const bool valid = row < q_end;
    const int k0 = p.cu_k[seg], nk = p.len_k ? p.len_k[seg] : p.cu_k[seg + 1] - k0;
    const int hk = h / p.kv_group;
    const int lim = p.causal ? (row - q_begin) + nk - (q_end - q_begin) : nk - 1;          // last key this query row sees
    const float* qr = p.q + (long)(valid ? row : q_begin) * p.ldq + (long)h * D;
    float o[D];
#pragma unroll
    for (int c = 0; c < D; ++c) o[c] = 0.f;
    float m = -INFINITY, l = 0.f;
    for (int kc = 0; kc < nk; kc += KB) {
        const int n = (nk - kc) < KB ? (nk - kc) : KB;
        __syncthreads();
        for (int i = tid; i < n * (D / 4); i += 256) {
            const int j = i / (D / 4), c = (i % (D / 4)) * 4;
            *reinterpret_cast<f32x4*>(&ks[j][c]) = *reinterpret_cast<const f32x4*>(p.k + (long)(k0 + kc + j) * p.ldk + (long)hk * D + c);
            *reinterpret_cast<f32x4*>(&vs[j][c]) = *reinterpret_cast<const f32x4*>(p.v + (long)(k0 + kc + j) * p.ldv + (long)hk * D + c);
        }
        __syncthreads();
        const int nv = (lim - kc + 1) < n ? (lim - kc + 1) : n;      // keys of this chunk the row sees (all of them without a causal mask)
        if (nv <= 0) continue;                                        // (the barrier at the loop head keeps the block together)
        float s[KB];
#pragma unroll
        for (int j = 0; j < KB; ++j) s[j] = 0.f;
#pragma unroll 2
        for (int c = 0; c < D; c += 4) {
            f32x4 q4 = *reinterpret_cast<const f32x4*>(qr + c);
            q4 *= p.scale;
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                if (j < nv) {
                    const f32x4 k4 = *reinterpret_cast<const f32x4*>(&ks[j][c]);
                    s[j] += q4[0] * k4[0] + q4[1] * k4[1] + q4[2] * k4[2] + q4[3] * k4[3];
                }
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < KB; ++j) if (j < nv) mx = fmaxf(mx, s[j]);
        const float m_new = fmaxf(m, mx);
        const float alpha = expf(m - m_new);
        l *= alpha;
#pragma unroll
        for (int c = 0; c < D; ++c) o[c] *= alpha;
        // probabilities go through a per-thread LDS column so the P·V loop can run over a RUNTIME key index (o[] stays in
        // registers: every o index is a compile-time constant)
#pragma unroll
        for (int j = 0; j < KB; ++j) {
            const float pj = j < nv ? expf(s[j] - m_new) : 0.f;
            l += pj;
            ps[j][tid] = pj;
        }
        for (int j = 0; j < nv; ++j) {
            const float pj = ps[j][tid];
#pragma unroll
            for (int c = 0; c < D; c += 4) {
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(&vs[j][c]);
                o[c] += pj * v4[0]; o[c + 1] += pj * v4[1]; o[c + 2] += pj * v4[2]; o[c + 3] += pj * v4[3];
            }
        }
        m = m_new;
    }
    if (!valid) return;
    const float inv = l > 0.f ? 1.f / l : 0.f;
#pragma unroll
    for (int c = 0; c < D; c += 4) {
        const float v4[4] = {o[c] * inv, o[c + 1] * inv, o[c + 2] * inv, o[c + 3] * inv};
        split_store4(p.out, (long)row * p.ldo, h * D + c, p.chunk, v4);
    }
}

}  // namespace

// y0 = f(x) and/or y1 = f(x) + pos[r % pos_rows], f(x) = act(RMSNorm_w(x[idx[r]] + add[r / add_div])) with every stage optional;
// each output fp32 rows (mode 1) or bf16 (hi | lo) split rows (mode 2; `chunk` = width of one hi / lo group, D % chunk == 0:
// a row is [hi(chunk) lo(chunk)] x D/chunk, so a (rows, D) → (rows * D/chunk, chunk) re-view keeps the pairing).
extern "C" int padt_norm_split(void* stream, const void* x, long ldx, int x_f32, const int* idx, const void* add_f32, long ld_add,
                               int add_div, const void* w, float eps, int act, const void* pos_f32, long ld_pos, long pos_rows,
                               void* y0, long ld_y0, int y0_mode, void* y1, long ld_y1, int y1_mode, long rows, long D, long chunk) {
    if (rows <= 0) return 0;
    if (chunk <= 0) chunk = D;
    if ((D & 3) || (chunk & 3) || D % chunk || (ldx & 3) || (add_f32 && ((ld_add & 3) || add_div <= 0)) || (pos_f32 && ((ld_pos & 3) || pos_rows <= 0)) ||
        y0_mode < 0 || y0_mode > 2 || y1_mode < 0 || y1_mode > 2 || (y0_mode && (!y0 || (ld_y0 & 3))) || (y1_mode && (!y1 || (ld_y1 & 3))) ||
        ((uintptr_t)x & 7) || (x_f32 && ((uintptr_t)x & 15)) || ((uintptr_t)add_f32 & 15) || ((uintptr_t)pos_f32 & 15) || ((uintptr_t)w & 7) ||
        ((uintptr_t)y0 & 15) || ((uintptr_t)y1 & 15) || (y0_mode == 0 && y1_mode == 0)) {
        padt_set_error("padt_norm_split: D, chunk and strides must be multiples of 4 (D % chunk == 0), pointers 16-byte aligned, modes in 0..2");
        return -1;
    }
    NormSplitArgs a{x, ldx, x_f32, idx, (const float*)add_f32, ld_add, add_div, (const x16_t*)w, eps, act, (const float*)pos_f32, ld_pos,
                    pos_rows, y0, ld_y0, y0_mode, y1, ld_y1, y1_mode, (int)rows, (int)D, (int)chunk};
    hipLaunchKernelGGL(norm_split_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_swiglu_split(void* stream, const void* gu_f32, long ld_gu, long I, void* y_split, long ld_y, long rows) {
    if (rows <= 0 || I <= 0) return 0;
    if ((I & 3) || (ld_gu & 3) || (ld_y & 3) || ld_gu < 2 * I || ld_y < 2 * I || ((uintptr_t)gu_f32 & 15) || ((uintptr_t)y_split & 7)) {
        padt_set_error("padt_swiglu_split: I and strides multiples of 4, ld_gu / ld_y >= 2 I, 16-byte aligned rows");
        return -1;
    }
    long blocks = (rows * (I / 4) + 255) / 256;
    if (blocks > 32768) blocks = 32768;
    hipLaunchKernelGGL(swiglu_split_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)gu_f32, ld_gu, (int)I, (x16_t*)y_split, ld_y, rows);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_layernorm_f32(void* stream, const void* x_f32, long ldx, const void* w, const void* b, float eps, void* y_f32, long ldy, long rows, long D) {
    if (rows <= 0) return 0;
    if ((D & 3) || (ldx & 3) || (ldy & 3) || w == nullptr || b == nullptr || ((uintptr_t)x_f32 & 15) || ((uintptr_t)y_f32 & 15) || ((uintptr_t)w & 7) || ((uintptr_t)b & 7)) {
        padt_set_error("padt_layernorm_f32: D and strides multiples of 4, bf16 weight and bias, 16-byte aligned rows");
        return -1;
    }
    hipLaunchKernelGGL(layernorm_f32_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)x_f32, ldx, (const x16_t*)w,
                       (const x16_t*)b, eps, (float*)y_f32, ldy, (int)rows, (int)D);
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_rope_half_f32(void* stream, void* x, long ldx, const void* cos_t, const void* sin_t, long ld_cs, long T,
                                  int n_heads, int head_dim) {
    if (T <= 0) return 0;
    if (head_dim & 1) { padt_set_error("padt_rope_half_f32: head_dim must be even"); return -1; }
    const long total = T * n_heads * (head_dim / 2);
    long blocks = (total + 255) / 256;
    if (blocks > 32768) blocks = 32768;
    hipLaunchKernelGGL(rope_half_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)x, ldx,
                       (const float*)cos_t, (const float*)sin_t, ld_cs, T, n_heads, head_dim);
    PADT_CHECK_LAUNCH();
    return 0;
}

template <int D>
static void launch_attn_f32(const AttnF32Args& a, int nseg, int max_q, int max_k, int n_heads, hipStream_t s) {
    if (max_q <= 4 * QB || max_k > max_q)                        // few queries per segment (or the longer side is the keys)
        hipLaunchKernelGGL(attn_f32_qfew_kernel<D>, dim3(n_heads, (max_q + QB - 1) / QB, nseg), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(attn_f32_kfew_kernel<D>, dim3((max_q + 255) / 256, n_heads, nseg), dim3(256), 0, s, a);
}

// fp32 varlen non-causal attention, softmax(q k^T * scale) v per segment and head (padt_decoder.py:52-58, flash_attn_varlen_func),
// exact expf, fp32 accumulation; output as split (hi | lo) rows for the out-projection.  q/k/v rows hold the heads contiguously.
extern "C" int padt_attn_f32(void* stream, const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* out_split,
                             long ldo, long chunk, const int* cu_q, const int* cu_k, int nseg, int max_seqlen_q, int max_seqlen_k,
                             int n_heads, int head_dim, float scale, int kv_group, int causal, const int* len_k) {
    if (nseg <= 0 || max_seqlen_q <= 0) return 0;
    if (kv_group < 1 || n_heads % kv_group) { padt_set_error("padt_attn_f32: kv_group must divide n_heads"); return -1; }
    if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3) || (chunk & 3) || chunk <= 0 || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) ||
        ((uintptr_t)v & 15) || ((uintptr_t)out_split & 7) || max_seqlen_k <= 0 || nseg > 65535 || n_heads > 65535) {
        padt_set_error("padt_attn_f32: strides / chunk multiples of 4, 16-byte aligned q/k/v, nseg and n_heads <= 65535");
        return -1;
    }
    AttnF32Args a{(const float*)q, ldq, (const float*)k, ldk, (const float*)v, ldv, (x16_t*)out_split, ldo, (int)chunk, cu_q, cu_k, scale, kv_group,
                  causal ? 1 : 0, len_k};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: launch_attn_f32<32>(a, nseg, max_seqlen_q, max_seqlen_k, n_heads, s); break;
        case 64: launch_attn_f32<64>(a, nseg, max_seqlen_q, max_seqlen_k, n_heads, s); break;
        case 80: launch_attn_f32<80>(a, nseg, max_seqlen_q, max_seqlen_k, n_heads, s); break;
        case 128: launch_attn_f32<128>(a, nseg, max_seqlen_q, max_seqlen_k, n_heads, s); break;
        default: padt_set_error("padt_attn_f32: head_dim must be 32, 64, 80 or 128"); return -1;
    }
    PADT_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// fp32 attention on the f32-input matrix cores (round 6): softmax(q k^T * scale) v with EXACT fp32 operands through
// v_mfma_f32_16x16x4_f32 (bit for bit an fmaf chain; 64 FLOP / clk / SIMD = the fp32 vector peak, reached from one wave per SIMD and with
// the VALU free for the softmax).  The reference-precision mode (padt_amd/reference.py) ran every attention of ViT and LLM on the VALU
// kernels above — 40 % of its time (profiles/r05_reference_precision_kernel_stats.md): 2116 x 2116 ViT layers 11.6 ms, a causal
// 577-token prompt layer 1.75 ms.  Same arguments and semantics as padt_attn_f32 (GQA, bottom-right causal mask, per-segment key counts
// over a strided cache, split (hi | lo) output rows).
//
// Everything is computed TRANSPOSED so that a lane owns one query column from the first MFMA to the store (as csrc/attention.hip does
// for 16-bit operands): S^T = K Q^T — lane (j, g) = (lane & 15, lane >> 4) ends up with S^T[key 4g + r][query j], r = 0..3 — the row
// max / sum are in-lane plus two shuffles across g, and those four registers ARE the B operand of O^T = V^T P^T under the key permutation
// "k-slot g of MFMA r = key 4g + r", which the V^T operand applies too.  The contraction index of Q K^T is permuted likewise so that every
// lane reads CONTIGUOUS floats: k-slot g of MFMA (c, e) = d = g * D/4 + 4c + e → lane (i, g) holds row i's chunk [g D/4, (g + 1) D/4) of K
// (and of Q) as D/16 float4 loads; the A-row index i of a V^T d-tile n maps to d = i * D/16 + n (D = 128: 8 contiguous floats per lane
// and key) or, for D = 80, d = 4i + n (n < 4) and 64 + i (n = 4): one float4 + one float.  Operands go global / L2 → registers directly
// (no LDS): a wave carries QT tiles of 16 queries, so each K / V fragment feeds QT MFMAs.
// Column modes: token mode — column c of a wave = query token qbase + c of head blockIdx.y; head mode (few queries per segment: the
// decode steps) — column c = (token qbase + c / G, head hk G + c % G) of kv head hk = blockIdx.y, so the G query heads of a GQA group
// share every K / V fragment.
struct AttnMfmaArgs {
    AttnF32Args a;
    int head_mode;       // 0 token mode, 1 head mode
};

template <int D>
struct VMap {            // lane (i = lane & 15) of V^T d-tile n ↔ d
    static constexpr int NT = D / 16;
};

// KS (head mode): the 4 waves of a block take the SAME query columns and every fourth 32-key block each; their (m, l, O) states are merged
// through LDS by wave 0 — a decode step has one query token per segment, so the key range is the only parallelism a block has.
template <int D, int QT, bool KS>
__global__ __launch_bounds__(256, 2) void attn_f32_mfma_kernel(AttnMfmaArgs pa) {
    static_assert(D == 128 || D == 80, "head widths of LLM (128) and ViT / PaDT decoder (80)");
    const AttnF32Args& p = pa.a;
    constexpr int C4 = D / 16;                  // float4 pieces of a lane's K / Q chunk (D/4 floats)
    constexpr int NT = D / 16;                  // 16-row d-tiles of O^T
    constexpr int COLS = 16 * QT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const int seg = blockIdx.z;
    const int qs0 = p.cu_q[seg], nq_seg = p.cu_q[seg + 1] - qs0;
    const int k0 = p.cu_k[seg], nk = p.len_k ? p.len_k[seg] : p.cu_k[seg + 1] - k0;
    const int G = p.kv_group;
    const int tpw = pa.head_mode ? COLS / G : COLS;                     // query tokens per wave
    const int qbase = (KS ? blockIdx.x : blockIdx.x * 4 + wave) * tpw;  // first token (within the segment) of this wave
    if (qbase >= nq_seg) return;                                        // (KS: block-uniform, so nobody waits at the merge barrier)
    const int hk = pa.head_mode ? blockIdx.y : blockIdx.y / G;
    const int shift = p.causal ? nk - nq_seg : nk;                      // query at segment position i sees keys 0 .. i + shift
    // ---- per q-tile: this lane's query column
    int q_pos[QT];            // position within the segment (clamped for loads)
    bool q_ok[QT];
    long q_off[QT];           // element offset of the column's head row in q / out coordinates: token * ld + head * D
    int q_head[QT];
    f32x4 qf[QT][C4];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int c = t * 16 + j;
        int tok = pa.head_mode ? qbase + c / G : qbase + c;
        const int hh = pa.head_mode ? hk * G + c % G : blockIdx.y;
        q_ok[t] = tok < nq_seg && (!pa.head_mode || c / G < tpw);
        tok = tok < nq_seg ? tok : nq_seg - 1;
        q_pos[t] = tok;
        q_head[t] = hh;
        const float* qr = p.q + (long)(qs0 + tok) * p.ldq + (long)hh * D + g * (D / 4);
#pragma unroll
        for (int c4 = 0; c4 < C4; ++c4) {
            f32x4 v = *reinterpret_cast<const f32x4*>(qr + 4 * c4);
            qf[t][c4] = v * p.scale;
        }
    }
    // last key any column of this wave may see (causal: the wave's last token)
    int k_end = nk;
    if (p.causal) {
        int last = qbase + tpw - 1;
        last = last < nq_seg ? last : nq_seg - 1;
        k_end = last + shift + 1;
        k_end = k_end < nk ? k_end : nk;
    }
    f32x4 o[QT][NT];
    float m[QT], l[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        m[t] = -INFINITY; l[t] = 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n) o[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* kbase = p.k + (long)k0 * p.ldk + (long)hk * D + g * (D / 4);
    const float* vbase = p.v + (long)k0 * p.ldv + (long)hk * D;
    constexpr int KB = 32;                                             // keys per softmax step (two 16-key MFMA tiles)
    for (int kb = KS ? wave * KB : 0; kb < k_end; kb += KS ? 4 * KB : KB) {
        f32x4 s[QT][2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            int key = kb + u * 16 + j;                                 // A row i = j: this lane's key row of tile u
            key = key < nk ? key : nk - 1;
            const float* kr = kbase + (long)key * p.ldk;
            f32x4 kf[C4];
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) kf[c4] = *reinterpret_cast<const f32x4*>(kr + 4 * c4);
#pragma unroll
            for (int t = 0; t < QT; ++t) s[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4)
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < QT; ++t) s[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[c4][e], qf[t][c4][e], s[t][u], 0, 0, 0);
        }
        // ---- mask + online softmax (per query column; the 4 lanes g = 0..3 of a column share m)
        float alpha[QT];
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const int vis = p.causal ? q_pos[t] + shift : nk - 1;      // last visible key of this column
            float mx = -INFINITY;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = kb + u * 16 + 4 * g + r;
                    const bool ok = key < nk && key <= vis;
                    s[t][u][r] = ok ? s[t][u][r] : -INFINITY;
                    mx = fmaxf(mx, s[t][u][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
            const float m_new = fmaxf(m[t], mx);
            // a column that has seen no visible key yet keeps m = -inf: exp(-inf - -inf) must not be NaN
            const float m_use = m_new == -INFINITY ? 0.f : m_new;
            alpha[t] = expf(m[t] - m_use);                             // first visible block: exp(-inf) = 0
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pj = expf(s[t][u][r] - m_use);
                    s[t][u][r] = pj;
                    sum += pj;
                }
            l[t] = l[t] * alpha[t] + sum;                              // per-lane partial; reduced across g at the end
            m[t] = m_new;
#pragma unroll
            for (int n = 0; n < NT; ++n) o[t][n] *= alpha[t];
        }
        // ---- O^T += V^T P^T: A[i][k-slot g] = V[key u 16 + 4g + r][dmap(i, n)], B = the P registers
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int key = kb + u * 16 + 4 * g + r;
                key = key < nk ? key : nk - 1;                         // P is exactly 0 there
                const float* vr = vbase + (long)key * p.ldv;
                float vf[NT];
                if constexpr (D == 128) {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(vr + 8 * j), a1 = *reinterpret_cast<const f32x4*>(vr + 8 * j + 4);
                    vf[0] = a0[0]; vf[1] = a0[1]; vf[2] = a0[2]; vf[3] = a0[3]; vf[4] = a1[0]; vf[5] = a1[1]; vf[6] = a1[2]; vf[7] = a1[3];
                } else {
                    const f32x4 a0 = *reinterpret_cast<const f32x4*>(vr + 4 * j);
                    vf[0] = a0[0]; vf[1] = a0[1]; vf[2] = a0[2]; vf[3] = a0[3]; vf[4] = vr[64 + j];
                }
#pragma unroll
                for (int n = 0; n < NT; ++n)
#pragma unroll
                    for (int t = 0; t < QT; ++t) o[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[n], s[t][u][r], o[t][n], 0, 0, 0);
            }
    }
    if constexpr (KS) {
        // ---- merge the 4 waves' partial states (disjoint key sets of the same columns): wave 0 rescales each to the common maximum
        static_assert(QT == 1, "head mode runs one query tile per wave");
        __shared__ float mst[3][64][NT * 4 + 2];
        if (wave > 0) {
            float* dst = mst[wave - 1][lane];
            dst[0] = m[0]; dst[1] = l[0];
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[2 + n * 4 + r] = o[0][n][r];
        }
        __syncthreads();
        if (wave > 0) return;
        float mw[3], mm = m[0];
#pragma unroll
        for (int w = 0; w < 3; ++w) { mw[w] = mst[w][lane][0]; mm = fmaxf(mm, mw[w]); }
        const float m_use = mm == -INFINITY ? 0.f : mm;
        const float f0 = expf(m[0] - m_use);
        l[0] *= f0;
#pragma unroll
        for (int n = 0; n < NT; ++n) o[0][n] *= f0;
#pragma unroll
        for (int w = 0; w < 3; ++w) {
            const float f = expf(mw[w] - m_use);
            const float* src = mst[w][lane];
            l[0] += src[1] * f;
#pragma unroll
            for (int n = 0; n < NT; ++n)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[0][n][r] += src[2 + n * 4 + r] * f;
        }
    }
    // ---- normalise and store split rows: lane (j, g) holds O[query j][d = dmap(4g + r, n)]
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        float ls = l[t];
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        if (!q_ok[t]) continue;
        const float inv = ls > 0.f ? 1.f / ls : 0.f;                   // a query without visible keys yields a zero row, not NaN
        const long row = (long)(qs0 + q_pos[t]) * p.ldo;
        const int col0 = q_head[t] * D;
        if constexpr (D == 128) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v4[4];
#pragma unroll
                for (int half = 0; half < 2; ++half) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v4[e] = o[t][half * 4 + e][r] * inv;
                    split_store4(p.out, row, col0 + 8 * (4 * g + r) + 4 * half, p.chunk, v4);
                }
            }
        } else {
            float v4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v4[e] = o[t][e][r] * inv;
                split_store4(p.out, row, col0 + 4 * (4 * g + r), p.chunk, v4);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) v4[r] = o[t][4][r] * inv;
            split_store4(p.out, row, col0 + 64 + 4 * g, p.chunk, v4);
        }
    }
}

template <int D>
static void launch_attn_f32_mfma(const AttnF32Args& a, int nseg, int max_q, int n_heads, hipStream_t s) {
    const int G = a.kv_group;
    // head mode pays when a segment has too few queries to fill 16 columns with tokens of ONE head and the group fits a tile
    const bool head_mode = G > 1 && G <= 16 && max_q < 16;
    AttnMfmaArgs pa{a, head_mode ? 1 : 0};
    if (head_mode) {
        const int tpw = 16 / G;
        hipLaunchKernelGGL((attn_f32_mfma_kernel<D, 1, true>), dim3((max_q + tpw - 1) / tpw, n_heads / G, nseg), dim3(256), 0, s, pa);
    } else if (max_q > 16) {
        hipLaunchKernelGGL((attn_f32_mfma_kernel<D, 2, false>), dim3((max_q + 127) / 128, n_heads, nseg), dim3(256), 0, s, pa);
    } else {
        hipLaunchKernelGGL((attn_f32_mfma_kernel<D, 1, false>), dim3((max_q + 63) / 64, n_heads, nseg), dim3(256), 0, s, pa);
    }
}

// padt_attn_f32 on the f32-input MFMA (same arguments, same results up to fp32 summation order); head_dim 80 or 128.
extern "C" int padt_attn_f32_mfma(void* stream, const void* q, long ldq, const void* k, long ldk, const void* v, long ldv, void* out_split,
                                  long ldo, long chunk, const int* cu_q, const int* cu_k, int nseg, int max_seqlen_q, int max_seqlen_k,
                                  int n_heads, int head_dim, float scale, int kv_group, int causal, const int* len_k) {
    if (nseg <= 0 || max_seqlen_q <= 0) return 0;
    if (kv_group < 1 || n_heads % kv_group) { padt_set_error("padt_attn_f32_mfma: kv_group must divide n_heads"); return -1; }
    if ((ldq & 3) || (ldk & 3) || (ldv & 3) || (ldo & 3) || (chunk & 3) || chunk <= 0 || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) ||
        ((uintptr_t)v & 15) || ((uintptr_t)out_split & 7) || max_seqlen_k <= 0 || nseg > 65535 || n_heads > 65535) {
        padt_set_error("padt_attn_f32_mfma: strides / chunk multiples of 4, 16-byte aligned q/k/v, nseg and n_heads <= 65535");
        return -1;
    }
    AttnF32Args a{(const float*)q, ldq, (const float*)k, ldk, (const float*)v, ldv, (x16_t*)out_split, ldo, (int)chunk, cu_q, cu_k, scale, kv_group,
                  causal ? 1 : 0, len_k};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 80: launch_attn_f32_mfma<80>(a, nseg, max_seqlen_q, n_heads, s); break;
        case 128: launch_attn_f32_mfma<128>(a, nseg, max_seqlen_q, n_heads, s); break;
        default: padt_set_error("padt_attn_f32_mfma: head_dim must be 80 or 128"); return -1;
    }
    PADT_CHECK_LAUNCH();
    return 0;
}

extern "C" int padt_mask_scatter_f32(void* stream, const void* e2, long ld_e2, const void* mask_tok, long ld_tok, const int* cu_patch,
                                     const int* obj_w, void* masks_f32, int n_obj, long total_patches, int Hm4, int Wm4, int dm) {
    if (n_obj <= 0 || total_patches <= 0) return 0;
    long blocks = (total_patches * 16 + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(mask_scatter_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)e2, ld_e2,
                       (const float*)mask_tok, ld_tok, cu_patch, obj_w, (float*)masks_f32, n_obj, Hm4, Wm4, dm);
    PADT_CHECK_LAUNCH();
    return 0;
}
