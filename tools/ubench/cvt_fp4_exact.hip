// Exhaustive check of the gfx950 e2m1 → 16-bit conversions behind the MXFP4 decode kernel (csrc/common.h fp4x8_to_x16x8):
// v_cvt_scalef32_pk_bf16_fp4 / v_cvt_scalef32_pk_f16_fp4 for every byte (two codes) x every E8M0 scale byte, against
// sign * {0, .5, 1, 1.5, 2, 3, 4, 6} * 2^(E - 127) computed in double.  Prints the nibble order, the first mismatches and, per type, the
// range of scale bytes over which all 16 codes convert exactly (result recorded in profiles/mxfp4_decode.md).
//   hipcc --offload-arch=gfx950 -O2 -o tools/ubench/cvt_fp4_exact tools/ubench/cvt_fp4_exact.hip && tools/ubench/cvt_fp4_exact
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
typedef __attribute__((ext_vector_type(2))) _Float16 h2;
// out[(E*256 + byte)*2 + t] : packed 2x16 result
__global__ void k(unsigned* out) {
    const int E = blockIdx.x, b = threadIdx.x;
    const float scale = __builtin_bit_cast(float, (unsigned)E << 23);
    const unsigned src = (unsigned)b << 8;          // byte 1 holds the codes: checks byte_sel too
    bf2 r = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(src, scale, 1);
    h2 s = __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(src, scale, 1);
    out[(E * 256 + b) * 2 + 0] = __builtin_bit_cast(unsigned, r);
    out[(E * 256 + b) * 2 + 1] = __builtin_bit_cast(unsigned, s);
}
static const double grid[8] = {0, .5, 1, 1.5, 2, 3, 4, 6};
static uint16_t to_bf16(double v) {   // exact values only: truncation is fine if exact, report otherwise
    float f = (float)v; uint32_t u; memcpy(&u, &f, 4);
    return (uint16_t)(u >> 16);
}
static uint16_t to_f16(double v, int* exact) {
    _Float16 h = (_Float16)v; *exact = ((double)h == v); uint16_t u; memcpy(&u, &h, 2); return u;
}
int main() {
    unsigned* d; const int n = 256 * 256 * 2;
    if (hipMalloc(&d, n * 4) != hipSuccess) return 2;
    hipLaunchKernelGGL(k, dim3(256), dim3(256), 0, 0, d);
    unsigned* h = (unsigned*)malloc(n * 4);
    if (hipMemcpy(h, d, n * 4, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    printf("byte 0x21 at E=127: bf16 %08x f16 %08x (low 16 bits = element 0)\n", h[(127 * 256 + 0x21) * 2], h[(127 * 256 + 0x21) * 2 + 1]);
    printf("byte 0x80 (element 1 = -0) at E=127: bf16 %08x f16 %08x\n", h[(127 * 256 + 0x80) * 2], h[(127 * 256 + 0x80) * 2 + 1]);
    int bf_lo = -1, bf_hi = -1, h_lo = -1, h_hi = -1, nbf = 0, nh = 0;
    for (int E = 0; E < 256; ++E) {
        int okb = 1, okh = 1;
        for (int b = 0; b < 256; ++b) for (int t = 0; t < 2; ++t) {
            const int c = t ? (b >> 4) : (b & 15);
            double v = grid[c & 7] * ldexp(1.0, E - 127) * ((c & 8) ? -1.0 : 1.0);
            if ((c & 7) == 0 && (c & 8)) v = -0.0;
            uint16_t gb = (h[(E * 256 + b) * 2] >> (16 * t)) & 0xffff, gh = (h[(E * 256 + b) * 2 + 1] >> (16 * t)) & 0xffff;
            float vf = (float)v; if ((double)vf != v || (to_bf16(v) != gb)) { uint32_t u; memcpy(&u, &vf, 4); if ((u & 0xffff) || to_bf16(v) != gb) { if (okb && nbf < 12) { printf("bf16 mismatch E=%d code=%x want %04x got %04x\n", E, c, to_bf16(v), gb); nbf++; } okb = 0; } }
            int ex; uint16_t wh = to_f16(v, &ex);
            if (!ex || wh != gh) { if (okh && ex && nh < 12) { printf("f16 mismatch (representable) E=%d code=%x want %04x got %04x\n", E, c, wh, gh); nh++; } okh = 0; }
        }
        if (okb) { if (bf_lo < 0) bf_lo = E; bf_hi = E; }
        if (okh) { if (h_lo < 0) h_lo = E; h_hi = E; }
    }
    printf("bf16 exact for E8M0 in [%d, %d]; f16 exact (all codes representable and equal) in [%d, %d]\n", bf_lo, bf_hi, h_lo, h_hi);
    return 0;
}
