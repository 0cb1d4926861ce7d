// cnn_split.h -- the operand splits of the identity network's matrix-core convolutions, shared by the 80x80 chain (cnn.hip and its
// headers) and the tiled convolutions of every other chain (conv_tiled.h): one definition, so the chains split an operand into the same bits.
//
// Every fp32 operand is split into three bf16 pieces x = x1 + x2 + x3 (x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2); 24
// mantissa bits in total) and a product a*w is formed from the six piece products whose order is >= 2^-16
// (a1w1, a1w2, a2w1, a1w3, a2w2, a3w1; NTERMS = 3 keeps only the first three).  bf16 x bf16 products are
// exact in fp32 and the MFMA accumulates in fp32, so what is dropped is ~3 * 2^-24 relative per product --
// the size of fp32 rounding itself.  v_mfma_f32_32x32x16_bf16 runs at 16x the rate of the fp32 MFMA, so six
// of them per product are 2.7x faster than v_mfma_f32_32x32x2_f32.
#pragma once
#include "conv_f32.h"

namespace trexhip {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t bf16_rne(float x) {
    uint32_t u = __float_as_uint(x);
    u += 0x7fffu + ((u >> 16) & 1u);
    return u >> 16;
}
__device__ __forceinline__ void split3(float x, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    p1 = bf16_rne(x);
    const float r1 = x - __uint_as_float(p1 << 16);
    p2 = bf16_rne(r1);
    const float r2 = r1 - __uint_as_float(p2 << 16);
    p3 = bf16_rne(r2);
}
// fp16 variant: two pieces x = h1 + h2 carry 22 mantissa bits (plus an absolute floor of 3e-8 from fp16 subnormals),
// so the three products h1g1, h1g2, h2g1 are already fp32-class.  fp16 cannot hold |x| >= 65520: such a value raises
// the overflow flag and the host reruns the layer stack with the bf16 split (never a silent wrong answer).
__device__ __forceinline__ void split2h(float x, uint32_t& p1, uint32_t& p2, bool& ovf) {
    const _Float16 h1 = (_Float16)x;
    ovf |= !(fabsf(x) < 65520.0f);
    const float r1 = x - (float)h1;
    const _Float16 h2 = (_Float16)r1;
    p1 = __builtin_bit_cast(uint16_t, h1);
    p2 = __builtin_bit_cast(uint16_t, h2);
}

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// the re-run plan of guard_plan (conv_tiled.h): plan[1] == 1 -> item i is crop plan[2 + i]
__device__ __forceinline__ int plan_crop(const uint32_t* __restrict__ plan, const int i) { return (plan && plan[1] == 1u) ? (int)plan[2 + i] : i; }

}  // namespace trexhip
