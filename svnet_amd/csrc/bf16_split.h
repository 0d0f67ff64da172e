// The exact three-way bf16 split of an fp32 value, x = h + m + l: what lets the bf16 matrix cores form fp32-exact products
// (gemm_mfma.hip, phase B of edgeblock_bwd.hip).  Both subtractions are exact; l has at most 8 significant bits.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;

__device__ __forceinline__ __bf16 bf16_from_bits(uint32_t b) { return __builtin_bit_cast(__bf16, (unsigned short)b); }

// one value: the pieces' bf16 bit patterns
__device__ __forceinline__ void split3(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
    const uint32_t hu = __float_as_uint(x) & 0xFFFF0000u;
    const float r1 = x - __uint_as_float(hu);
    const uint32_t mu = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(mu);
    h = hu >> 16;
    m = mu >> 16;
    l = __float_as_uint(r2) >> 16;
}
// an MFMA fragment of eight values
struct Split3 {
    bf16x8 h, m, l;
};
__device__ __forceinline__ Split3 split_frag(const float (&x)[8]) {
    Split3 s;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        uint32_t h, m, l;
        split3(x[j], h, m, l);
        s.h[j] = bf16_from_bits(h);
        s.m[j] = bf16_from_bits(m);
        s.l[j] = bf16_from_bits(l);
    }
    return s;
}
// a pair of values, packed as two bf16 per word (low half = a)
__device__ __forceinline__ void split3_pair(float a, float b, uint32_t& h, uint32_t& m, uint32_t& l) {
    const float a1 = a - __uint_as_float(__float_as_uint(a) & 0xFFFF0000u), b1 = b - __uint_as_float(__float_as_uint(b) & 0xFFFF0000u);
    const float a2 = a1 - __uint_as_float(__float_as_uint(a1) & 0xFFFF0000u), b2 = b1 - __uint_as_float(__float_as_uint(b1) & 0xFFFF0000u);
    h = __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);      // upper halves of (a, b)
    m = __builtin_amdgcn_perm(__float_as_uint(b1), __float_as_uint(a1), 0x07060302u);
    l = __builtin_amdgcn_perm(__float_as_uint(b2), __float_as_uint(a2), 0x07060302u);
}
