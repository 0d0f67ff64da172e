// Wave-level primitives of the gfx950 kernels, each stated once: DPP moves, the row / half swaps, the sums and arg-max butterflies built
// from them, a lane's rank in a ballot, and the order-preserving float keys.  CDNA4 only: wave = 64 lanes = 4 rows of 16.  Included by common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifdef __HIPCC__
__device__ __forceinline__ int lane_id() { return (int)(threadIdx.x & 63); }

// ---- DPP moves.  Controls whose every lane has a source (quad_perm, row_ror, the mirrors) and full-row-mask shifts run with
// bound_ctrl: the `old` operand is then dead and the DPP read folds into the consuming instruction instead of costing a v_mov for
// `old` plus a v_mov_dpp.  A partial ROW_MASK keeps `old` (= 0) in the rows it leaves out.
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_ROR4 = 0x124, DPP_ROW_ROR8 = 0x128, DPP_ROW_ROR12 = 0x12C,
              DPP_ROW_MIRROR = 0x140, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;
template <int CTRL, int ROW_MASK = 0xF>
__device__ __forceinline__ float svnet_dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, ROW_MASK == 0xF));
}
template <int CTRL>
__device__ __forceinline__ uint32_t svnet_dpp_u32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, true);
}

// ---- value of lane (l ^ S) without the LDS crossbar: DPP modifiers inside a 16-lane row, the gfx950 row / half swaps across rows
// (__shfl_xor is a ds_bpermute, a ~100-cycle LDS round trip: a bitonic sort is a chain of 21 dependent exchanges)
__device__ __forceinline__ uint32_t lane_half_swap(uint32_t x) {      // S = 32
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (threadIdx.x & 32) ? r[0] : r[1];
}
__device__ __forceinline__ float lane_half_swap(float x) { return __uint_as_float(lane_half_swap(__float_as_uint(x))); }
template <int S>
__device__ __forceinline__ uint32_t svnet_lane_xor_u32(uint32_t x, int lane) {
    if (S == 1) return svnet_dpp_u32<DPP_QUAD_1032>(x);
    if (S == 2) return svnet_dpp_u32<DPP_QUAD_2301>(x);
    if (S == 4) {                                                    // row_ror:4 reads lane l-4, row_ror:12 lane l+4 (mod 16): keep l ^ 4
        const uint32_t a = svnet_dpp_u32<DPP_ROW_ROR4>(x), b = svnet_dpp_u32<DPP_ROW_ROR12>(x);
        return (lane & 4) ? a : b;
    }
    if (S == 8) return svnet_dpp_u32<DPP_ROW_ROR8>(x);
    if (S == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
        return (lane & 16) ? r[0] : r[1];
    }
    const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
    return (lane & 32) ? r[0] : r[1];
}

// ---- sums.  fold32: the wave sum of a (lanes 0..31 of the result) and of b (lanes 32..63), each still spread over its 32 lanes;
// fold16: rows 0..3 of the result are a.row0+a.row1 | b.row0+b.row1 | a.row2+a.row3 | b.row2+b.row3
__device__ __forceinline__ float fold32(float a, float b) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float fold16(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// Sums over groups of G consecutive lanes (G = 4 .. 64), every lane of a group ending up with its group's sum: the steps inside a
// row are DPP operand modifiers of the adds themselves, the two steps across rows the row / half swaps.
template <int G>
__device__ __forceinline__ float group_sum_dpp(float v) {
    static_assert(G == 1 || G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "group size");
    if (G >= 4) {
        v += svnet_dpp_f32<DPP_QUAD_1032>(v);
        v += svnet_dpp_f32<DPP_QUAD_2301>(v);
    }
    if (G >= 8) v += svnet_dpp_f32<DPP_ROW_HALF_MIRROR>(v);   // the other quad of the 8
    if (G >= 16) v += svnet_dpp_f32<DPP_ROW_MIRROR>(v);       // the other half of the row
    if (G >= 32) v = fold16(v, v);                            // rows 0+1 | 0+1 | 2+3 | 2+3
    if (G >= 64) v = fold32(v, v);
    return v;
}
__device__ __forceinline__ float wave_sum(float v) { return group_sum_dpp<64>(v); }
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// Eight wave-wide sums in 18 VALU instructions: every lane of the 8-lane group g = lane >> 3 ends up with the sum over the
// wave of s[bitreverse3(g)]  (groups 0..7 hold s0, s4, s2, s6, s1, s5, s3, s7).
__device__ __forceinline__ float wave_sum8_packed(const float (&s)[8], int lane) {
    const float x0 = fold16(fold32(s[0], s[1]), fold32(s[2], s[3]));   // rows: s0 | s2 | s1 | s3
    const float x1 = fold16(fold32(s[4], s[5]), fold32(s[6], s[7]));   // rows: s4 | s6 | s5 | s7
    const bool hi = (lane & 8) != 0;
    float y = (hi ? x1 : x0) + svnet_dpp_f32<DPP_ROW_ROR8>(hi ? x0 : x1);
    y += svnet_dpp_f32<DPP_QUAD_1032>(y);
    y += svnet_dpp_f32<DPP_QUAD_2301>(y);
    y += svnet_dpp_f32<DPP_ROW_HALF_MIRROR>(y);
    return y;
}
// wave-wide sum, valid in lane 63
__device__ __forceinline__ float wave_sum_last(float v) {
    v += svnet_dpp_f32<DPP_QUAD_1032>(v);
    v += svnet_dpp_f32<DPP_QUAD_2301>(v);
    v += svnet_dpp_f32<DPP_ROW_HALF_MIRROR>(v);
    v += svnet_dpp_f32<DPP_ROW_MIRROR>(v);
    v += svnet_dpp_f32<DPP_ROW_BCAST15, 0xA>(v);
    v += svnet_dpp_f32<DPP_ROW_BCAST31, 0xC>(v);
    return v;
}

// ---- rank of a lane among the set lanes of a ballot: the number of set bits of `mask` BELOW this lane (v_mbcnt_lo + v_mbcnt_hi).
// With mask = __ballot(keep), found + lanes_below(mask) is the slot of a kept lane in a list the wave appends to in lane order.
__device__ __forceinline__ int lanes_below(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- ballot of a comparison over the lanes of `lane_mask` (a wave-uniform word, taken once per kernel as the ballot of the lane
// predicate: never as (1ull << n) - 1, which is undefined at n = 64).  __ballot(in_lane && cmp) materialises its predicate: v_cmp,
// s_and_b64 with the lane predicate's mask, then v_cndmask_b32 v, 0, 1 and v_cmp_ne_u32 0, v to turn the bool back into a mask - two
// VALU instructions per ballot for nothing.  The ballot of the raw comparison is the v_cmp's own result, and the AND runs on the
// scalar unit.  Equal to __ballot(in_lane && cmp) only where every lane of the wave is active: call it in wave-uniform control flow
// with a full exec mask (an inactive lane contributes 0 to a ballot, but its bit of lane_mask was taken when it was active).
__device__ __forceinline__ uint64_t wave_ballot_masked(bool cmp, uint64_t lane_mask) { return __builtin_amdgcn_ballot_w64(cmp) & lane_mask; }

// ---- (value, index) ranking: "a ranks before b" = larger value first, equal values -> smaller index first
__device__ __forceinline__ bool ranks_before(float va, int ja, float vb, int jb) { return (va > vb) | ((va == vb) & (ja < jb)); }   // (bitwise: selects, not branches)
// the same for values that may be NaN (torch.argmax: a NaN is the maximum, the first one wins).  Its own name, not an overload: a
// caller with int indices would silently get the NaN-blind rule.
__device__ __forceinline__ bool ranks_before_nan_first(float a, int64_t ia, float b, int64_t ib) {
    const bool na = a != a, nb = b != b;
    if (na != nb) return na;
    if (!na && a != b) return a > b;
    return ia < ib;
}
// first-ranked (value, index) pair among groups of G consecutive lanes, in every lane of the group
template <int S>
__device__ __forceinline__ void argmax_step(float& v, int& i, int lane) {
    const float ov = __uint_as_float(svnet_lane_xor_u32<S>(__float_as_uint(v), lane));
    const int oi = (int)svnet_lane_xor_u32<S>((uint32_t)i, lane);
    const bool take = ranks_before(ov, oi, v, i);
    v = take ? ov : v;
    i = take ? oi : i;
}
template <int G>
__device__ __forceinline__ void argmax_group(float& v, int& i, int lane) {
    if (G >= 2) argmax_step<1>(v, i, lane);
    if (G >= 4) argmax_step<2>(v, i, lane);
    if (G >= 8) argmax_step<4>(v, i, lane);
    if (G >= 16) argmax_step<8>(v, i, lane);
    if (G >= 32) argmax_step<16>(v, i, lane);
    if (G >= 64) argmax_step<32>(v, i, lane);
}

// ---- order-preserving keys.  ord_bits maps a float's bit pattern to a uint32 whose unsigned order is the float order; ord_key first
// makes -0 a +0, so that equal floats have equal keys, and ord_val is its inverse.  pack_key is the 64-bit composite whose unsigned
// maximum (atomicMax) is the largest value and, among equal values, the lowest row; it keeps the sign of a zero.  unpack_key is its inverse.
__device__ __forceinline__ uint32_t ord_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t ord_key(float v) { return ord_bits(__float_as_uint(v + 0.f)); }
__device__ __forceinline__ float ord_val(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}
__device__ __forceinline__ unsigned long long pack_key(float v, int64_t r) {
    return ((unsigned long long)ord_bits(__float_as_uint(v)) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)r);
}
__device__ __forceinline__ void unpack_key(unsigned long long key, float& v, int32_t& r) {
    v = ord_val((uint32_t)(key >> 32));
    r = (int32_t)(0xFFFFFFFFu - (uint32_t)key);
}

// ---- 32 x 32 bit-matrix transpose across 32 consecutive lanes (both halves of the wave at once): lane r of a half holds row r
// (bit b = element [r][b]); afterwards lane b holds column b (bit r = element [r][b]).  Five butterfly stages of ~7 instructions
// (swap the off-diagonal J x J blocks of every 2J x 2J block) instead of 32 ballots + selects.
template <int J>
__device__ __forceinline__ uint32_t svnet_bt_stage(uint32_t x, int lane) {
    constexpr uint32_t MLO = J == 16 ? 0x0000FFFFu : J == 8 ? 0x00FF00FFu : J == 4 ? 0x0F0F0F0Fu : J == 2 ? 0x33333333u : 0x55555555u;
    const uint32_t p = svnet_lane_xor_u32<J>(x, lane);
    const bool lower = (lane & J) != 0;
    const uint32_t keep = lower ? (x & ~MLO) : (x & MLO);
    const uint32_t take = lower ? ((p >> J) & MLO) : ((p & MLO) << J);
    return keep | take;
}
__device__ __forceinline__ uint32_t svnet_bit_transpose32(uint32_t x, int lane) {
    x = svnet_bt_stage<16>(x, lane);
    x = svnet_bt_stage<8>(x, lane);
    x = svnet_bt_stage<4>(x, lane);
    x = svnet_bt_stage<2>(x, lane);
    return svnet_bt_stage<1>(x, lane);
}
#endif
