// Shared helpers for the gfx950 kernels of libsvnet_hip.so.  CDNA4 only: wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "../../include/svnet_hip.h"

#define SVNET_WAVE 64

// The range of the k-NN's bit-exact contract (knn.hip): past it the streamed form's limits (ids are 32-bit keys; a list holds 128)
// and MKL's K blocking.  SVNET_KNN_MAX_N is also the limit on the points of a cloud in propagate.hip and group.hip.
#define SVNET_KNN_MAX_N 32768
#define SVNET_KNN_MAX_K 128
#define SVNET_KNN_MAX_C 384

void svnet_set_error(const char* fmt, ...);

#define SVNET_REQUIRE(cond, code, ...)        \
    do {                                      \
        if (!(cond)) {                        \
            svnet_set_error(__VA_ARGS__);     \
            return (code);                    \
        }                                     \
    } while (0)

#define SVNET_CHECK_LAUNCH(name)                                                   \
    do {                                                                           \
        hipError_t e_ = hipGetLastError();                                         \
        if (e_ != hipSuccess) {                                                    \
            svnet_set_error("%s: launch failed: %s", name, hipGetErrorString(e_)); \
            return SVNET_E_LAUNCH;                                                 \
        }                                                                          \
    } while (0)

static inline int64_t svnet_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// More than 64 KiB of dynamic LDS needs an explicit opt-in, and hipFuncSetAttribute applies to the CURRENT device only: one bit per
// device ordinal and call site (a process that touches a second GPU opts in there too), atomic (two host threads may race: the call is
// idempotent), and the hipError_t is reported instead of dropped - the message of the launch failure that follows would not name it.
static inline bool svnet_lds_optin(std::atomic<uint64_t>& done, const void* const* fns, int nf, int bytes, const char* name) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) {
        const uint64_t bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return true;
        for (int i = 0; i < nf && e == hipSuccess; ++i) e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) { done.fetch_or(bit, std::memory_order_release); return true; }
    }
    svnet_set_error("%s: cannot opt in to %d bytes of dynamic LDS on device %d: %s", name, bytes, dev, hipGetErrorString(e));
    return false;
}
// SVNET_LDS_OPTIN(ok, bytes, name, kernel, ...): ok = false (and svnet_last_error set) when the opt-in failed on this device
#define SVNET_LDS_OPTIN(ok, bytes, name, ...)                                                                 \
    do {                                                                                                      \
        static std::atomic<uint64_t> done_{0};                                                                \
        const void* const fns_[] = {__VA_ARGS__};                                                             \
        (ok) = svnet_lds_optin(done_, fns_, (int)(sizeof(fns_) / sizeof(fns_[0])), (int)(bytes), name);       \
    } while (0)

// Grid for memory-bound grid-stride kernels: enough blocks to fill 256 CUs x 8, capped.
static inline unsigned svnet_grid(int64_t work_items, int block, int64_t cap = 256 * 16) {
    int64_t g = svnet_cdiv(work_items, block);
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// Floats per row of the fused edge block's backward message table [dn (Cs) | dve (3 Cv) | dz (9)], rounded up to whole float4s.
template <typename T>
__host__ __device__ inline T msg_stride(T Cs, T Cv, T Ov) { (void)Ov; return ((Cs + 3 * Cv + 9) + 3) / 4 * 4; }

#include "wave.h"

#ifdef __HIPCC__
// ---- grid-wide column sums without a thousand adders per address.  A reduction kernel used to end in one atomic per output per
// workgroup onto the SAME L addresses; same-address atomics are served one after the other at the memory side (~2.5 ns each per cache
// line, measured: 512 workgroups x 340 doubles = 12 us of a 39 us kernel, the float reductions twice that), and removing them from
// the BatchNorm / VectorBN reductions of one step was worth 0.065 ms.  Now the caller's (zero-filled) buffer holds
//   [L result | SVNET_RED_SLICES x L slices | 2 spare]               (SVNET_SLICED_LEN(L) elements, svnet_hip.h)
// workgroup w adds to slice w % SVNET_RED_SLICES and NOTHING else happens in the reducing kernel: the slices are added up by the
// kernel that consumes the sums (svnet_slices_total: bn_finalize / vbn_fwd / the *_bwd_apply kernels, each of which also leaves the
// totals in the first L elements), or by svnet_slices_sum_* where no such kernel follows.  The hand-off between the adders and the
// reader is therefore a KERNEL BOUNDARY on one stream - the only inter-workgroup ordering HIP guarantees without a protocol.
// (Round 3 summed the slices in the reducing kernel's last workgroup to arrive, ordered by returning atomics + an arrival counter;
//  one run of its no-return form lost a share.  The memory-model-conforming form of that hand-off - an agent-scope release fence by
//  one thread per workgroup in front of the counter add, an acquire fence in the last arriver - measured +0.05 ms per step
//  (4.657 against 4.606 ms, three alternating runs on one box, gpurun_out/r04_ab_slices.log); this form needs no hand-off at all.)
template <typename T>
__device__ __forceinline__ T* svnet_slice_ptr(T* buf, int L) {
    const unsigned w = blockIdx.x + blockIdx.y * gridDim.x;
    return buf + (size_t)L * (1u + (w & (SVNET_RED_SLICES - 1)));
}
template <typename T>
__device__ __forceinline__ void svnet_slice_add(T* p, T v) { atomicAdd(p, v); }
// Sum i of a sliced accumulator a PREVIOUS kernel of the stream filled (fixed order: bit-reproducible for a given set of slice values).
template <typename T>
__device__ __forceinline__ T svnet_slices_total(const T* buf, int L, int i) {
    T s = 0;
#pragma unroll
    for (int sl = 0; sl < SVNET_RED_SLICES; ++sl) s += buf[(size_t)L * (1 + sl) + i];
    return s;
}

// Single-instruction square root / reciprocal (v_sqrt_f32, v_rcp_f32: 1 ulp each) for the per-edge vector norms of the fused
// kernels, where the correctly rounded sequences (10 instructions each) were a fifth of the instruction stream.
__device__ __forceinline__ float fast_sqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// Activation of the BatchNorm kernels and its derivative: act 0 = none, 1 = LeakyReLU(slope), 2 = ReLU
__device__ __forceinline__ float act_apply(float z, int act, float slope) {
    if (act == 1) return z > 0.f ? z : z * slope;
    if (act == 2) return z > 0.f ? z : 0.f;
    return z;
}
__device__ __forceinline__ float act_grad(float z, int act, float slope) {
    if (act == 1) return z > 0.f ? 1.f : slope;
    if (act == 2) return z > 0.f ? 1.f : 0.f;
    return 1.f;
}

// Ternary dot product of two bit-plane words (sign plane s, non-zero plane z; 64 or 32 bits wide) of the fused edge block.
__device__ __forceinline__ int popcw(uint64_t x) { return __popcll(x); }
__device__ __forceinline__ int popcw(uint32_t x) { return __popc(x); }
template <typename W>
__device__ __forceinline__ int tdot(W xs, W xz, W ws, W wz) {
    const W m = xz & wz;
    return popcw(m) - 2 * popcw(m & (xs ^ ws));
}
// The same product as two running popcounts, pm += popc(m), pd += popc(m & (xs ^ ws)): v_bcnt_u32_b32 adds into its third operand
// for free, so a row of words costs one "pm - 2*pd" instead of a subtract-and-add per word.
template <typename W>
__device__ __forceinline__ void tacc(W xs, W xz, W ws, W wz, int& pm, int& pd) {
    const W m = xz & wz;
    pm += popcw(m);
    pd += popcw(m & (xs ^ ws));
}
// DENSE weights (no exact zero in W1: *w_dense, set by svnet_edgeblock_prepare_f32): the mask of a product is the edge's own non-zero plane,
// so popc(m) is ONE wave-uniform count per edge (scalar unit) and a word costs xor + and + bcnt instead of and + bcnt + xor + and + bcnt:
// 40 % fewer instructions in the half of the kernel that is popcounts.  Same integer, bit for bit.
template <typename W>
__device__ __forceinline__ void tacc_dense(W xs, W xz, W ws, int& pd) { pd += popcw(xz & (xs ^ ws)); }

// A float at wave-uniform `base` + per-lane BYTE offset, loaded with the SGPR-base addressing mode (global_load v, voff, s[base]).
// The empty asm keeps the 32->64-bit extension of the lane offset next to the load: once it is hoisted out of a loop, instruction
// selection no longer sees it and falls back to a 64-bit VALU add per load.
__device__ __forceinline__ uint32_t keep_here(uint32_t x) { asm volatile("" : "+v"(x)); return x; }
__device__ __forceinline__ float ld_f32_sbase(const float* base, uint32_t byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + keep_here(byte_off));
}
// The same for a lane offset that is formed inside the loop (nothing to hoist): without keep_here, whose "+v" costs a v_mov_b32 per load
// whenever its operand lives on.
__device__ __forceinline__ float ld_f32_sbase_fresh(const float* base, uint32_t byte_off) {
    return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(base) + byte_off);
}
__device__ __forceinline__ int16_t ld_i16_sbase(const int16_t* base, uint32_t byte_off) {
    return *reinterpret_cast<const int16_t*>(reinterpret_cast<const char*>(base) + keep_here(byte_off));
}
__device__ __forceinline__ void st_f32_sbase(float* base, uint32_t byte_off, float v) {
    *reinterpret_cast<float*>(reinterpret_cast<char*>(base) + keep_here(byte_off)) = v;
}
__device__ __forceinline__ void st_i16_sbase_fresh(int16_t* base, uint32_t byte_off, int16_t v) {
    *reinterpret_cast<int16_t*>(reinterpret_cast<char*>(base) + byte_off) = v;
}
__device__ __forceinline__ void st_u64_sbase_fresh(uint64_t* base, uint32_t byte_off, uint64_t v) {
    *reinterpret_cast<uint64_t*>(reinterpret_cast<char*>(base) + byte_off) = v;
}

#endif
