// The post-pool stage of a fused level, shared by the edge block (edgeblock.hip) and the xyz block (xyzblock.hip).
//
// The two edge passes differ (binarized features / coordinates); everything behind the pooling is one computation: the BatchNorm
// coefficients of the scalar and the vector set (+ running statistics and counters) with the gate MLP beside them, the apply pass
// that writes the pooled (s, v) and their concatenation slices, optionally with the next level's k-NN table (apply_knn.h), and the
// one-launch tail that does all of it at once (svnet_hip.h: svnet_block_tail_desc).  A block supplies
//   CoefArgs + block_coefs_channel(const CoefArgs&, int c, bool commit, float* out): the inputs of its coefficients and the device
//              function that derives channel c of both sets (the scalar sets differ: integer slices and a pre-BN scale / fp64 slices).
//              CoefArgs has the members the code below reads: stat1, stat_v, E, Os, Ov, g1, b1, rm1, rv1, g2, b2, rm2, rv2, training
//   Math:      the apply functor of apply_knn.h, over pooled extrema of type T
// and instantiates the kernels in its own translation unit (the two are compiled with different flags: Makefile).
#pragma once
#include "common.h"
#include "gate_mlp.h"
#include "apply_knn.h"

namespace {

// coef layout: [A1 (Os) | B1 (Os) | mean_y (Os) | invstd_y (Os) | Av (Ov) | Bv (Ov) | mean' (Ov) | invstd' (Ov)]
//   scalar: y = A1*x + B1 on the pooled extremum x (A1 >= 0 ? max : min), B1 = beta - gamma*mean_y*invstd_y
//   vector: q(n') = Av + Bv/n' with Av = gamma'*invstd', Bv = beta' - gamma'*mean'*invstd'
template <class CoefArgs>
__global__ void block_coeffs_kernel(CoefArgs a, float* __restrict__ coef, long long* __restrict__ nbt1,
                                    long long* __restrict__ nbt2, svnet_gate_fwd_job job, int coef_blocks) {
    if ((int)blockIdx.x >= coef_blocks) { svnet_gate_fwd_block(job, (int)blockIdx.x - coef_blocks); return; }   // the gate MLP beside the coefficients
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && a.training) {
        if (nbt1) *nbt1 += 1;
        if (nbt2) *nbt2 += 1;
    }
    block_coefs_channel(a, c, true, coef);
}

// Pooled outputs: s_out = Math::s, v_out = Math::v.  (One functor per block for the three kernels below: the same expressions, so the
// same contraction - their outputs are bit-identical, tests/test_hip_fused.py)
template <class Math, typename T>
__global__ __launch_bounds__(256) void block_apply_kernel(const T* __restrict__ hi, const T* __restrict__ lo, const float* __restrict__ mv,
                                                          const float* __restrict__ mvn, const float* __restrict__ coef,
                                                          const float* __restrict__ gate, int64_t P, int64_t N, int Os, int Ov, float slope,
                                                          float* __restrict__ s_out, float* __restrict__ v_out, float* __restrict__ s_cat,
                                                          int64_t s_ld, float* __restrict__ v_cat, int64_t v_ld) {
    const Math m = {hi, lo, mv, mvn, coef, coef + Os, coef + 4 * Os, coef + 4 * Os + Ov, gate, Os, Ov, slope};
    // a wave per point row: lanes over the Os scalar channels, then over the 3*Ov vector entries - no per-element divisions (the flat
    // e -> (e % Os, q % Ov, q / 3Ov, p / N) form spent four 64-bit divisions on every output)
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t p = wave0; p < P; p += nwaves) {
        const int64_t b = p / N;
        for (int o = lane; o < Os; o += 64) {
            const float z = m.s(p, o);
            s_out[p * Os + o] = z;
            if (s_cat) s_cat[p * s_ld + o] = z;            // (the level's column slice of the pyramid's concatenation, written in place)
        }
        for (int q = lane; q < 3 * Ov; q += 64) {
            const int dd = q >= 2 * Ov ? 2 : (q >= Ov ? 1 : 0), c = q - dd * Ov;
            const float z = m.v(p, b, q, c);
            v_out[p * 3 * Ov + q] = z;
            if (v_cat) v_cat[(p * 3 + dd) * v_ld + c] = z;
        }
    }
}

// ... and the same pass preparing the k-NN table of its output (apply_knn.h)
template <class Math, typename T>
__global__ __launch_bounds__(256) void block_apply_knn_kernel(const T* __restrict__ hi, const T* __restrict__ lo, const float* __restrict__ mv,
                                                              const float* __restrict__ mvn, const float* __restrict__ coef,
                                                              const float* __restrict__ gate, int64_t P, int64_t N, int Os, int Ov,
                                                              float slope, float* __restrict__ s_out, float* __restrict__ v_out,
                                                              float* __restrict__ s_cat, int64_t s_ld, float* __restrict__ v_cat, int64_t v_ld,
                                                              float* __restrict__ xT, float* __restrict__ xx, int64_t Cpad) {
    extern __shared__ float apply_knn_rows[];
    const Math m = {hi, lo, mv, mvn, coef, coef + Os, coef + 4 * Os, coef + 4 * Os + Ov, gate, Os, Ov, slope};
    apply_knn_tiles<APPLY_KNN_TP>(m, P, N, Os, Ov, s_out, v_out, s_cat, s_ld, v_cat, v_ld, xT, xx, Cpad, apply_knn_rows);
}

// ---- coefficients + gate MLP + apply (+ the next k-NN's table) in one launch (svnet_hip.h: svnet_block_tail_desc).  A workgroup = one
// tile of APPLY_KNN_TP points of cloud b: its 256 threads derive the coefficients into LDS (thread c: channel c of both sets, as the
// coefficient kernel's threads do), run cloud b's gate MLP (every workgroup of the cloud writes the same h / gin / gate values), then the
// apply pass reads both from there.  Workgroup 0 alone commits: coef, running statistics, counters.
template <class CoefArgs, class Math, typename T>
__global__ __launch_bounds__(256) void block_tail_kernel(CoefArgs ca, float* __restrict__ coef, long long* __restrict__ nbt1,
                                                         long long* __restrict__ nbt2, svnet_gate_fwd_job job, const T* __restrict__ hi,
                                                         const T* __restrict__ lo, const float* __restrict__ mv, const float* __restrict__ mvn,
                                                         int64_t P, int64_t N, float slope, float* __restrict__ s_out, float* __restrict__ v_out,
                                                         float* __restrict__ s_cat, int64_t s_ld, float* __restrict__ v_cat, int64_t v_ld,
                                                         float* __restrict__ xT, float* __restrict__ xx, int64_t Cpad) {
    extern __shared__ float tail_lds[];                                  // [coef: 4 Os + 4 Ov (rounded to 4) | the tile's rows]
    const int Os = ca.Os, Ov = ca.Ov;
    const int ncoef = (4 * Os + 4 * Ov + 3) & ~3;
    const bool first = blockIdx.x == 0;
    const int64_t b = ((int64_t)blockIdx.x * APPLY_KNN_TP) / N;
    if (first && threadIdx.x == 0 && ca.training) {
        if (nbt1) *nbt1 += 1;
        if (nbt2) *nbt2 += 1;
    }
    block_coefs_channel(ca, (int)threadIdx.x, first, tail_lds);
    svnet_gate_fwd_block(job, (int)b);
    __syncthreads();                                                     // the coefficients in LDS, the cloud's gate in global memory
    if (first)
        for (int i = threadIdx.x; i < 4 * Os + 4 * Ov; i += blockDim.x) coef[i] = tail_lds[i];
    const Math m = {hi, lo, mv, mvn, tail_lds, tail_lds + Os, tail_lds + 4 * Os, tail_lds + 4 * Os + Ov, job.gate, Os, Ov, slope};
    apply_knn_tiles<APPLY_KNN_TP>(m, P, N, Os, Ov, s_out, v_out, s_cat, s_ld, v_cat, v_ld, xT, xx, Cpad, tail_lds + ncoef);
}

// ---- the host side of the four entry points of a block.  who: the entry point's name, kernel: the name its launch is reported
// under; the extern "C" functions of the two blocks forward here.
template <class CoefArgs>
int block_coeffs_launch(const char* who, const char* kernel, const CoefArgs& ca, int64_t Os, int64_t Ov, float* coef, int64_t* num_batches_tracked1,
                        int64_t* num_batches_tracked2, const svnet_gate_fwd_job* gate_job, void* stream) {
    SVNET_REQUIRE(ca.g1 && ca.b1 && ca.g2 && ca.b2 && coef && ca.E > 0 && Os > 0 && Ov > 0, SVNET_E_ARG, "%s: bad arguments", who);
    SVNET_REQUIRE(ca.training ? (ca.stat1 && ca.stat_v) : (ca.rm1 && ca.rv1 && ca.rm2 && ca.rv2), SVNET_E_ARG, "%s: missing statistics", who);
    const int64_t n = Os > Ov ? Os : Ov;
    SVNET_REQUIRE(!gate_job || svnet_gate_fwd_job_ok(gate_job), SVNET_E_ARG, "%s: bad gate job", who);
    const int coef_blocks = (int)svnet_cdiv(n, 256);
    const svnet_gate_fwd_job job = gate_job ? *gate_job : svnet_gate_fwd_job{};
    hipLaunchKernelGGL(block_coeffs_kernel<CoefArgs>, dim3((unsigned)(coef_blocks + (gate_job ? gate_job->B : 0))), dim3(256), 0,
                       (hipStream_t)stream, ca, coef, reinterpret_cast<long long*>(num_batches_tracked1),
                       reinterpret_cast<long long*>(num_batches_tracked2), job, coef_blocks);
    SVNET_CHECK_LAUNCH(kernel);
    return SVNET_OK;
}

template <class Math, typename T>
int block_apply_launch(const char* who, const char* kernel, const T* hi, const T* lo, const float* mv, const float* mvn, const float* coef,
                       const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope, float* s_out, float* v_out, float* s_cat,
                       int64_t s_ld, float* v_cat, int64_t v_ld, void* stream) {
    SVNET_REQUIRE(hi && lo && mv && mvn && coef && gate && s_out && v_out && P >= 0 && N > 0, SVNET_E_ARG, "%s: bad arguments", who);
    SVNET_REQUIRE((!s_cat || s_ld >= Os) && (!v_cat || v_ld >= Ov), SVNET_E_ARG, "%s: concatenation row shorter than the slice", who);
    if (P == 0) return SVNET_OK;
    hipLaunchKernelGGL((block_apply_kernel<Math, T>), dim3(svnet_grid(P * 64, 256, 256 * 8)), dim3(256), 0, (hipStream_t)stream, hi, lo, mv, mvn,
                       coef, gate, P, N, (int)Os, (int)Ov, slope, s_out, v_out, s_cat, s_ld, v_cat, v_ld);
    SVNET_CHECK_LAUNCH(kernel);
    return SVNET_OK;
}

template <class Math, typename T>
int block_apply_knn_launch(const char* who, const char* kernel, const T* hi, const T* lo, const float* mv, const float* mvn,
                           const float* coef, const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope, float* s_out,
                           float* v_out, float* s_cat, int64_t s_ld, float* v_cat, int64_t v_ld, void* knn_workspace,
                           size_t knn_workspace_bytes, void* stream) {
    SVNET_REQUIRE(hi && lo && mv && mvn && coef && gate && s_out && v_out && knn_workspace && P > 0 && N > 0 && P % N == 0, SVNET_E_ARG,
                  "%s: bad arguments", who);
    SVNET_REQUIRE((!s_cat || s_ld >= Os) && (!v_cat || v_ld >= Ov), SVNET_E_ARG, "%s: concatenation row shorter than the slice", who);
    int64_t Cpad = 0;
    SVNET_REQUIRE(apply_knn_supported(P, N, Os, Ov, &Cpad), SVNET_E_UNSUPPORTED,
                  "%s: N=%lld, Os=%lld, Ov=%lld not supported (ask svnet_knn_table_fusable first)", who, (long long)N, (long long)Os,
                  (long long)Ov);
    SVNET_REQUIRE(knn_workspace_bytes >= svnet_knn_workspace_bytes(P / N, N, Os + 3 * Ov), SVNET_E_WORKSPACE, "%s: k-NN workspace too small", who);
    float* xT = (float*)knn_workspace;
    float* xx = xT + P * ((Os + 3 * Ov + 7) / 8 * 8);
    hipLaunchKernelGGL((block_apply_knn_kernel<Math, T>), dim3((unsigned)(P / APPLY_KNN_TP)), dim3(256), apply_knn_lds_bytes(Os, Ov),
                       (hipStream_t)stream, hi, lo, mv, mvn, coef, gate, P, N, (int)Os, (int)Ov, slope, s_out, v_out, s_cat, s_ld, v_cat, v_ld,
                       xT, xx, Cpad);
    SVNET_CHECK_LAUNCH(kernel);
    return SVNET_OK;
}

// the checks of a tail launch; returns its dynamic LDS bytes through *lds and the table pointers
inline int block_tail_check(const svnet_block_tail_desc& d, const char* who, size_t* lds, float** xT, float** xx, int64_t* Cpad) {
    SVNET_REQUIRE(d.hi && d.lo && d.mv && d.mvn && d.coef && d.s_out && d.v_out && d.gamma1 && d.beta1 && d.gamma2 && d.beta2, SVNET_E_ARG,
                  "%s: null pointer", who);
    SVNET_REQUIRE(d.training ? (d.stat1 && d.stat_v) : (d.running_mean1 && d.running_var1 && d.running_mean2 && d.running_var2), SVNET_E_ARG,
                  "%s: missing statistics", who);
    SVNET_REQUIRE(svnet_gate_fwd_job_ok(&d.gate) && d.gate.Ov == d.Ov && d.gate.B * d.N == d.P, SVNET_E_ARG, "%s: bad gate job", who);
    SVNET_REQUIRE((!d.s_cat || d.s_ld >= d.Os) && (!d.v_cat || d.v_ld >= d.Ov), SVNET_E_ARG, "%s: concatenation row shorter than the slice", who);
    SVNET_REQUIRE(svnet_block_tail_supported(d.P, d.N, d.Os, d.Ov, d.knn_workspace != nullptr), SVNET_E_UNSUPPORTED,
                  "%s: P=%lld N=%lld Os=%lld Ov=%lld not supported (svnet_block_tail_supported)", who, (long long)d.P, (long long)d.N,
                  (long long)d.Os, (long long)d.Ov);
    *xT = nullptr; *xx = nullptr; *Cpad = 0;
    if (d.knn_workspace) {
        SVNET_REQUIRE(d.knn_workspace_bytes >= svnet_knn_workspace_bytes(d.P / d.N, d.N, d.Os + 3 * d.Ov), SVNET_E_WORKSPACE,
                      "%s: k-NN workspace too small", who);
        apply_knn_supported(d.P, d.N, d.Os, d.Ov, Cpad);
        *xT = (float*)d.knn_workspace;
        *xx = *xT + d.P * ((d.Os + 3 * d.Ov + 7) / 8 * 8);
    }
    *lds = block_tail_lds_bytes(d.Os, d.Ov, d.knn_workspace != nullptr);
    return SVNET_OK;
}

// ca: the block's coefficient inputs, taken from the descriptor by its entry point
template <class Math, typename T, class CoefArgs>
int block_tail_launch(const char* who, const char* kernel, const svnet_block_tail_desc& d, const CoefArgs& ca, void* stream) {
    size_t lds; float* xT; float* xx; int64_t Cpad;
    const int rc = block_tail_check(d, who, &lds, &xT, &xx, &Cpad);
    if (rc != SVNET_OK) return rc;
    hipLaunchKernelGGL((block_tail_kernel<CoefArgs, Math, T>), dim3((unsigned)(d.P / APPLY_KNN_TP)), dim3(256), lds, (hipStream_t)stream, ca,
                       d.coef, reinterpret_cast<long long*>(d.num_batches_tracked1), reinterpret_cast<long long*>(d.num_batches_tracked2), d.gate,
                       (const T*)d.hi, (const T*)d.lo, d.mv, d.mvn, d.P, d.N, d.slope, d.s_out, d.v_out, d.s_cat, d.s_ld, d.v_cat, d.v_ld, xT,
                       xx, Cpad);
    SVNET_CHECK_LAUNCH(kernel);
    return SVNET_OK;
}

}  // namespace
