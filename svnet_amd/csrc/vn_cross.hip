// Fused vector-neuron position level for inference: the eval-mode forward of a VNLinearLeakyReLU over 3 -> O vector channels
// (models/vn_layers.py:50-78) on the edge feature [x_j - x_i | x_i | x_j x x_i] of get_graph_feature_cross (models/utils/vn_util.py:52-76)
// followed by mean_pool over the k neighbours - the first level of models/vn_pointnet_cls.py - as a fold and one launch that writes 3 O
// floats per point and nothing else.  The contract is in include/svnet_hip.h ("fused vector-neuron cross edge level") and
// svnet_amd/vn_pointnet.py; tests/vn_pointnet_ref.py restates it.
//
// The cross product depends on the pair, so the level is not linear in a per-point table and vn_edge.hip's tables cannot take it; but
// its input is one vector channel, so an edge is nine floats and a channel's product is three fmaf per component.  Two kernels:
//   vn_cross_fold_kernel  W = [W_f | W_d] stacked as the rows lie, [O + Od][3], and BatchNorm's running statistics folded into s, t [O].
//   vn_cross_kernel       grid (ceil(N / 64), ceil(O / VX_CH), B), one wave per workgroup.  A lane takes a point n, so the loads of the
//                         centre and the stores to out[b,o,a,n] run along n; the wave takes VX_CH = 8 consecutive output channels,
//                         whose 8 x (3 + 3 + 2) weights, s and t are the same in every lane (the addresses come from blockIdx alone:
//                         scalar loads, scalar registers).  The lane walks its k neighbours: the id is clamped before any address
//                         is formed, the edge's nine feature values are computed once and every channel of the chunk is applied to
//                         them; the 3 x 8 running sums stay in registers for every O.  The edge values are recomputed per chunk,
//                         nine operations against the hundred and more of a channel's non-linearity.  No LDS, no barrier.
// Built with -ffp-contract=off (Makefile, NO_CONTRACT): every product, sum, quotient and square root is its own correctly rounded fp32
// operation.  The fold of the statistics and the norm / leaky rule are vn_math.h's, shared with vn_edge.hip and vn_tail.hip.  No atomics.
#include "vn_math.h"

namespace {

constexpr int VX_THREADS = 64;          // one wave: lanes along n
constexpr int VX_CH = 8;                // output channels per wave: 24 running sums per lane
constexpr int VX_MAX_K = 64, VX_MAX_O = 128, VX_MAX_B = 65535;      // the envelope (svnet_vn_cross_supported)

inline bool vx_ok(int64_t N, int64_t k, int64_t O, int64_t Od) {
    return k >= 1 && k <= VX_MAX_K && N >= k && N <= VN_MAX_N && O >= 1 && O <= VX_MAX_O && vn_dir_rows_ok(O, Od);
}

// e over [3 (O + Od) | O]: the rows of [W_f | W_d] as they lie; then s and t
__global__ __launch_bounds__(256) void vn_cross_fold_kernel(const float* __restrict__ wf, const float* __restrict__ wd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ rmean,
                                                            const float* __restrict__ rvar, int O, int Od, float eps, float* __restrict__ folded) {
    const int WR = 3 * (O + Od);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < WR) {
        folded[e] = e < 3 * O ? wf[e] : wd[e - 3 * O];
    } else if (e < WR + O) {
        const int o = e - WR;
        vn_bn_fold(gamma[o], beta[o], rmean[o], rvar[o], eps, folded[WR + o], folded[WR + O + o]);
    }
}

// one row of W on the three feature vectors of an edge: acc = +0, then fmaf over c = 0, 1, 2
__device__ __forceinline__ float vx_row(float e0, float e1, float e2, const float (&w)[3]) { return fmaf(e2, w[2], fmaf(e1, w[1], fmaf(e0, w[0], 0.f))); }

// SHARE: one direction row for every channel (Od = 1 < O), computed once per edge.
template <bool SHARE>
__global__ __launch_bounds__(VX_THREADS) void vn_cross_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx, const float* __restrict__ W,
                                                              const float* __restrict__ s, const float* __restrict__ t, int N, int k, int O, float slope,
                                                              float* __restrict__ out) {
    const int n = blockIdx.x * VX_THREADS + threadIdx.x;
    if (n >= N) return;                                  // (no barrier below)
    const int64_t b = blockIdx.z;
    const int o0 = blockIdx.y * VX_CH;
    // the chunk's weights: a channel past O reads the last one and is not stored
    float wf[VX_CH][3], wd[SHARE ? 1 : VX_CH][3], so[VX_CH], to[VX_CH];
#pragma unroll
    for (int i = 0; i < VX_CH; ++i) {
        const int oc = o0 + i < O ? o0 + i : O - 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            wf[i][c] = W[oc * 3 + c];
            if (!SHARE) wd[i][c] = W[(O + oc) * 3 + c];
        }
        so[i] = s[oc];
        to[i] = t[oc];
    }
    if (SHARE) {
#pragma unroll
        for (int c = 0; c < 3; ++c) wd[0][c] = W[O * 3 + c];
    }
    const float* xb = x + b * 3 * N;                      // x [B][1][3][N]
    const float xi0 = xb[n], xi1 = xb[N + n], xi2 = xb[2 * (int64_t)N + n];
    const int64_t* ib = idx + (b * N + n) * k;
    const float one_minus = 1.f - slope;
    float acc[VX_CH][3];
#pragma unroll
    for (int i = 0; i < VX_CH; ++i) acc[i][0] = acc[i][1] = acc[i][2] = 0.f;
    for (int j = 0; j < k; ++j) {
        const int m = (int)clamp_index(ib[j], N);
        const float xj0 = xb[m], xj1 = xb[N + m], xj2 = xb[2 * (int64_t)N + m];
        // the edge feature's three vectors x_j - x_i, x_i, x_j x x_i: fa[c] is component a of vector c
        const float f0[3] = {xj0 - xi0, xi0, xj1 * xi2 - xj2 * xi1};
        const float f1[3] = {xj1 - xi1, xi1, xj2 * xi0 - xj0 * xi2};
        const float f2[3] = {xj2 - xi2, xi2, xj0 * xi1 - xj1 * xi0};
        float ds0 = 0.f, ds1 = 0.f, ds2 = 0.f;
        if (SHARE) {
            ds0 = vx_row(f0[0], f0[1], f0[2], wd[0]);
            ds1 = vx_row(f1[0], f1[1], f1[2], wd[0]);
            ds2 = vx_row(f2[0], f2[1], f2[2], wd[0]);
        }
#pragma unroll
        for (int i = 0; i < VX_CH; ++i) {
            const float p0 = vx_row(f0[0], f0[1], f0[2], wf[i]);
            const float p1 = vx_row(f1[0], f1[1], f1[2], wf[i]);
            const float p2 = vx_row(f2[0], f2[1], f2[2], wf[i]);
            float d0 = ds0, d1 = ds1, d2 = ds2, y[3];
            if (!SHARE) {
                d0 = vx_row(f0[0], f0[1], f0[2], wd[i]);
                d1 = vx_row(f1[0], f1[1], f1[2], wd[i]);
                d2 = vx_row(f2[0], f2[1], f2[2], wd[i]);
            }
            vn_norm_leaky(p0, p1, p2, d0, d1, d2, so[i], to[i], slope, one_minus, y);
            acc[i][0] += y[0];
            acc[i][1] += y[1];
            acc[i][2] += y[2];
        }
    }
    const float kf = (float)k;
    float* ob = out + b * O * 3 * N + n;                  // out [B][O][3][N]
#pragma unroll
    for (int i = 0; i < VX_CH; ++i) {
        if (o0 + i < O) {
            float* oo = ob + (int64_t)(o0 + i) * 3 * N;
            oo[0] = acc[i][0] / kf;
            oo[N] = acc[i][1] / kf;
            oo[2 * (int64_t)N] = acc[i][2] / kf;
        }
    }
}

}  // namespace

extern "C" int svnet_vn_cross_supported(int64_t N, int64_t k, int64_t O, int64_t Od) { return vx_ok(N, k, O, Od) ? 1 : 0; }

extern "C" int svnet_vn_cross_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                                       const float* running_var, int64_t O, int64_t Od, float eps, float* folded, void* stream) {
    SVNET_REQUIRE(w_feat && w_dir && gamma && beta && running_mean && running_var && folded, SVNET_E_ARG,
                  "svnet_vn_cross_fold_f32: null w_feat / w_dir / gamma / beta / running_mean / running_var / folded");
    SVNET_REQUIRE(vx_ok(1, 1, O, Od), SVNET_E_UNSUPPORTED, "svnet_vn_cross_fold_f32: O %lld, Od %lld: needs 1 <= O <= %d, Od = O or 1", (long long)O,
                  (long long)Od, VX_MAX_O);
    const int64_t total = 3 * (O + Od) + O;
    hipLaunchKernelGGL(vn_cross_fold_kernel, dim3((unsigned)svnet_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, w_feat, w_dir, gamma, beta,
                       running_mean, running_var, (int)O, (int)Od, eps, folded);
    SVNET_CHECK_LAUNCH("vn_cross_fold_kernel");
    return SVNET_OK;
}

extern "C" int svnet_vn_edge_cross_mean_f32(const float* x, const int64_t* idx, const float* folded, int64_t B, int64_t N, int64_t k, int64_t O, int64_t Od,
                                            float slope, float* out, void* stream) {
    SVNET_REQUIRE(x && idx && folded && out, SVNET_E_ARG, "svnet_vn_edge_cross_mean_f32: null x / idx / folded / out");
    SVNET_REQUIRE(B >= 1 && B <= VX_MAX_B, SVNET_E_ARG, "svnet_vn_edge_cross_mean_f32: B %lld must lie in 1 .. %d", (long long)B, VX_MAX_B);
    SVNET_REQUIRE(vx_ok(N, k, O, Od), SVNET_E_UNSUPPORTED,
                  "svnet_vn_edge_cross_mean_f32: N %lld, k %lld, O %lld, Od %lld: needs 1 <= k <= %d, k <= N <= %d, 1 <= O <= %d, Od = O or 1", (long long)N,
                  (long long)k, (long long)O, (long long)Od, VX_MAX_K, VN_MAX_N, VX_MAX_O);
    const float* s = folded + 3 * (O + Od);
    const dim3 grid((unsigned)svnet_cdiv(N, VX_THREADS), (unsigned)svnet_cdiv(O, VX_CH), (unsigned)B);
    if (Od == 1 && O != 1)
        hipLaunchKernelGGL(vn_cross_kernel<true>, grid, dim3(VX_THREADS), 0, (hipStream_t)stream, x, idx, folded, s, s + O, (int)N, (int)k, (int)O, slope, out);
    else
        hipLaunchKernelGGL(vn_cross_kernel<false>, grid, dim3(VX_THREADS), 0, (hipStream_t)stream, x, idx, folded, s, s + O, (int)N, (int)k, (int)O, slope, out);
    SVNET_CHECK_LAUNCH("vn_cross_kernel");
    return SVNET_OK;
}
