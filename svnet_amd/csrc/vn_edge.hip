// Fused vector-neuron edge level for inference: the eval-mode forward of a VNLinearLeakyReLU (models/vn_layers.py:50-78) on the edge
// feature [x_j - x_i | x_i] of get_graph_feature (models/utils/vn_util.py:23-49) followed by mean_pool over the k neighbours - as a
// fold, one launch for the point tables and one for the edge pass, which writes 3 O floats per point and nothing else.  The contract
// is in include/svnet_hip.h ("fused vector-neuron edge level") and svnet_amd/vn_fused.py; tests/vn_ref.py restates it.
//
// The level is linear in the edge feature in front of its non-linearity, W [x_j - x_i | x_i] = W_a x_j + (W_b - W_a) x_i, so the
// products are taken once per point (the tables) and an edge adds two table rows.  Three kernels:
//   vn_fold_kernel    the two weight matrices split into their halves [A | D = B - A] and transposed into WT [C][R], R = 2 (O + Od)
//                     columns [A_f | A_d | D_f | D_d], and BatchNorm's running statistics folded into s, t [O].
//   vn_tables_kernel  one wave takes 64 columns of WT and VN_QT = 16 consecutive (component, point) pairs of a cloud as four 16 x 16
//                     accumulators of v_mfma_f32_16x16x4_f32 - bit for bit the chain of the contract, K never split - and writes,
//                     per pair, runs of 16 consecutive floats of a table row.
//   vn_edge_kernel    a workgroup takes VN_P consecutive points of a cloud.  The neighbour ids of the tile are clamped and staged in
//                     LDS once; a thread takes a (point, o) pair - o fastest, so the lanes of a wave read contiguous runs of a
//                     gathered row - keeps the centre's six floats and the three running sums in registers and walks the k
//                     neighbours.  The means go through LDS so that the stores run along n.  Workgroups are ordered so that a
//                     cloud's tiles share an XCD (edgeblock.hip's order): its neighbour table, up to 3 (O + Od) N floats = 2 MB at
//                     the classifier's widest level, stays in that XCD's L2.
// Table rows: [P: a O + o | Q: 3 O + a Od + od] for component a; TN (gathered by neighbour) holds Pn | Qn, TC (the centre's) Pc | Qc;
// the workspace is [TN | TC], each [B][N][3 (O + Od)].  Built with -ffp-contract=off (Makefile, NO_CONTRACT): every product, sum,
// quotient and square root is its own correctly rounded fp32 operation.  The fold of the statistics and the norm / leaky rule are
// vn_math.h's, shared with vn_tail.hip.
#include "vn_math.h"

namespace {

constexpr int VN_THREADS = 256;
constexpr int VN_MAX_K = 64, VN_MAX_C = 128, VN_MAX_O = 128;      // the envelope (svnet_vn_supported)
constexpr int VN_QT = 16;           // (component, point) pairs per wave of the tables kernel
constexpr int VN_P = 16;            // points per workgroup of the edge kernel
constexpr int VN_PP = VN_P + 1;     // row stride of the LDS image of the means: odd, so that o-adjacent lanes fall on distinct banks

inline bool vn_ok(int64_t N, int64_t k, int64_t C, int64_t O, int64_t Od) {
    return k >= 1 && k <= VN_MAX_K && N >= k && N <= VN_MAX_N && C >= 1 && C <= VN_MAX_C && O >= 1 && O <= VN_MAX_O && vn_dir_rows_ok(O, Od);
}
inline int64_t vn_row(int64_t O, int64_t Od) { return 3 * (O + Od); }
inline int64_t vn_cols(int64_t O, int64_t Od) { return 2 * (O + Od); }

// e over [C R columns | O]: column r of WT is A_f (r < O), A_d (< O + Od), D_f (< 2 O + Od), D_d; then s and t.
__global__ __launch_bounds__(VN_THREADS) void vn_fold_kernel(const float* __restrict__ wf, const float* __restrict__ wd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ rmean,
                                                             const float* __restrict__ rvar, int C, int O, int Od, float eps,
                                                             float* __restrict__ folded) {
    const int R = 2 * (O + Od), CR = C * R;
    const int e = blockIdx.x * VN_THREADS + threadIdx.x;
    if (e < CR) {
        const int c = e / R;
        int r = e - c * R;
        const bool diff = r >= O + Od;
        if (diff) r -= O + Od;
        const float* row = r < O ? wf + (int64_t)r * 2 * C : wd + (int64_t)(r - O) * 2 * C;
        folded[e] = diff ? row[C + c] - row[c] : row[c];
    } else if (e < CR + O) {
        const int o = e - CR;
        vn_bn_fold(gamma[o], beta[o], rmean[o], rvar[o], eps, folded[CR + o], folded[CR + O + o]);
    }
}

// grid (ceil(3 N / VN_QT), ceil(R / 64), B), one wave per block: VN_QT = 16 pairs x 64 columns as four 16 x 16 accumulators of
// v_mfma_f32_16x16x4_f32, bit for bit the c-ascending fmaf chain from +0 (mlp_tile.h's operand order: A = the inputs, lane = pair
// l & 15 at k = l >> 4; B = the weights, lane = column l & 15 at k = l >> 4; D[i] = pair 4 (l >> 4) + i, column l & 15).  K is padded
// to a multiple of 4 with zeros in both operands, which add exact zeros; pairs past 3 N and columns past R are computed on clamped
// addresses and not stored.
__global__ __launch_bounds__(64) void vn_tables_kernel(const float* __restrict__ x, const float* __restrict__ WT, int N, int C, int O, int Od,
                                                       float* __restrict__ TN, float* __restrict__ TC) {
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int R = 2 * (O + Od), ROW = 3 * (O + Od), Q = 3 * N;
    const int lane = threadIdx.x, r16 = lane & 15, kq = lane >> 4;
    const int r0 = blockIdx.y * 64, q0 = blockIdx.x * VN_QT;
    const int64_t b = blockIdx.z;
    const float* xb = x + b * C * Q;                                 // x [B][C][3][N]: per channel the 3 N pairs q = a N + n lie side by side
    const int qa = q0 + r16 < Q ? q0 + r16 : Q - 1;
    int wcol[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) wcol[t] = r0 + 16 * t + r16 < R ? r0 + 16 * t + r16 : R - 1;
    f32x4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int Kp = (C + 3) & ~3;
    for (int k0 = 0; k0 < Kp; k0 += 4) {
        const int c = k0 + kq;
        const bool live = c < C;
        const int cc = live ? c : C - 1;
        const float av = xb[(int64_t)cc * Q + qa];
        const float a = live ? av : 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float wv = WT[cc * R + wcol[t]];
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, live ? wv : 0.f, acc[t], 0, 0, 0);
        }
    }
    // where a column goes inside a table row: offset col + a * step
    int an[4], nn[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = q0 + 4 * kq + i;
        an[i] = q < Q ? q / N : -1;
        nn[i] = q - (an[i] < 0 ? 0 : an[i]) * N;
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = r0 + 16 * t + r16;
        const int h = r < O + Od ? r : r - (O + Od);
        float* tab = (r < O + Od ? TN : TC) + b * N * ROW;
        const int col = h < O ? h : 3 * O + (h - O), step = h < O ? O : Od;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (r < R && an[i] >= 0) tab[(int64_t)nn[i] * ROW + col + an[i] * step] = acc[t][i];
    }
}

__global__ __launch_bounds__(VN_THREADS) void vn_edge_kernel(const float* __restrict__ TN, const float* __restrict__ TC, const int64_t* __restrict__ idx,
                                                             const float* __restrict__ s, const float* __restrict__ t, int64_t B, int N, int k, int O,
                                                             int Od, int64_t chunks, float slope, float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char vn_lds[];
    int* s_idx = reinterpret_cast<int*>(vn_lds);                                // [VN_P][k] neighbour ids, clamped
    float* s_y = reinterpret_cast<float*>(s_idx + VN_P * k);                    // [3 O][VN_PP] the tile's means, (o, a)-major

    int64_t blk = blockIdx.x;
    if ((B & 7) == 0) {                                                         // XCD-aware order (edgeblock.hip): workgroups w and w + 8 share an XCD,
        const int64_t xcd = blk & 7, slot = blk >> 3;                           // so XCD x walks the clouds x, x + 8, ... one after the other
        blk = ((slot / chunks) * 8 + xcd) * chunks + (slot % chunks);
    }
    const int64_t b = blk / chunks;
    const int n0 = (int)(blk % chunks) * VN_P;
    const int np = N - n0 < VN_P ? N - n0 : VN_P;
    const int tid = threadIdx.x, ROW = 3 * (O + Od);

    const int64_t* ib = idx + (b * N + n0) * k;
    for (int e = tid; e < np * k; e += VN_THREADS) s_idx[e] = (int)clamp_index(ib[e], N);
    __syncthreads();

    const float* tnb = TN + b * N * ROW;
    const float one_minus = 1.f - slope, kf = (float)k;
    for (int e = tid; e < np * O; e += VN_THREADS) {
        const int p = e / O, o = e - p * O, od = Od == 1 ? 0 : o;
        const float* tc = TC + (b * N + n0 + p) * ROW;
        const int po = o, qo = 3 * O + od;
        const float pc0 = tc[po], pc1 = tc[po + O], pc2 = tc[po + 2 * O];
        const float qc0 = tc[qo], qc1 = tc[qo + Od], qc2 = tc[qo + 2 * Od];
        const float so = s[o], to = t[o];
        const int* nb = s_idx + p * k;
        float y0 = 0.f, y1 = 0.f, y2 = 0.f;
#pragma unroll 2
        for (int j = 0; j < k; ++j) {
            const float* tn = tnb + nb[j] * ROW;
            const float p0 = tn[po] + pc0, p1 = tn[po + O] + pc1, p2 = tn[po + 2 * O] + pc2;
            const float d0 = tn[qo] + qc0, d1 = tn[qo + Od] + qc1, d2 = tn[qo + 2 * Od] + qc2;
            float y[3];
            vn_norm_leaky(p0, p1, p2, d0, d1, d2, so, to, slope, one_minus, y);
            y0 += y[0];
            y1 += y[1];
            y2 += y[2];
        }
        float* sy = s_y + (o * 3) * VN_PP + p;
        sy[0] = y0 / kf;
        sy[VN_PP] = y1 / kf;
        sy[2 * VN_PP] = y2 / kf;
    }
    __syncthreads();
    float* ob = out + b * O * 3 * N + n0;                                       // out [B][O][3][N]
    for (int e = tid; e < 3 * O * VN_P; e += VN_THREADS) {
        const int oa = e / VN_P, p = e - oa * VN_P;
        if (p < np) ob[(int64_t)oa * N + p] = s_y[oa * VN_PP + p];
    }
}

}  // namespace

extern "C" int svnet_vn_supported(int64_t N, int64_t k, int64_t C, int64_t O, int64_t Od) { return vn_ok(N, k, C, O, Od) ? 1 : 0; }

extern "C" size_t svnet_vn_workspace_bytes(int64_t B, int64_t N, int64_t O, int64_t Od) {
    if (B < 1 || !vn_ok(N, 1, 1, O, Od)) return 0;
    return (size_t)2 * (size_t)B * (size_t)N * (size_t)vn_row(O, Od) * sizeof(float);
}

extern "C" int svnet_vn_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, int64_t C, int64_t O, int64_t Od, float eps, float* folded, void* stream) {
    SVNET_REQUIRE(w_feat && w_dir && gamma && beta && running_mean && running_var && folded, SVNET_E_ARG,
                  "svnet_vn_fold_f32: null w_feat / w_dir / gamma / beta / running_mean / running_var / folded");
    SVNET_REQUIRE(vn_ok(1, 1, C, O, Od), SVNET_E_UNSUPPORTED, "svnet_vn_fold_f32: C %lld, O %lld, Od %lld: needs 1 <= C <= %d, 1 <= O <= %d, Od = O or 1",
                  (long long)C, (long long)O, (long long)Od, VN_MAX_C, VN_MAX_O);
    const int64_t total = C * vn_cols(O, Od) + O;
    hipLaunchKernelGGL(vn_fold_kernel, dim3((unsigned)svnet_cdiv(total, VN_THREADS)), dim3(VN_THREADS), 0, (hipStream_t)stream, w_feat, w_dir, gamma, beta,
                       running_mean, running_var, (int)C, (int)O, (int)Od, eps, folded);
    SVNET_CHECK_LAUNCH("vn_fold_kernel");
    return SVNET_OK;
}

extern "C" int svnet_vn_tables_f32(const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, int64_t Od, float* workspace,
                                   size_t workspace_bytes, void* stream) {
    SVNET_REQUIRE(x && folded && workspace, SVNET_E_ARG, "svnet_vn_tables_f32: null x / folded / workspace");
    SVNET_REQUIRE(B >= 1 && B <= 65535, SVNET_E_ARG, "svnet_vn_tables_f32: B %lld must lie in 1 .. 65535", (long long)B);
    SVNET_REQUIRE(vn_ok(N, 1, C, O, Od), SVNET_E_UNSUPPORTED,
                  "svnet_vn_tables_f32: N %lld, C %lld, O %lld, Od %lld: needs 1 <= N <= %d, 1 <= C <= %d, 1 <= O <= %d, Od = O or 1", (long long)N,
                  (long long)C, (long long)O, (long long)Od, VN_MAX_N, VN_MAX_C, VN_MAX_O);
    SVNET_REQUIRE(workspace_bytes >= svnet_vn_workspace_bytes(B, N, O, Od), SVNET_E_WORKSPACE, "svnet_vn_tables_f32: workspace of %zu bytes, needs %zu",
                  workspace_bytes, svnet_vn_workspace_bytes(B, N, O, Od));
    float* TN = workspace;
    float* TC = workspace + B * N * vn_row(O, Od);
    const dim3 grid((unsigned)svnet_cdiv(3 * N, VN_QT), (unsigned)svnet_cdiv(vn_cols(O, Od), 64), (unsigned)B);
    hipLaunchKernelGGL(vn_tables_kernel, grid, dim3(64), 0, (hipStream_t)stream, x, folded, (int)N, (int)C, (int)O, (int)Od, TN, TC);
    SVNET_CHECK_LAUNCH("vn_tables_kernel");
    return SVNET_OK;
}

extern "C" int svnet_vn_edge_mean_f32(const float* workspace, size_t workspace_bytes, const int64_t* idx, const float* folded, int64_t B, int64_t N,
                                      int64_t k, int64_t C, int64_t O, int64_t Od, float slope, float* out, void* stream) {
    SVNET_REQUIRE(workspace && idx && folded && out, SVNET_E_ARG, "svnet_vn_edge_mean_f32: null workspace / idx / folded / out");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_vn_edge_mean_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(vn_ok(N, k, C, O, Od), SVNET_E_UNSUPPORTED,
                  "svnet_vn_edge_mean_f32: N %lld, k %lld, C %lld, O %lld, Od %lld: needs 1 <= k <= %d, k <= N <= %d, 1 <= C <= %d, 1 <= O <= %d, Od = O or 1",
                  (long long)N, (long long)k, (long long)C, (long long)O, (long long)Od, VN_MAX_K, VN_MAX_N, VN_MAX_C, VN_MAX_O);
    SVNET_REQUIRE(workspace_bytes >= svnet_vn_workspace_bytes(B, N, O, Od), SVNET_E_WORKSPACE, "svnet_vn_edge_mean_f32: workspace of %zu bytes, needs %zu",
                  workspace_bytes, svnet_vn_workspace_bytes(B, N, O, Od));
    const CloudGrid grid = cloud_grid(B, N, VN_P);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_vn_edge_mean_f32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)N, VN_P);
    const float* TN = workspace;
    const float* TC = workspace + B * N * vn_row(O, Od);
    const float* s = folded + C * vn_cols(O, Od);
    const size_t lds = sizeof(int) * VN_P * k + sizeof(float) * 3 * O * VN_PP;      // (at most 4 KB + 26 KB: no opt-in)
    hipLaunchKernelGGL(vn_edge_kernel, dim3((unsigned)grid.blocks), dim3(VN_THREADS), lds, (hipStream_t)stream, TN, TC, idx, s, s + O, B, (int)N, (int)k,
                       (int)O, (int)Od, grid.chunks, slope, out);
    SVNET_CHECK_LAUNCH("vn_edge_kernel");
    return SVNET_OK;
}
