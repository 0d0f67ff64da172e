// Fused two-layer vector-neuron edge level for inference: get_graph_feature -> VNLinearLeakyReLU -> VNLinearLeakyReLU -> mean over the k
// neighbours, the first two edge levels of VN_DGCNN_PSEG (models/vn_dgcnn_partseg.py: conv1 -> conv2 -> pool1, conv3 -> conv4 -> pool2)
// with pooling = 'mean', in eval mode.  The contract is in include/svnet_hip.h ("fused two-layer vector-neuron edge level") and
// svnet_amd/vn_fused.py; tests/vn_pseg_ref.py restates it.
//
// Layer 1 is linear in the edge feature in front of its non-linearity, so it is vn_edge.hip's: the point tables of svnet_vn_tables_f32
// and, per edge, two table rows added and vn_math.h's norm / leaky rule.  Layer 2 acts on layer 1's non-linear output: a dense product
// per edge that cannot be tabled.  vn_edge2_kernel keeps everything between the tables and the mean on the chip:
//   a workgroup takes P consecutive points of a cloud (P = 4, 2 or 1: e2_points).  The neighbour ids, clamped, and the centres' table rows
//   are staged in LDS once.
//   phase 1   a thread takes an (edge, channel) pair - channel fastest, so the lanes of a wave read contiguous runs of a gathered
//             row - and writes layer 1's y1 [3] into the LDS image ys [P][Kp][3][16 JT]: the edges of a point padded to JT = ceil(k / 16)
//             row tiles of 16, the O1 channels to Kp = a multiple of 4, both with exact zeros.  y1 never reaches HBM.
//   phase 2   a wave takes a (point, column tile of 16 output channels) pair.  Its row tiles are the point's JT edge tiles x the three
//             components, so the accumulators of v_mfma_f32_16x16x4_f32 (mlp_tile.h's operand order: A = y1 from LDS, lane = edge
//             l & 15 at k = l >> 4; B = the weights from memory, lane = column l & 15 at k = l >> 4; D[i] = edge 4 (l >> 4) + i, column
//             l & 15) leave p[o,0..2] and d[o,0..2] of one edge in one lane and the norm / leaky epilogue runs in registers.  The chain
//             is bit for bit the c-ascending fmaf chain from +0; K is never split.  With one direction row (Od2 = 1) the row is
//             computed once per edge, by plain fmaf chains into LDS, and shared by every column tile.
//   the mean  an ORDERED pass, not a tree: the running sums travel through the four lane quarters of a tile in edge order (a quarter adds
//             its four edges j-ascending, the next quarter reads the result by a lane shuffle), tile after tile; rows past k are never
//             added.  The lanes of quarter a write component a.
// Workgroups are ordered so that a cloud's tiles share an XCD (vn_edge_kernel's order): the cloud's neighbour table stays in that XCD's L2.
// Built with -ffp-contract=off (Makefile, NO_CONTRACT).  No atomics.
#include "vn_math.h"

namespace {

typedef float e2_f32x4 __attribute__((ext_vector_type(4)));

constexpr int E2_THREADS = 256, E2_WAVES = E2_THREADS / SVNET_WAVE;
constexpr int E2_MAX_K = 64, E2_MAX_C = 128, E2_MAX_O = 128;      // the envelope (svnet_vn_edge2_supported)
constexpr int E2_MAX_JT = E2_MAX_K / 16;
constexpr int E2_LDS_MAX = 160 * 1024;

inline bool e2_ok(int64_t N, int64_t k, int64_t C, int64_t O1, int64_t Od1, int64_t O2, int64_t Od2) {
    return k >= 1 && k <= E2_MAX_K && N >= k && N <= VN_MAX_N && C >= 1 && C <= E2_MAX_C && O1 >= 1 && O1 <= E2_MAX_O && O2 >= 1 && O2 <= E2_MAX_O &&
           vn_dir_rows_ok(O1, Od1) && vn_dir_rows_ok(O2, Od2);
}

// floats per channel of a point's image [3][16 JT], padded to 17 (mod 32): the channel-adjacent lanes of phase 1 write distinct banks and
// the four k-quarters of a wave's A fragment overlap in three banks only
constexpr int e2_xs(int jt) { return 48 * jt + ((jt & 1) ? 1 : 17); }
inline int64_t e2_lds(int P, int jt, int64_t k, int64_t O1, int64_t Od1, bool share2) {
    const int64_t Kp = (O1 + 3) & ~(int64_t)3;
    return 4 * P * (Kp * e2_xs(jt) + 3 * (O1 + Od1) + (share2 ? 3 * 16 * jt : 0) + k);
}
// points per workgroup: the most of which two workgroups share a CU (one gathers while one multiplies); one point's image always fits
// (128 channels x 209 floats = 107 KB at k = 64)
inline int e2_points(int jt, int64_t k, int64_t O1, int64_t Od1, bool share2) {
    for (const int P : {4, 2})
        if (e2_lds(P, jt, k, O1, Od1, share2) <= E2_LDS_MAX / 2) return P;
    return 1;
}

template <int JT, bool SHARE2>
__global__ __launch_bounds__(E2_THREADS) void vn_edge2_kernel(const float* __restrict__ TN, const float* __restrict__ TC, const int64_t* __restrict__ idx,
                                                              const float* __restrict__ s1, const float* __restrict__ t1, const float* __restrict__ WT2,
                                                              const float* __restrict__ s2, const float* __restrict__ t2, int64_t B, int N, int k, int O1,
                                                              int Od1, int O2, int P, int64_t chunks, float slope1, float slope2,
                                                              float* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char e2_smem[];
    constexpr int ROWS = 16 * JT, XS = e2_xs(JT);
    const int Kp = (O1 + 3) & ~3, ROW1 = 3 * (O1 + Od1), R2 = O2 + (SHARE2 ? 1 : O2);
    float* ys = reinterpret_cast<float*>(e2_smem);                              // [P][Kp][XS]: y1[c][a][j] of point p at (p Kp + c) XS + a ROWS + j
    float* tcs = ys + P * Kp * XS;                                              // [P][ROW1]: the centres' table rows
    float* ds = tcs + P * ROW1;                                                 // [P][3][ROWS]: the one direction row of layer 2 (SHARE2)
    int* s_idx = reinterpret_cast<int*>(ds + (SHARE2 ? P * 3 * ROWS : 0));      // [P][k] neighbour ids, clamped

    int64_t blk = blockIdx.x;
    if ((B & 7) == 0) {                                                         // XCD-aware order (vn_edge_kernel's)
        const int64_t xcd = blk & 7, slot = blk >> 3;
        blk = ((slot / chunks) * 8 + xcd) * chunks + (slot % chunks);
    }
    const int64_t b = blk / chunks;
    const int n0 = (int)(blk % chunks) * P;
    const int np = N - n0 < P ? N - n0 : P;
    const int tid = threadIdx.x;

    const int64_t* ib = idx + (b * N + n0) * k;
    for (int e = tid; e < np * k; e += E2_THREADS) s_idx[e] = (int)clamp_index(ib[e], N);
    const float* tcb = TC + (b * N + n0) * ROW1;
    for (int e = tid; e < np * ROW1; e += E2_THREADS) tcs[e] = tcb[e];
    __syncthreads();

    // ---- phase 1: layer 1 per (edge, channel), vn_edge_kernel's arithmetic in front of its sum; zeros in the padding
    const float* tnb = TN + b * N * ROW1;
    const float om1 = 1.f - slope1;
    for (int e = tid; e < np * ROWS * Kp; e += E2_THREADS) {
        const int rr = e / Kp, c = e - rr * Kp, p = rr / ROWS, j = rr - p * ROWS;
        float y[3] = {0.f, 0.f, 0.f};
        if (c < O1 && j < k) {
            const int od = Od1 == 1 ? 0 : c, qo = 3 * O1 + od;
            const float* tn = tnb + s_idx[p * k + j] * ROW1;
            const float* tc = tcs + p * ROW1;
            const float p0 = tn[c] + tc[c], p1 = tn[c + O1] + tc[c + O1], p2 = tn[c + 2 * O1] + tc[c + 2 * O1];
            const float d0 = tn[qo] + tc[qo], d1 = tn[qo + Od1] + tc[qo + Od1], d2 = tn[qo + 2 * Od1] + tc[qo + 2 * Od1];
            vn_norm_leaky(p0, p1, p2, d0, d1, d2, s1[c], t1[c], slope1, om1, y);
        }
        float* yp = ys + (p * Kp + c) * XS + j;
        yp[0] = y[0];
        yp[ROWS] = y[1];
        yp[2 * ROWS] = y[2];
    }
    __syncthreads();
    if (SHARE2) {
        for (int e = tid; e < np * 3 * ROWS; e += E2_THREADS) {
            const int p = e / (3 * ROWS), aj = e - p * 3 * ROWS;                // aj = a ROWS + j
            const float* xv = ys + p * Kp * XS + aj;
            const float* w = WT2 + O2;
            float acc = 0.f;
#pragma unroll 4
            for (int c = 0; c < O1; ++c) acc = fmaf(xv[c * XS], w[c * R2], acc);
            ds[e] = acc;
        }
        __syncthreads();
    }

    // ---- phase 2: layer 2 per (point, column tile), the epilogue and the ordered sum in registers
    const int wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int nct = (O2 + 15) >> 4;
    const float om2 = 1.f - slope2, kf = (float)k;
    for (int unit = wave; unit < np * nct; unit += E2_WAVES) {
        const int p = unit % np, ct = unit / np;
        const int o = ct * 16 + r16;
        const bool ov = o < O2;
        const int oc = ov ? o : O2 - 1;
        e2_f32x4 accp[JT][3], accd[JT][3];
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                accp[jt][a] = e2_f32x4{0.f, 0.f, 0.f, 0.f};
                accd[jt][a] = e2_f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        const float* wcol = WT2 + oc;
        const float* arow = ys + (p * Kp + kq) * XS + r16;
        // the weights of the next k-step are under way while this one multiplies (a channel past O1 reads the last row and is replaced
        // by an exact zero)
        float bf, bd = 0.f;
        {
            const int at = (kq < O1 ? kq : O1 - 1) * R2;
            bf = wcol[at];
            if (!SHARE2) bd = wcol[at + O2];
        }
        for (int k0 = 0; k0 < Kp; k0 += 4) {
            float nf = 0.f, nd = 0.f;
            if (k0 + 4 < Kp) {                                                   // (wave-uniform)
                const int cn = k0 + 4 + kq, at = (cn < O1 ? cn : O1 - 1) * R2;
                nf = wcol[at];
                if (!SHARE2) nd = wcol[at + O2];
            }
            const bool live = k0 + kq < O1;
            const float wf = live ? bf : 0.f, wd = live ? bd : 0.f;
            const float* ap = arow + k0 * XS;
#pragma unroll
            for (int jt = 0; jt < JT; ++jt) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const float av = ap[a * ROWS + jt * 16];
                    accp[jt][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wf, accp[jt][a], 0, 0, 0);
                    if (!SHARE2) accd[jt][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wd, accd[jt][a], 0, 0, 0);
                }
            }
            bf = nf;
            bd = nd;
        }
        const float so = s2[oc], to = t2[oc];
        const float* dp = ds + p * 3 * ROWS;
        float sum0 = 0.f, sum1 = 0.f, sum2 = 0.f;                               // the same in the four quarters of a column
#pragma unroll
        for (int jt = 0; jt < JT; ++jt) {
            if (jt * 16 >= k) break;                                            // (wave-uniform)
            float y[4][3];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = jt * 16 + 4 * kq + i;
                float d0, d1, d2;
                if (SHARE2) {
                    d0 = dp[j];
                    d1 = dp[ROWS + j];
                    d2 = dp[2 * ROWS + j];
                } else {
                    d0 = accd[jt][0][i];
                    d1 = accd[jt][1][i];
                    d2 = accd[jt][2][i];
                }
                vn_norm_leaky(accp[jt][0][i], accp[jt][1][i], accp[jt][2][i], d0, d1, d2, so, to, slope2, om2, y[i]);
            }
            // quarter q holds the tile's edges 4 q .. 4 q + 3: it adds them in order to the sums so far, every lane takes its column's result
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j0 = jt * 16 + 4 * q;
                if (j0 >= k) break;                                             // (wave-uniform)
                float a0 = sum0, a1 = sum1, a2 = sum2;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (j0 + i < k) {                                           // (wave-uniform) a padded row never enters the sum
                        a0 += y[i][0];
                        a1 += y[i][1];
                        a2 += y[i][2];
                    }
                }
                const int src = (q << 4) | r16;
                sum0 = __shfl(a0, src);
                sum1 = __shfl(a1, src);
                sum2 = __shfl(a2, src);
            }
        }
        if (ov && kq < 3) {                                                     // out [B][O2][3][N]: quarter a writes component a
            const float sum = kq == 0 ? sum0 : kq == 1 ? sum1 : sum2;
            out[((b * O2 + o) * 3 + kq) * N + n0 + p] = sum / kf;
        }
    }
}

template <int JT, bool SHARE2>
void e2_launch(unsigned blocks, size_t lds, hipStream_t stream, const float* TN, const float* TC, const int64_t* idx, const float* s1, const float* WT2,
               const float* s2, int64_t B, int N, int k, int O1, int Od1, int O2, int P, int64_t chunks, float slope1, float slope2, float* out) {
    hipLaunchKernelGGL((vn_edge2_kernel<JT, SHARE2>), dim3(blocks), dim3(E2_THREADS), lds, stream, TN, TC, idx, s1, s1 + O1, WT2, s2, s2 + O2, B, N, k, O1, Od1,
                       O2, P, chunks, slope1, slope2, out);
}

}  // namespace

extern "C" int svnet_vn_edge2_supported(int64_t N, int64_t k, int64_t C, int64_t O1, int64_t Od1, int64_t O2, int64_t Od2) {
    return e2_ok(N, k, C, O1, Od1, O2, Od2) ? 1 : 0;
}

extern "C" int svnet_vn_edge2_mean_f32(const float* workspace, size_t workspace_bytes, const int64_t* idx, const float* folded1, const float* folded2,
                                       int64_t B, int64_t N, int64_t k, int64_t C, int64_t O1, int64_t Od1, int64_t O2, int64_t Od2, float slope1,
                                       float slope2, float* out, void* stream) {
    SVNET_REQUIRE(workspace && idx && folded1 && folded2 && out, SVNET_E_ARG, "svnet_vn_edge2_mean_f32: null workspace / idx / folded1 / folded2 / out");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_vn_edge2_mean_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(e2_ok(N, k, C, O1, Od1, O2, Od2), SVNET_E_UNSUPPORTED,
                  "svnet_vn_edge2_mean_f32: N %lld, k %lld, C %lld, O1 %lld, Od1 %lld, O2 %lld, Od2 %lld: needs 1 <= k <= %d, k <= N <= %d, 1 <= C <= %d, "
                  "1 <= O1, O2 <= %d, Od1 = O1 or 1, Od2 = O2 or 1",
                  (long long)N, (long long)k, (long long)C, (long long)O1, (long long)Od1, (long long)O2, (long long)Od2, E2_MAX_K, VN_MAX_N, E2_MAX_C,
                  E2_MAX_O);
    SVNET_REQUIRE(workspace_bytes >= svnet_vn_workspace_bytes(B, N, O1, Od1), SVNET_E_WORKSPACE, "svnet_vn_edge2_mean_f32: workspace of %zu bytes, needs %zu",
                  workspace_bytes, svnet_vn_workspace_bytes(B, N, O1, Od1));
    const bool share2 = Od2 == 1 && O2 != 1;
    const int jt = (int)((k + 15) >> 4);
    const int P = e2_points(jt, k, O1, Od1, share2);
    const CloudGrid grid = cloud_grid(B, N, P);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_vn_edge2_mean_f32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)N, P);
    const size_t lds = (size_t)e2_lds(P, jt, k, O1, Od1, share2);
    if (lds > 64 * 1024) {
        bool ok = true;
        SVNET_LDS_OPTIN(ok, E2_LDS_MAX, "svnet_vn_edge2_mean_f32", reinterpret_cast<const void*>(vn_edge2_kernel<1, false>),
                        reinterpret_cast<const void*>(vn_edge2_kernel<1, true>), reinterpret_cast<const void*>(vn_edge2_kernel<2, false>),
                        reinterpret_cast<const void*>(vn_edge2_kernel<2, true>), reinterpret_cast<const void*>(vn_edge2_kernel<3, false>),
                        reinterpret_cast<const void*>(vn_edge2_kernel<3, true>), reinterpret_cast<const void*>(vn_edge2_kernel<4, false>),
                        reinterpret_cast<const void*>(vn_edge2_kernel<4, true>));
        if (!ok) return SVNET_E_LAUNCH;
    }
    const float* TN = workspace;
    const float* TC = workspace + B * N * 3 * (O1 + Od1);
    const float* s1 = folded1 + C * 2 * (O1 + Od1);
    const float* s2 = folded2 + O1 * (O2 + Od2);
    const hipStream_t st = (hipStream_t)stream;
#define E2_GO(JT, SHARE2)                                                                                                                             \
    e2_launch<JT, SHARE2>((unsigned)grid.blocks, lds, st, TN, TC, idx, s1, folded2, s2, B, (int)N, (int)k, (int)O1, (int)Od1, (int)O2, P, grid.chunks, \
                          slope1, slope2, out)
    static_assert(E2_MAX_JT == 4, "the dispatch below names every tile count");
    if (share2) {
        if (jt == 1) E2_GO(1, true);
        else if (jt == 2) E2_GO(2, true);
        else if (jt == 3) E2_GO(3, true);
        else E2_GO(4, true);
    } else {
        if (jt == 1) E2_GO(1, false);
        else if (jt == 2) E2_GO(2, false);
        else if (jt == 3) E2_GO(3, false);
        else E2_GO(4, false);
    }
#undef E2_GO
    SVNET_CHECK_LAUNCH("vn_edge2_kernel");
    return SVNET_OK;
}
