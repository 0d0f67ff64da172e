// Fused vector-neuron tail for inference: what VN_DGCNN_CLS.tail runs behind the four edge levels - conv5, the cloud mean, VNStdFeature's
// vn1 and vn2, its frame and einsum, and the [amax | mean] pool over the points - as per-point kernels.  The contract is in
// include/svnet_hip.h ("fused vector-neuron tail for inference") and svnet_amd/vn_tail.py; tests/vn_tail_ref.py restates it.
//
//   vn_point_fold_kernel   [W_f | W_d] transposed into WT [C + Cg][R], R = O + Od, so that a wave reads consecutive columns of one c;
//                          BatchNorm's running statistics folded into s, t [O].
//   vn_cloud_term_kernel   u [B][3][R]: per cloud the chain over the Cg channels that are constant over it (Cg > 0 only).
//   vn_point_kernel        the eval forward of a VNLinearLeakyReLU per point.  A workgroup takes TP = 16 NPT consecutive points of a
//                          cloud and stages their x, all K channels x 3 components, in LDS once; NPT is the largest of 4, 2, 1 whose
//                          image leaves room for a second workgroup on the CU (vt_point_tiles).  A wave takes the column tiles
//                          wave, wave + 4, ... of 16 output channels; its three row tiles are the three components of the same 16
//                          points, so the accumulators of v_mfma_f32_16x16x4_f32 (mlp_tile.h's operand order) leave p[o,0..2] and
//                          d[o,0..2] of one point in one lane and the norm, BatchNorm and leaky epilogue runs in registers: neither p
//                          nor d goes to memory.  The chain starts at the cloud term and K is never split.  With one direction row
//                          (Od = 1) the row is computed once per point, by plain fmaf chains into LDS, and shared by every wave.
//                          The epilogue is a policy: VtLeaky is the layer above; VtNormOnly is a VNLinear followed by a VNBatchNorm
//                          (svnet_vn_point_norm_f32) - no direction rows, R = O, and the norm half of the rule alone.
//   vn_cloud_mean_kernel   m [B,C,3]: per row of N floats the sums of runs of 64, n-ascending, then the runs' sums in order.
//   vn_std_pool_kernel     grid (runs, B): the three frame rows z of the run's 64 points (chains over Cy) into LDS, then the channels in
//                          slabs of 64 through LDS; a thread owns a column (i, k) and walks the run's points n-ascending, keeping the
//                          maximum and the sum, which go to the workspace as per-run partials.
//   vn_std_finish_kernel   per column the maximum of the runs' maxima and the runs' sums added in order (split_reduce.h), over fl(N).
//   vn_std_coords_kernel   grid (runs, B): the same frame rows, then the coordinates of every channel of x per point, unpooled, stored
//                          along n: what VN_DGCNN_PSEG's head reads of the levels' features.  The frame rows and the coordinates are
//                          stated once (vt_stage_frame, vt_coordinate) and both kernels call them.
// Every entry exists twice: in the base envelope (widths to 512) and, named svnet_vn_*_wide_*, in the wide one (widths to 768:
// VN_PointNet_PSEG's 682).  The kernels are the same and so is the plan: above 426 channels the image of x at NPT 1 is more than half of LDS, so one
// workgroup has the CU to itself and staging does not overlap the products; at 768 it is 144 KiB (VtEnvelope).
// The fold of the statistics and the norm / BatchNorm / leaky arithmetic are vn_math.h's, shared with vn_edge.hip.  Built with
// -ffp-contract=off (Makefile, NO_CONTRACT).  No atomics.
#include "vn_math.h"
#include "split_reduce.h"
#include <type_traits>

namespace {

typedef __attribute__((ext_vector_type(4))) float vt_f32x4;

constexpr int VT_THREADS = 256, VT_WAVES = VT_THREADS / SVNET_WAVE;
constexpr int VT_MAX_B = 65535;
// The envelope of an entry: the widest C, Cg and Cy and the widest O it admits.  The kernels are written for any width whose image fits
// LDS; what an entry admits is what its tests pin.  VT_BASE is the entries' of ABI 433 to 435, VT_WIDE the svnet_vn_*_wide_* entries':
// at NPT 1 the image of 768 channels is 4 x 768 x 48 = 147456 bytes (+ 192 with one direction row), under VT_LDS_MAX.
struct VtEnvelope { int max_c, max_o; };
constexpr VtEnvelope VT_BASE{512, 512}, VT_WIDE{768, 768};
constexpr int VT_RUN = 64;              // points per run of the ordered sums: part of the contract
constexpr int VT_LDS_MAX = 160 * 1024;
constexpr int VT_SLAB = 64;             // channels per LDS slab of the std-pool kernel
constexpr int VT_VS = 3 * VT_RUN + 1;   // floats per channel of a slab: odd, so that channel-adjacent lanes fall on distinct banks
constexpr int VT_SU = 8;                // loads of a thread in flight while x is staged
constexpr int VT_U = 8;                 // k-steps whose weights a lane holds at a time: 32 channels

inline bool vt_point_ok(const VtEnvelope& v, int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od) {
    return N >= 1 && N <= VN_MAX_N && C >= 1 && C <= v.max_c && Cg >= 0 && Cg <= v.max_c && O >= 1 && O <= v.max_o && vn_dir_rows_ok(O, Od);
}
inline bool vt_std_ok(const VtEnvelope& v, int64_t N, int64_t C, int64_t Cg, int64_t Cy) {
    return N >= 1 && N <= VN_MAX_N && C >= 1 && C <= v.max_c && Cg >= 0 && Cg <= v.max_c && Cy >= 1 && Cy <= v.max_c;
}
inline bool vt_batch_ok(int64_t B) { return B >= 1 && B <= VT_MAX_B; }

// points per workgroup of the point kernel as 16-point tiles, and the row stride of the LDS image of x [Kp][3][TP]: padded so that the
// four k-quarters of a wave's A fragment fall on distinct banks
constexpr int vt_xs(int npt) { return 48 * npt + (npt == 1 ? 0 : 16); }
inline int64_t vt_point_lds(int npt, int64_t C, bool share) { return 4 * (((C + 3) & ~(int64_t)3) * vt_xs(npt) + (share ? 48 * npt : 0)); }
inline int vt_point_tiles(int64_t N, int64_t C, bool share) {
    for (const int npt : {4, 2})                         // the most points of which two workgroups share a CU: one stages while one multiplies
        if (N > 8 * npt && vt_point_lds(npt, C, share) <= VT_LDS_MAX / 2) return npt;
    return 1;
}

// ---- the epilogue of the point kernel on p, d [3] of one (point, channel); DIR: whether the layer has direction rows at all
struct VtLeaky {
    static constexpr bool DIR = true;
    static __device__ __forceinline__ void apply(float p0, float p1, float p2, float d0, float d1, float d2, float so, float to, float slope,
                                                 float one_minus, float (&y)[3]) {
        vn_norm_leaky(p0, p1, p2, d0, d1, d2, so, to, slope, one_minus, y);
    }
};
struct VtNormOnly {
    static constexpr bool DIR = false;
    static __device__ __forceinline__ void apply(float p0, float p1, float p2, float, float, float, float so, float to, float, float, float (&y)[3]) {
        vn_norm(p0, p1, p2, so, to, y);
    }
};

// e over [K R | O]: WT[c][r] = row r of [W_f | W_d] at channel c; then s and t.  Od = 0 (a layer without direction rows): w_d is not read.
__global__ __launch_bounds__(VT_THREADS) void vn_point_fold_kernel(const float* __restrict__ wf, const float* __restrict__ wd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, const float* __restrict__ rmean,
                                                                   const float* __restrict__ rvar, int K, int O, int Od, float eps,
                                                                   float* __restrict__ folded) {
    const int R = O + Od, KR = K * R;
    const int e = blockIdx.x * VT_THREADS + threadIdx.x;
    if (e < KR) {
        const int c = e / R, r = e - c * R;
        folded[e] = r < O ? wf[(int64_t)r * K + c] : wd[(int64_t)(r - O) * K + c];
    } else if (e < KR + O) {
        const int o = e - KR;
        vn_bn_fold(gamma[o], beta[o], rmean[o], rvar[o], eps, folded[KR + o], folded[KR + O + o]);
    }
}

// e over [B][3][R]: u = +0, then u = fmaf(g[b,c,a], W[r, C + c], u) for c ascending over Cg
__global__ __launch_bounds__(VT_THREADS) void vn_cloud_term_kernel(const float* __restrict__ g, const float* __restrict__ WT, int64_t total, int C, int Cg,
                                                                   int R, float* __restrict__ u) {
    const int64_t e = (int64_t)blockIdx.x * VT_THREADS + threadIdx.x;
    if (e >= total) return;
    const int r = (int)(e % R), a = (int)((e / R) % 3);
    const int64_t b = e / (3 * R);
    const float* gb = g + b * Cg * 3 + a;
    const float* w = WT + (int64_t)C * R + r;
    float acc = 0.f;
    for (int c = 0; c < Cg; ++c) acc = fmaf(gb[3 * c], w[(int64_t)c * R], acc);
    u[e] = acc;
}

// grid (ceil(N / TP), B), TP = 16 NPT.  A = the inputs from LDS (lane = point l & 15 at k = l >> 4), B = the weights from global memory
// (lane = column l & 15 at k = l >> 4), D[i] = point 4 (l >> 4) + i, column l & 15.  K is padded to a multiple of 4 with zeros in both
// operands; points past N are zeros in LDS and are not stored; columns past O are computed on a clamped address and not stored.
template <int NPT, bool SHARE, class EPI>
__global__ __launch_bounds__(VT_THREADS) void vn_point_kernel(const float* __restrict__ x, const float* __restrict__ WT, const float* __restrict__ s,
                                                              const float* __restrict__ t, const float* __restrict__ u, int N, int C, int O, float slope,
                                                              int vec, float* __restrict__ out) {
    extern __shared__ __align__(16) float vt_lds[];
    constexpr int TP = 16 * NPT, XS = vt_xs(NPT);
    const int Od = !EPI::DIR ? 0 : SHARE ? 1 : O, R = O + Od, Kp = (C + 3) & ~3;
    float* xs = vt_lds;                                  // [Kp][XS]: x[c][a][p] at c XS + a TP + p
    float* ds = vt_lds + Kp * XS;                        // [3][TP]: the one direction row (SHARE)
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int n0 = blockIdx.x * TP;
    const float* xb = x + b * C * 3 * N;
    // the image of x: VT_SU loads of a thread are under way before the first is stored; whole float4s where N and x allow them
    if (vec) {
        constexpr int TQ = TP / 4;
        const int total = Kp * 3 * TQ;
        for (int e0 = tid; e0 < total; e0 += VT_THREADS * VT_SU) {
            float4 v[VT_SU];
#pragma unroll
            for (int uu = 0; uu < VT_SU; ++uu) {
                const int e = e0 + uu * VT_THREADS, ca = e / TQ, p = 4 * (e - ca * TQ);
                v[uu] = float4{0.f, 0.f, 0.f, 0.f};
                if (e < total && ca < 3 * C && n0 + p < N) v[uu] = *reinterpret_cast<const float4*>(xb + (int64_t)ca * N + n0 + p);
            }
#pragma unroll
            for (int uu = 0; uu < VT_SU; ++uu) {
                const int e = e0 + uu * VT_THREADS, ca = e / TQ, c = ca / 3, a = ca - 3 * c, p = 4 * (e - ca * TQ);
                if (e < total) *reinterpret_cast<float4*>(xs + c * XS + a * TP + p) = v[uu];
            }
        }
    } else {
        const int total = Kp * 3 * TP;
        for (int e0 = tid; e0 < total; e0 += VT_THREADS * VT_SU) {
            float v[VT_SU];
#pragma unroll
            for (int uu = 0; uu < VT_SU; ++uu) {
                const int e = e0 + uu * VT_THREADS, ca = e / TP, p = e - ca * TP;
                v[uu] = e < total && ca < 3 * C && n0 + p < N ? xb[(int64_t)ca * N + n0 + p] : 0.f;
            }
#pragma unroll
            for (int uu = 0; uu < VT_SU; ++uu) {
                const int e = e0 + uu * VT_THREADS, ca = e / TP, c = ca / 3, a = ca - 3 * c, p = e - ca * TP;
                if (e < total) xs[c * XS + a * TP + p] = v[uu];
            }
        }
    }
    __syncthreads();
    const float* ub = u ? u + b * 3 * R : nullptr;
    if (SHARE) {
        for (int e = tid; e < 3 * TP; e += VT_THREADS) {
            const int a = e / TP, p = e - a * TP;
            float acc = ub ? ub[a * R + O] : 0.f;
            const float* xv = xs + a * TP + p;
            const float* w = WT + O;
#pragma unroll 4
            for (int c = 0; c < C; ++c) acc = fmaf(xv[c * XS], w[(int64_t)c * R], acc);
            ds[e] = acc;
        }
        __syncthreads();
    }
    const int wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    const int nct = (O + 15) >> 4;
    const float one_minus = 1.f - slope;
    for (int ct = wave; ct < nct; ct += VT_WAVES) {
        const int o = ct * 16 + r16;
        const bool ov = o < O;
        const int oc = ov ? o : O - 1;
        vt_f32x4 accp[NPT][3], accd[NPT][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float up = ub ? ub[a * R + oc] : 0.f;
            const float ud = (EPI::DIR && !SHARE && ub) ? ub[a * R + O + oc] : 0.f;
#pragma unroll
            for (int tt = 0; tt < NPT; ++tt) {
                accp[tt][a] = vt_f32x4{up, up, up, up};
                accd[tt][a] = vt_f32x4{ud, ud, ud, ud};
            }
        }
        const float* wcol = WT + oc;
        const float* arow = xs + kq * XS + r16;
        // a lane holds the weights of VT_U k-steps; the next VT_U are under way while these multiply (a channel past C reads the
        // last row and is replaced by an exact zero)
        float wfc[VT_U], wdc[VT_U], wfn[VT_U], wdn[VT_U];
        const auto weights = [&](int c0, float (&wf)[VT_U], float (&wd)[VT_U]) {
#pragma unroll
            for (int uu = 0; uu < VT_U; ++uu) {
                const int c = c0 + 4 * uu + kq, at = (c < C ? c : C - 1) * R;
                wf[uu] = wcol[at];
                wd[uu] = SHARE || !EPI::DIR ? 0.f : wcol[at + O];
            }
        };
        // VT_U k-steps on the weights in wfc / wdc.  Whole blocks carry no branch, so their LDS reads are scheduled ahead of the
        // products; the last, partial block stops at Kp.
        const auto steps = [&](int k0, auto whole) {
#pragma unroll
            for (int uu = 0; uu < VT_U; ++uu) {
                const int k = k0 + 4 * uu;
                if (!decltype(whole)::value && k >= Kp) break;   // (wave-uniform)
                const bool live = k + kq < C;
                const float bf = live ? wfc[uu] : 0.f, bd = live ? wdc[uu] : 0.f;
                const float* ap = arow + k * XS;
#pragma unroll
                for (int tt = 0; tt < NPT; ++tt) {
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        const float av = ap[a * TP + tt * 16];
                        accp[tt][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bf, accp[tt][a], 0, 0, 0);
                        if (EPI::DIR && !SHARE) accd[tt][a] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bd, accd[tt][a], 0, 0, 0);
                    }
                }
            }
        };
        weights(0, wfc, wdc);
        int k0 = 0;
        for (; k0 + 4 * VT_U <= Kp; k0 += 4 * VT_U) {
            weights(k0 + 4 * VT_U, wfn, wdn);
            steps(k0, std::true_type{});
#pragma unroll
            for (int uu = 0; uu < VT_U; ++uu) {
                wfc[uu] = wfn[uu];
                wdc[uu] = wdn[uu];
            }
        }
        if (k0 < Kp) steps(k0, std::false_type{});
        const float so = s[oc], to = t[oc];
        float* ob = out + (b * O + oc) * 3 * N;
#pragma unroll
        for (int tt = 0; tt < NPT; ++tt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = tt * 16 + 4 * kq + i, n = n0 + p;
                float d0, d1, d2, y[3];
                if (SHARE) {
                    d0 = ds[p];
                    d1 = ds[TP + p];
                    d2 = ds[2 * TP + p];
                } else {
                    d0 = accd[tt][0][i];
                    d1 = accd[tt][1][i];
                    d2 = accd[tt][2][i];
                }
                EPI::apply(accp[tt][0][i], accp[tt][1][i], accp[tt][2][i], d0, d1, d2, so, to, slope, one_minus, y);
                if (ov && n < N) {
                    ob[n] = y[0];
                    ob[(int64_t)N + n] = y[1];
                    ob[2 * (int64_t)N + n] = y[2];
                }
            }
        }
    }
}

// A workgroup takes rpb rows of N floats (rpb runs-per-row <= 512 partials): a thread sums a run n-ascending from +0, then a thread
// per row adds the runs' sums j-ascending from +0 and divides by fl(N).
__global__ __launch_bounds__(VT_THREADS) void vn_cloud_mean_kernel(const float* __restrict__ x, int64_t rows, int N, int runs, int rpb,
                                                                   float* __restrict__ m) {
    __shared__ float part[512];
    const int64_t row0 = (int64_t)blockIdx.x * rpb;
    const int nr = rows - row0 < rpb ? (int)(rows - row0) : rpb;
    for (int e = threadIdx.x; e < nr * runs; e += VT_THREADS) {
        const int r = e / runs, j = e - r * runs;
        const float* p = x + (row0 + r) * N + VT_RUN * j;
        const int len = N - VT_RUN * j < VT_RUN ? N - VT_RUN * j : VT_RUN;
        float sum = 0.f;
        if (len == VT_RUN) {
#pragma unroll 16
            for (int i = 0; i < VT_RUN; ++i) sum += p[i];
        } else {
            for (int i = 0; i < len; ++i) sum += p[i];
        }
        part[e] = sum;
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) {
        float sum = 0.f;
        for (int j = 0; j < runs; ++j) sum += part[threadIdx.x * runs + j];
        m[row0 + threadIdx.x] = sum / (float)N;
    }
}

// ---- the two rules of the learnt frame, stated once: the standardise-and-pool kernel and the per-point coordinates kernel call them
// frame rows: z[k][a](n) = +0, then fmaf(y[c,a,n], w_lin[k,c], z) for c ascending over Cy.  The first 3 VT_RUN threads of a workgroup take
// an (a, point) pair of the run at n0 each and leave zs [p][k][a | pad]; a point past the run's end reads the cloud's last one.
__device__ __forceinline__ void vt_stage_frame(const float* __restrict__ y, const float* __restrict__ wlin, int64_t b, int n0, int np, int N, int Cy,
                                               float* __restrict__ zs) {
    const int tid = threadIdx.x;
    if (tid < 3 * VT_RUN) {
        const int a = tid / VT_RUN, p = tid - a * VT_RUN;
        const int n = p < np ? n0 + p : N - 1;
        const float* yp = y + (b * Cy * 3 + a) * N + n;
        float z0 = 0.f, z1 = 0.f, z2 = 0.f;
#pragma unroll 4
        for (int c = 0; c < Cy; ++c) {
            const float yv = yp[(int64_t)c * 3 * N];
            z0 = fmaf(yv, wlin[c], z0);
            z1 = fmaf(yv, wlin[Cy + c], z1);
            z2 = fmaf(yv, wlin[2 * Cy + c], z2);
        }
        zs[p * 12 + a] = z0;
        zs[p * 12 + 4 + a] = z1;
        zs[p * 12 + 8 + a] = z2;
        if (a == 0) zs[p * 12 + 3] = zs[p * 12 + 7] = zs[p * 12 + 11] = 0.f;
    }
}
// coordinates: e[i,k](n) = fmaf(v[2], z[k][2], fmaf(v[1], z[k][1], fl(v[0] z[k][0]))), z = the frame row k of the point
__device__ __forceinline__ float vt_coordinate(float v0, float v1, float v2, const float4& z) { return fmaf(v2, z.z, fmaf(v1, z.y, v0 * z.x)); }

// grid (runs, B).  pmax, psum: [runs][B][3 I], I = C + Cg.
__global__ __launch_bounds__(VT_THREADS) void vn_std_pool_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ y,
                                                                 const float* __restrict__ wlin, int N, int C, int Cg, int Cy, float* __restrict__ pmax,
                                                                 float* __restrict__ psum) {
    __shared__ __align__(16) float zs[VT_RUN * 12];      // [p][k][a | pad]: the frame rows of the run's points
    __shared__ float vs[VT_SLAB * VT_VS];                // [channel of the slab][a][p]
    const int tid = threadIdx.x, j = blockIdx.x;
    const int64_t b = blockIdx.y, B = gridDim.y;
    const int n0 = VT_RUN * j, np = N - n0 < VT_RUN ? N - n0 : VT_RUN;
    vt_stage_frame(y, wlin, b, n0, np, N, Cy, zs);
    const int I = C + Cg;
    const int64_t total = B * 3 * I;
    const int ci = tid / 3, k = tid - ci * 3;
    for (int i0 = 0; i0 < I; i0 += VT_SLAB) {
        __syncthreads();                                 // zs written; the slab before this one read
        const int nx = C - i0 < VT_SLAB ? C - i0 : VT_SLAB;
        for (int e = tid; e < nx * 3 * VT_RUN; e += VT_THREADS) {
            const int c = e / (3 * VT_RUN), rem = e - c * 3 * VT_RUN, a = rem / VT_RUN, p = rem - a * VT_RUN;
            vs[c * VT_VS + a * VT_RUN + p] = p < np ? x[((b * C + i0 + c) * 3 + a) * N + n0 + p] : 0.f;
        }
        __syncthreads();
        const int i = i0 + ci;
        if (tid < 3 * VT_SLAB && i < I) {
            float sum = 0.f, best = 0.f;
            if (i < C) {
                const float* v = vs + ci * VT_VS;
                for (int p = 0; p < np; ++p) {
                    const float4 z = *reinterpret_cast<const float4*>(zs + p * 12 + 4 * k);
                    const float e = vt_coordinate(v[p], v[VT_RUN + p], v[2 * VT_RUN + p], z);
                    sum += e;
                    best = p == 0 || e > best ? e : best;
                }
            } else {
                const float* gv = g + (b * Cg + (i - C)) * 3;
                const float g0 = gv[0], g1 = gv[1], g2 = gv[2];
                for (int p = 0; p < np; ++p) {
                    const float4 z = *reinterpret_cast<const float4*>(zs + p * 12 + 4 * k);
                    const float e = vt_coordinate(g0, g1, g2, z);
                    sum += e;
                    best = p == 0 || e > best ? e : best;
                }
            }
            const int64_t at = (int64_t)j * total + b * 3 * I + 3 * i + k;
            pmax[at] = best;
            psum[at] = sum;
        }
    }
}

// e over [B][3 I]: h[b][col] = the maximum over the runs, h[b][3 I + col] = (the runs' sums in order) / fl(N)
__global__ __launch_bounds__(VT_THREADS) void vn_std_finish_kernel(const float* __restrict__ pmax, const float* __restrict__ psum, int64_t runs, int64_t total,
                                                                   int cols, int N, float* __restrict__ h) {
    const int64_t e = (int64_t)blockIdx.x * VT_THREADS + threadIdx.x;
    if (e >= total) return;
    float best = pmax[e];
    for (int64_t j = 1; j < runs; ++j) {
        const float v = pmax[j * total + e];
        best = v > best ? v : best;
    }
    const int64_t b = e / cols, col = e - b * cols;
    h[b * 2 * cols + col] = best;
    h[b * 2 * cols + cols + col] = ordered_chunk_sum(psum, runs, total, e) / (float)N;
}

// grid (runs, B): the frame rows of the run's 64 points into LDS, then a thread takes a (channel, point) pair - point fastest, so the loads
// and the stores of a wave run along n - and writes the channel's three coordinates.  e [B][3 C][N].
__global__ __launch_bounds__(VT_THREADS) void vn_std_coords_kernel(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ wlin,
                                                                   int N, int C, int Cy, float* __restrict__ e) {
    __shared__ __align__(16) float zs[VT_RUN * 12];      // [p][k][a | pad]
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.y;
    const int n0 = VT_RUN * blockIdx.x, np = N - n0 < VT_RUN ? N - n0 : VT_RUN;
    vt_stage_frame(y, wlin, b, n0, np, N, Cy, zs);
    __syncthreads();
    const float* xb = x + b * C * 3 * N + n0;
    float* eb = e + b * 3 * C * N + n0;
    for (int w = tid; w < C * VT_RUN; w += VT_THREADS) {
        const int i = w / VT_RUN, p = w - i * VT_RUN;
        if (p >= np) continue;
        const float* xv = xb + (int64_t)i * 3 * N + p;
        const float v0 = xv[0], v1 = xv[N], v2 = xv[2 * (int64_t)N];
        float* ev = eb + (int64_t)i * 3 * N + p;
#pragma unroll
        for (int k = 0; k < 3; ++k) ev[(int64_t)k * N] = vt_coordinate(v0, v1, v2, *reinterpret_cast<const float4*>(zs + p * 12 + 4 * k));
    }
}

template <int NPT, bool SHARE, class EPI>
void vt_launch_point(dim3 grid, size_t lds, hipStream_t stream, const float* x, const float* WT, const float* s, const float* t, const float* u, int N, int C,
                     int O, float slope, float* out) {
    const int vec = (N & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;      // whole, aligned float4s along n
    hipLaunchKernelGGL((vn_point_kernel<NPT, SHARE, EPI>), grid, dim3(VT_THREADS), lds, stream, x, WT, s, t, u, N, C, O, slope, vec, out);
}

}  // namespace

// ---- the host side, stated once: an entry of the base envelope and its _wide twin pass their envelope and their own name (for the
// messages) to the same function, which checks, plans (vt_point_tiles) and launches.  Within the base envelope both therefore choose
// the same kernel and return the same bits.
namespace {

size_t vt_point_workspace(const VtEnvelope& v, int64_t B, int64_t Cg, int64_t O, int64_t Od) {
    if (!vt_batch_ok(B) || !vt_point_ok(v, 1, 1, Cg, O, Od)) return 0;
    return Cg > 0 ? (size_t)B * 3 * (size_t)(O + Od) * sizeof(float) : 0;
}

int vt_point_fold(const VtEnvelope& v, const char* name, const float* w_feat, const float* w_dir, const float* gamma, const float* beta,
                  const float* running_mean, const float* running_var, int64_t C, int64_t Cg, int64_t O, int64_t Od, float eps, float* folded, void* stream) {
    SVNET_REQUIRE(w_feat && w_dir && gamma && beta && running_mean && running_var && folded, SVNET_E_ARG,
                  "%s: null w_feat / w_dir / gamma / beta / running_mean / running_var / folded", name);
    SVNET_REQUIRE(vt_point_ok(v, 1, C, Cg, O, Od), SVNET_E_UNSUPPORTED,
                  "%s: C %lld, Cg %lld, O %lld, Od %lld: needs 1 <= C <= %d, 0 <= Cg <= %d, 1 <= O <= %d, Od = O or 1", name, (long long)C, (long long)Cg,
                  (long long)O, (long long)Od, v.max_c, v.max_c, v.max_o);
    const int64_t total = (C + Cg) * (O + Od) + O;
    hipLaunchKernelGGL(vn_point_fold_kernel, dim3((unsigned)svnet_cdiv(total, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, w_feat, w_dir, gamma,
                       beta, running_mean, running_var, (int)(C + Cg), (int)O, (int)Od, eps, folded);
    SVNET_CHECK_LAUNCH("vn_point_fold_kernel");
    return SVNET_OK;
}

int vt_point(const VtEnvelope& v, const char* name, const float* x, const float* g, const float* folded, int64_t B, int64_t N, int64_t C, int64_t Cg,
             int64_t O, int64_t Od, float slope, void* workspace, size_t workspace_bytes, float* out, void* stream) {
    SVNET_REQUIRE(x && folded && out && (Cg <= 0 || (g && workspace)), SVNET_E_ARG, "%s: null x / folded / out, or g / workspace with Cg > 0", name);
    SVNET_REQUIRE(vt_batch_ok(B), SVNET_E_ARG, "%s: B %lld must lie in 1 .. %d", name, (long long)B, VT_MAX_B);
    SVNET_REQUIRE(vt_point_ok(v, N, C, Cg, O, Od), SVNET_E_UNSUPPORTED,
                  "%s: N %lld, C %lld, Cg %lld, O %lld, Od %lld: needs 1 <= N <= %d, 1 <= C <= %d, 0 <= Cg <= %d, 1 <= O <= %d, Od = O or 1", name,
                  (long long)N, (long long)C, (long long)Cg, (long long)O, (long long)Od, VN_MAX_N, v.max_c, v.max_c, v.max_o);
    SVNET_REQUIRE(workspace_bytes >= vt_point_workspace(v, B, Cg, O, Od), SVNET_E_WORKSPACE, "%s: workspace of %zu bytes, needs %zu", name, workspace_bytes,
                  vt_point_workspace(v, B, Cg, O, Od));
    const int R = (int)(O + Od);
    const float* s = folded + (C + Cg) * R;
    float* u = nullptr;
    if (Cg > 0) {
        u = static_cast<float*>(workspace);
        const int64_t total = B * 3 * R;
        hipLaunchKernelGGL(vn_cloud_term_kernel, dim3((unsigned)svnet_cdiv(total, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, g, folded, total,
                           (int)C, (int)Cg, R, u);
        SVNET_CHECK_LAUNCH("vn_cloud_term_kernel");
    }
    const bool share = Od == 1 && O != 1;
    const int npt = vt_point_tiles(N, C, share);
    const size_t lds = (size_t)vt_point_lds(npt, C, share);
    SVNET_REQUIRE(lds <= (size_t)VT_LDS_MAX, SVNET_E_UNSUPPORTED, "%s: an image of %zu bytes does not fit LDS", name, lds);
    if (lds > 64 * 1024) {
        bool ok = true;
        SVNET_LDS_OPTIN(ok, VT_LDS_MAX, name, reinterpret_cast<const void*>(vn_point_kernel<1, false, VtLeaky>),
                        reinterpret_cast<const void*>(vn_point_kernel<1, true, VtLeaky>), reinterpret_cast<const void*>(vn_point_kernel<2, false, VtLeaky>),
                        reinterpret_cast<const void*>(vn_point_kernel<2, true, VtLeaky>), reinterpret_cast<const void*>(vn_point_kernel<4, false, VtLeaky>),
                        reinterpret_cast<const void*>(vn_point_kernel<4, true, VtLeaky>));
        if (!ok) return SVNET_E_LAUNCH;
    }
    const dim3 grid((unsigned)svnet_cdiv(N, 16 * npt), (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
#define VT_POINT(NPT, SHARE) vt_launch_point<NPT, SHARE, VtLeaky>(grid, lds, st, x, folded, s, s + O, u, (int)N, (int)C, (int)O, slope, out)
    if (share) {
        if (npt == 4) VT_POINT(4, true);
        else if (npt == 2) VT_POINT(2, true);
        else VT_POINT(1, true);
    } else {
        if (npt == 4) VT_POINT(4, false);
        else if (npt == 2) VT_POINT(2, false);
        else VT_POINT(1, false);
    }
#undef VT_POINT
    SVNET_CHECK_LAUNCH("vn_point_kernel");
    return SVNET_OK;
}

int vt_point_norm_fold(const VtEnvelope& v, const char* name, const float* w_feat, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, int64_t C, int64_t O, float eps, float* folded, void* stream) {
    SVNET_REQUIRE(w_feat && gamma && beta && running_mean && running_var && folded, SVNET_E_ARG,
                  "%s: null w_feat / gamma / beta / running_mean / running_var / folded", name);
    SVNET_REQUIRE(vt_point_ok(v, 1, C, 0, O, O), SVNET_E_UNSUPPORTED, "%s: C %lld, O %lld: needs 1 <= C <= %d, 1 <= O <= %d", name, (long long)C, (long long)O,
                  v.max_c, v.max_o);
    const int64_t total = C * O + O;
    hipLaunchKernelGGL(vn_point_fold_kernel, dim3((unsigned)svnet_cdiv(total, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, w_feat, w_feat, gamma,
                       beta, running_mean, running_var, (int)C, (int)O, 0, eps, folded);
    SVNET_CHECK_LAUNCH("vn_point_fold_kernel");
    return SVNET_OK;
}

int vt_point_norm(const VtEnvelope& v, const char* name, const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, float* out,
                  void* stream) {
    SVNET_REQUIRE(x && folded && out, SVNET_E_ARG, "%s: null x / folded / out", name);
    SVNET_REQUIRE(vt_batch_ok(B), SVNET_E_ARG, "%s: B %lld must lie in 1 .. %d", name, (long long)B, VT_MAX_B);
    SVNET_REQUIRE(vt_point_ok(v, N, C, 0, O, O), SVNET_E_UNSUPPORTED, "%s: N %lld, C %lld, O %lld: needs 1 <= N <= %d, 1 <= C <= %d, 1 <= O <= %d", name,
                  (long long)N, (long long)C, (long long)O, VN_MAX_N, v.max_c, v.max_o);
    const float* s = folded + C * O;
    const int npt = vt_point_tiles(N, C, false);
    const size_t lds = (size_t)vt_point_lds(npt, C, false);
    SVNET_REQUIRE(lds <= (size_t)VT_LDS_MAX, SVNET_E_UNSUPPORTED, "%s: an image of %zu bytes does not fit LDS", name, lds);
    if (lds > 64 * 1024) {
        bool ok = true;
        SVNET_LDS_OPTIN(ok, VT_LDS_MAX, name, reinterpret_cast<const void*>(vn_point_kernel<1, false, VtNormOnly>),
                        reinterpret_cast<const void*>(vn_point_kernel<2, false, VtNormOnly>), reinterpret_cast<const void*>(vn_point_kernel<4, false, VtNormOnly>));
        if (!ok) return SVNET_E_LAUNCH;
    }
    const dim3 grid((unsigned)svnet_cdiv(N, 16 * npt), (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
#define VT_NORM(NPT) vt_launch_point<NPT, false, VtNormOnly>(grid, lds, st, x, folded, s, s + O, nullptr, (int)N, (int)C, (int)O, 0.f, out)
    if (npt == 4) VT_NORM(4);
    else if (npt == 2) VT_NORM(2);
    else VT_NORM(1);
#undef VT_NORM
    SVNET_CHECK_LAUNCH("vn_point_kernel");
    return SVNET_OK;
}

int vt_cloud_mean(const VtEnvelope& v, const char* name, const float* x, int64_t B, int64_t C, int64_t N, float* m, void* stream) {
    SVNET_REQUIRE(x && m, SVNET_E_ARG, "%s: null x / m", name);
    SVNET_REQUIRE(vt_batch_ok(B), SVNET_E_ARG, "%s: B %lld must lie in 1 .. %d", name, (long long)B, VT_MAX_B);
    SVNET_REQUIRE(N >= 1 && N <= VN_MAX_N && C >= 1 && C <= v.max_c, SVNET_E_UNSUPPORTED, "%s: N %lld, C %lld: needs 1 <= N <= %d, 1 <= C <= %d", name,
                  (long long)N, (long long)C, VN_MAX_N, v.max_c);
    const int64_t rows = B * C * 3;
    const int runs = (int)svnet_cdiv(N, VT_RUN), rpb = runs >= VT_THREADS ? 1 : VT_THREADS / runs;
    hipLaunchKernelGGL(vn_cloud_mean_kernel, dim3((unsigned)svnet_cdiv(rows, rpb)), dim3(VT_THREADS), 0, (hipStream_t)stream, x, rows, (int)N, runs, rpb, m);
    SVNET_CHECK_LAUNCH("vn_cloud_mean_kernel");
    return SVNET_OK;
}

size_t vt_std_pool_workspace(const VtEnvelope& v, int64_t B, int64_t N, int64_t C, int64_t Cg) {
    if (!vt_batch_ok(B) || !vt_std_ok(v, N, C, Cg, 1)) return 0;
    return (size_t)2 * (size_t)svnet_cdiv(N, VT_RUN) * (size_t)B * 3 * (size_t)(C + Cg) * sizeof(float);
}

int vt_std_pool(const VtEnvelope& v, const char* name, const float* x, const float* g, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C,
                int64_t Cg, int64_t Cy, void* workspace, size_t workspace_bytes, float* h, void* stream) {
    SVNET_REQUIRE(x && y && w_lin && workspace && h && (Cg <= 0 || g), SVNET_E_ARG, "%s: null x / y / w_lin / workspace / h, or g with Cg > 0", name);
    SVNET_REQUIRE(vt_batch_ok(B), SVNET_E_ARG, "%s: B %lld must lie in 1 .. %d", name, (long long)B, VT_MAX_B);
    SVNET_REQUIRE(vt_std_ok(v, N, C, Cg, Cy), SVNET_E_UNSUPPORTED,
                  "%s: N %lld, C %lld, Cg %lld, Cy %lld: needs 1 <= N <= %d, 1 <= C <= %d, 0 <= Cg <= %d, 1 <= Cy <= %d", name, (long long)N, (long long)C,
                  (long long)Cg, (long long)Cy, VN_MAX_N, v.max_c, v.max_c, v.max_c);
    SVNET_REQUIRE(workspace_bytes >= vt_std_pool_workspace(v, B, N, C, Cg), SVNET_E_WORKSPACE, "%s: workspace of %zu bytes, needs %zu", name, workspace_bytes,
                  vt_std_pool_workspace(v, B, N, C, Cg));
    const int64_t runs = svnet_cdiv(N, VT_RUN), cols = 3 * (C + Cg), total = B * cols;
    float* pmax = static_cast<float*>(workspace);
    float* psum = pmax + runs * total;
    hipLaunchKernelGGL(vn_std_pool_kernel, dim3((unsigned)runs, (unsigned)B), dim3(VT_THREADS), 0, (hipStream_t)stream, x, g ? g : x, y, w_lin, (int)N, (int)C,
                       (int)Cg, (int)Cy, pmax, psum);
    SVNET_CHECK_LAUNCH("vn_std_pool_kernel");
    hipLaunchKernelGGL(vn_std_finish_kernel, dim3((unsigned)svnet_cdiv(total, VT_THREADS)), dim3(VT_THREADS), 0, (hipStream_t)stream, pmax, psum, runs, total,
                       (int)cols, (int)N, h);
    SVNET_CHECK_LAUNCH("vn_std_finish_kernel");
    return SVNET_OK;
}

int vt_std_coords(const VtEnvelope& v, const char* name, const float* x, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cy,
                  float* e, void* stream) {
    SVNET_REQUIRE(x && y && w_lin && e, SVNET_E_ARG, "%s: null x / y / w_lin / e", name);
    SVNET_REQUIRE(vt_batch_ok(B), SVNET_E_ARG, "%s: B %lld must lie in 1 .. %d", name, (long long)B, VT_MAX_B);
    SVNET_REQUIRE(vt_std_ok(v, N, C, 0, Cy), SVNET_E_UNSUPPORTED, "%s: N %lld, C %lld, Cy %lld: needs 1 <= N <= %d, 1 <= C <= %d, 1 <= Cy <= %d", name,
                  (long long)N, (long long)C, (long long)Cy, VN_MAX_N, v.max_c, v.max_c);
    hipLaunchKernelGGL(vn_std_coords_kernel, dim3((unsigned)svnet_cdiv(N, VT_RUN), (unsigned)B), dim3(VT_THREADS), 0, (hipStream_t)stream, x, y, w_lin, (int)N,
                       (int)C, (int)Cy, e);
    SVNET_CHECK_LAUNCH("vn_std_coords_kernel");
    return SVNET_OK;
}

}  // namespace

// ---- the entries: V is the envelope, INFIX what the wide twin's name carries behind the stage's (include/svnet_hip.h states the rule)
#define VT_ENTRIES(V, INFIX)                                                                                                                                   \
    extern "C" int svnet_vn_point##INFIX##_supported(int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od) { return vt_point_ok(V, N, C, Cg, O, Od) ? 1 : 0; } \
    extern "C" size_t svnet_vn_point##INFIX##_workspace_bytes(int64_t B, int64_t Cg, int64_t O, int64_t Od) { return vt_point_workspace(V, B, Cg, O, Od); }    \
    extern "C" int svnet_vn_point##INFIX##_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean, \
                                                    const float* running_var, int64_t C, int64_t Cg, int64_t O, int64_t Od, float eps, float* folded,         \
                                                    void* stream) {                                                                                            \
        return vt_point_fold(V, "svnet_vn_point" #INFIX "_fold_f32", w_feat, w_dir, gamma, beta, running_mean, running_var, C, Cg, O, Od, eps, folded, stream); \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_point##INFIX##_f32(const float* x, const float* g, const float* folded, int64_t B, int64_t N, int64_t C, int64_t Cg, int64_t O,    \
                                               int64_t Od, float slope, void* workspace, size_t workspace_bytes, float* out, void* stream) {                   \
        return vt_point(V, "svnet_vn_point" #INFIX "_f32", x, g, folded, B, N, C, Cg, O, Od, slope, workspace, workspace_bytes, out, stream);                 \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_point_norm##INFIX##_supported(int64_t N, int64_t C, int64_t O) { return vt_point_ok(V, N, C, 0, O, O) ? 1 : 0; }                   \
    extern "C" int svnet_vn_point_norm##INFIX##_fold_f32(const float* w_feat, const float* gamma, const float* beta, const float* running_mean,                \
                                                         const float* running_var, int64_t C, int64_t O, float eps, float* folded, void* stream) {             \
        return vt_point_norm_fold(V, "svnet_vn_point_norm" #INFIX "_fold_f32", w_feat, gamma, beta, running_mean, running_var, C, O, eps, folded, stream);     \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_point_norm##INFIX##_f32(const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, float* out,               \
                                                    void* stream) {                                                                                            \
        return vt_point_norm(V, "svnet_vn_point_norm" #INFIX "_f32", x, folded, B, N, C, O, out, stream);                                                      \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_cloud_mean##INFIX##_f32(const float* x, int64_t B, int64_t C, int64_t N, float* m, void* stream) {                                 \
        return vt_cloud_mean(V, "svnet_vn_cloud_mean" #INFIX "_f32", x, B, C, N, m, stream);                                                                   \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_std_pool##INFIX##_supported(int64_t N, int64_t C, int64_t Cg, int64_t Cy) { return vt_std_ok(V, N, C, Cg, Cy) ? 1 : 0; }           \
    extern "C" size_t svnet_vn_std_pool##INFIX##_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t Cg) { return vt_std_pool_workspace(V, B, N, C, Cg); } \
    extern "C" int svnet_vn_std_pool##INFIX##_f32(const float* x, const float* g, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C,         \
                                                  int64_t Cg, int64_t Cy, void* workspace, size_t workspace_bytes, float* h, void* stream) {                   \
        return vt_std_pool(V, "svnet_vn_std_pool" #INFIX "_f32", x, g, y, w_lin, B, N, C, Cg, Cy, workspace, workspace_bytes, h, stream);                      \
    }                                                                                                                                                          \
    extern "C" int svnet_vn_std_coords##INFIX##_supported(int64_t N, int64_t C, int64_t Cy) { return vt_std_ok(V, N, C, 0, Cy) ? 1 : 0; }                      \
    extern "C" int svnet_vn_std_coords##INFIX##_f32(const float* x, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cy, float* e, \
                                                    void* stream) {                                                                                            \
        return vt_std_coords(V, "svnet_vn_std_coords" #INFIX "_f32", x, y, w_lin, B, N, C, Cy, e, stream);                                                     \
    }

VT_ENTRIES(VT_BASE, )
VT_ENTRIES(VT_WIDE, _wide)
#undef VT_ENTRIES
