// Multi-scale grouping (models/utils/pointnet_util.py:210-267 PointNetSetAbstractionMsg.forward): the same centres grouped at up to
// SVNET_MSG_MAX_SCALES radii by ONE query pass over the cloud, ONE grouping launch and ONE ordered sum for the gradient.  The contract
// is in svnet_amd/group.py's docstring ("Multi-scale grouping") and include/svnet_hip.h; tests/msg_ref.py restates it.  Every scale's
// list is exactly what ball_query_kernel (group.hip) gives for its radius: the same sq_len distance (pointset.h), the same <=, order,
// padding and empty-group rule.  A row of the grouped output is [attributes | centred xyz], D columns then 3 - the reference's Msg
// order, not group_points_kernel's.  The kernels follow the single-scale ones of group.hip and pointset_grad.hip, whose launch shapes
// are restated here (GM_*): this file is a translation unit of its own, built with -ffp-contract=off like them (Makefile, NO_CONTRACT).
#include "pointset.h"

namespace {

constexpr int GM_THREADS = 256;                                  // every kernel here: four waves
constexpr int GM_MAX_ROWS = 1024;                                // grouping: output rows per workgroup, at most
constexpr int GM_UNITS = 4096;                                   // grouping: floats or float4s per workgroup, about
static_assert(POINTSET_TILE % SVNET_WAVE == 0, "ball_query_msg_kernel takes the tile in whole 64-candidate steps");

// ---- the scales of a multi-scale grouping call handed to the kernels by value: no device copy.
// A centre's row of the concatenated index table is the scales' lists end to end, list i at columns off[i] .. off[i] + nsample[i] - 1
// of ktot.  msg_scales fills one from the caller's host arrays (r2 may be null where no radius is needed); false unless
// svnet_group_msg_supported.  MsgRows: one pointer per scale, the outputs of the grouping or the upstream gradients of its backward.
struct MsgScales {
    float r2[SVNET_MSG_MAX_SCALES];
    int nsample[SVNET_MSG_MAX_SCALES], off[SVNET_MSG_MAX_SCALES];
    int scales, ktot;
};
struct MsgRows { float* p[SVNET_MSG_MAX_SCALES]; };
inline bool msg_scales(int64_t N, int64_t S, int64_t scales, const float* r2, const int64_t* nsample, int64_t D, MsgScales& sc) {
    if (!svnet_group_msg_supported(N, S, scales, nsample, D)) return false;
    sc = MsgScales{};
    sc.scales = (int)scales;
    for (int i = 0; i < sc.scales; ++i) {
        sc.r2[i] = r2 ? r2[i] : 0.f;
        sc.nsample[i] = (int)nsample[i];
        sc.off[i] = sc.ktot;
        sc.ktot += sc.nsample[i];
    }
    return true;
}


// ---- multi-scale grouping (models/utils/pointnet_util.py:210-267).  The scales of a call travel to the kernels by value.
// ball_query_msg_kernel<R>: ball_query_kernel with `found` and `first` per (centre, scale).  A candidate's distance is computed
// once; every scale that is not yet full takes its own ballot of dist <= r2[i] and appends to its own list, columns off[i] ..
// off[i] + nsample[i] - 1 of the centre's row of ktot; a full scale's ballot is skipped (wave-uniform), the wave leaves a centre
// when all its scales are full.  R is a template argument so that the per-scale state is indexed at compile time: registers.
constexpr int BQM_CPW = 8;                                       // centres per wave: 8 x 4 scales x (found, first) stay in registers
constexpr int BQM_CENTRES = (GM_THREADS / SVNET_WAVE) * BQM_CPW;

template <int R>
__global__ __launch_bounds__(GM_THREADS) void ball_query_msg_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int64_t N,
                                                                    int64_t S, int64_t chunks, MsgScales sc, int64_t* __restrict__ idx,
                                                                    int* __restrict__ count) {
    __shared__ __align__(16) float tile[POINTSET_TILE * 3];
    const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
    const int64_t b = blockIdx.x / chunks;
    const int64_t s0 = (blockIdx.x % chunks) * BQM_CENTRES + wave * BQM_CPW;          // this wave's first centre
    const int mine = (int)(S - s0 < 0 ? 0 : S - s0 < BQM_CPW ? S - s0 : BQM_CPW);     // its centres: 0 .. BQM_CPW
    const float* pts = xyz + b * N * 3;
    const float* ctr = new_xyz + (b * S + s0) * 3;
    int64_t* rows = idx + (b * S + s0) * sc.ktot;

    int found[BQM_CPW][R], first[BQM_CPW][R];
#pragma unroll
    for (int c = 0; c < BQM_CPW; ++c)
#pragma unroll
        for (int i = 0; i < R; ++i) { found[c][i] = 0; first[c][i] = 0; }
    int pending = mine > 0;
    for (int64_t base = 0; base < N; base += POINTSET_TILE) {
        const int cnt = (int)(N - base < POINTSET_TILE ? N - base : POINTSET_TILE);
        if (base && !__syncthreads_or(pending)) break;           // the previous tile has been read by every wave; all full: done
        stage_xyz<GM_THREADS>(tile, pts + base * 3, cnt, t);
        __syncthreads();
        pending = 0;
#pragma unroll
        for (int c = 0; c < BQM_CPW; ++c) {
            bool open = false;
#pragma unroll
            for (int i = 0; i < R; ++i) open |= found[c][i] < sc.nsample[i];
            if (c >= mine || !open) continue;                    // wave-uniform
            const float qx = ctr[3 * c], qy = ctr[3 * c + 1], qz = ctr[3 * c + 2];
            int64_t* row = rows + (int64_t)c * sc.ktot;
            for (int n0 = 0; n0 < cnt; n0 += SVNET_WAVE) {
                const int n = n0 + lane;
                float dist = SVNET_QNAN;                         // past the tile's points: never inside
                if (n < cnt) {
                    const float d0 = qx - tile[3 * n], d1 = qy - tile[3 * n + 1], d2 = qz - tile[3 * n + 2];
                    dist = sq_len(d0, d1, d2);
                }
                open = false;
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    if (found[c][i] >= sc.nsample[i]) continue;  // a full scale: no ballot (wave-uniform)
                    const bool inside = dist <= sc.r2[i];
                    const unsigned long long mask = __ballot(inside);
                    if (mask) {
                        if (found[c][i] == 0) first[c][i] = (int)base + n0 + (int)__builtin_ctzll(mask);
                        const int slot = found[c][i] + lanes_below(mask);
                        if (inside && slot < sc.nsample[i]) row[sc.off[i] + slot] = (int64_t)((int)base + n);
                        found[c][i] += (int)__popcll(mask);
                    }
                    open |= found[c][i] < sc.nsample[i];
                }
                if (!open) break;
            }
            pending |= open;
        }
    }
#pragma unroll
    for (int c = 0; c < BQM_CPW; ++c) {
        if (c >= mine) continue;
        int64_t* row = rows + (int64_t)c * sc.ktot;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int f = found[c][i] < sc.nsample[i] ? found[c][i] : sc.nsample[i];
            for (int j = f + lane; j < sc.nsample[i]; j += SVNET_WAVE) row[sc.off[i] + j] = first[c][i];     // 0 when nothing was found
            if (lane == 0) count[(b * S + s0 + c) * R + i] = f;
        }
    }
}

// group_points_kernel over the rows of the concatenated table, R = B * S * ktot of them: a row (centre cs, slot j) belongs to the
// scale i with off[i] <= j < off[i] + nsample[i] and lands in row cs * nsample[i] + (j - off[i]) of out_i.  A row is [attributes |
// centred xyz]: the attribute copy has the output's column, so in the float4 form (3 + D a multiple of 4, hence D % 4 == 1) every
// unit but the last is four attributes and the last is the D-th attribute and the three coordinates.
template <bool VEC>
__global__ __launch_bounds__(GM_THREADS) void group_points_msg_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                      const float* __restrict__ points, const int64_t* __restrict__ idx,
                                                                      int64_t N, int64_t S, MsgScales sc, int D, int U, int rows_per_block,
                                                                      int64_t R, MsgRows outs) {
    __shared__ int64_t s_src[GM_MAX_ROWS];      // b * N + the row's point
    __shared__ int s_ctr[GM_MAX_ROWS];          // b * S + the row's centre
    __shared__ float* s_dst[GM_MAX_ROWS];       // the row of its scale's output
    const int t = threadIdx.x;
    const int W = 3 + D;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int rows = (int)(R - r0 < rows_per_block ? R - r0 : rows_per_block);
    for (int r = t; r < rows; r += GM_THREADS) {
        const int64_t cs = (r0 + r) / sc.ktot;
        const int j = (int)((r0 + r) % sc.ktot);
        float* out = outs.p[0];
        int ns = sc.nsample[0], off = 0;
#pragma unroll
        for (int i = 1; i < SVNET_MSG_MAX_SCALES; ++i)
            if (i < sc.scales && j >= sc.off[i]) { out = outs.p[i]; ns = sc.nsample[i]; off = sc.off[i]; }
        s_src[r] = (cs / S) * N + clamp_index(idx[r0 + r], N);
        s_ctr[r] = (int)cs;
        s_dst[r] = out + (cs * ns + (j - off)) * W;
    }
    __syncthreads();
    const int total = rows * U;
    const int qstep = GM_THREADS / U, rstep = GM_THREADS % U;
    int row = t / U, col = t % U;
    for (int e = t; e < total; e += GM_THREADS) {
        const float* p = xyz + s_src[row] * 3;
        const float* q = new_xyz + (int64_t)s_ctr[row] * 3;
        const float* a = points + s_src[row] * D;                // (D = 0: never read)
        float* dst = s_dst[row];
        if (VEC) {
            float4 v;
            const float* s = a + 4 * col;
            v.x = s[0];
            if (col == U - 1) {
                v.y = p[0] - q[0]; v.z = p[1] - q[1]; v.w = p[2] - q[2];
            } else {
                v.y = s[1]; v.z = s[2]; v.w = s[3];
            }
            reinterpret_cast<float4*>(dst)[col] = v;
        } else {
            dst[col] = col < D ? a[col] : p[col - D] - q[col - D];
        }
        col += rstep; row += qstep;
        if (col >= U) { col -= U; ++row; }
    }
}

// The multi-scale form (group_points_msg_kernel above).  The lists are those of the concatenated table, E = S * ktot edges per
// cloud: edge e = s ktot + j lies in the scale i with off[i] <= j < off[i] + nsample[i], and its term is column c - the attributes
// come first in a multi-scale row - of row s nsample[i] + (j - off[i]) of that scale's upstream gradient.  Ascending e is, per centre,
// scale 0's slots, then scale 1's, ...  An edge is wave-uniform, so finding its row is scalar work.
__device__ __forceinline__ const float* msg_row(int e, int64_t bS, const MsgScales& sc, const MsgRows& dg, int W) {
    const int s = e / sc.ktot, j = e - s * sc.ktot;
    const float* base = dg.p[0];
    int ns = sc.nsample[0], off = 0;
#pragma unroll
    for (int i = 1; i < SVNET_MSG_MAX_SCALES; ++i)
        if (i < sc.scales && j >= sc.off[i]) { base = dg.p[i]; ns = sc.nsample[i]; off = sc.off[i]; }
    return base + ((bS + s) * ns + (j - off)) * W;
}

__global__ __launch_bounds__(GM_THREADS) void group_points_msg_bwd_kernel(MsgRows dg, const int32_t* __restrict__ rev_start,
                                                                           const int32_t* __restrict__ rev_edge, int64_t N, int64_t S,
                                                                           MsgScales sc, int D, int64_t BN, float* __restrict__ dpoints) {
    const int lane = lane_id();
    const int64_t bn = (int64_t)blockIdx.x * (GM_THREADS / SVNET_WAVE) + (threadIdx.x >> 6);
    if (bn >= BN) return;
    const int64_t b = bn / N, n = bn % N;
    const int32_t* st = rev_start + b * (N + 1) + n;
    const int lo = st[0], hi = st[1];
    const int32_t* list = rev_edge + b * S * sc.ktot;
    const int W = 3 + D;
    const int64_t bS = b * S;
    float* dst = dpoints + bn * D;
    for (int c0 = 0; c0 < D; c0 += SVNET_WAVE) {
        const int c = c0 + lane;
        const bool on = c < D;
        float acc = 0.f;                                         // an empty list: +0, written
        int i = lo;
        if (i < hi) {                                            // the first term itself (a -0 stays a -0)
            const float* r = msg_row(list[i++], bS, sc, dg, W);
            if (on) acc = r[c];
        }
        for (; i + 4 <= hi; i += 4) {
            const float* r0 = msg_row(list[i], bS, sc, dg, W);
            const float* r1 = msg_row(list[i + 1], bS, sc, dg, W);
            const float* r2 = msg_row(list[i + 2], bS, sc, dg, W);
            const float* r3 = msg_row(list[i + 3], bS, sc, dg, W);
            if (on) {
                const float t0 = r0[c], t1 = r1[c], t2 = r2[c], t3 = r3[c];
                acc = (((acc + t0) + t1) + t2) + t3;
            }
        }
        for (; i < hi; ++i) {
            const float* r = msg_row(list[i], bS, sc, dg, W);
            if (on) acc += r[c];
        }
        if (on) dst[c] = acc;
    }
}

// output rows per workgroup of the grouping for U units per row
inline int gm_rows(int64_t U) {
    const int64_t r = GM_UNITS / U;
    return (int)(r < 1 ? 1 : r > GM_MAX_ROWS ? GM_MAX_ROWS : r);
}

}  // namespace

extern "C" int svnet_group_msg_supported(int64_t N, int64_t S, int64_t scales, const int64_t* nsample, int64_t D) {
    if (!nsample || scales < 1 || scales > SVNET_MSG_MAX_SCALES) return 0;
    for (int64_t i = 0; i < scales; ++i)
        if (!svnet_group_supported(N, S, nsample[i], D)) return 0;
    return 1;
}

extern "C" int svnet_ball_query_msg_f32(const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, int64_t scales, const float* r2,
                                        const int64_t* nsample, int64_t* idx, int* count, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && r2 && nsample && idx && count, SVNET_E_ARG,
                  "svnet_ball_query_msg_f32: null xyz / new_xyz / r2 / nsample / idx / count");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_ball_query_msg_f32: B %lld must be positive", (long long)B);
    MsgScales sc;
    SVNET_REQUIRE(msg_scales(N, S, scales, r2, nsample, 0, sc), SVNET_E_UNSUPPORTED,
                  "svnet_ball_query_msg_f32: N %lld, S %lld, scales %lld: needs 1 <= scales <= %d, every 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1",
                  (long long)N, (long long)S, (long long)scales, SVNET_MSG_MAX_SCALES, (long long)SVNET_KNN_MAX_N);
    SVNET_REQUIRE(B <= 0x7fffffffll / S / sc.ktot, SVNET_E_UNSUPPORTED, "svnet_ball_query_msg_f32: B %lld x S %lld x nsample %d indices > 2^31 - 1",
                  (long long)B, (long long)S, sc.ktot);
    const CloudGrid grid = cloud_grid(B, S, BQM_CENTRES);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_ball_query_msg_f32: B %lld x ceil(S %lld / %d) workgroups > 2^31 - 1",
                  (long long)B, (long long)S, BQM_CENTRES);
    const dim3 blocks((unsigned)grid.blocks), threads(GM_THREADS);
    switch (sc.scales) {
        case 1: hipLaunchKernelGGL(ball_query_msg_kernel<1>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        case 2: hipLaunchKernelGGL(ball_query_msg_kernel<2>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        case 3: hipLaunchKernelGGL(ball_query_msg_kernel<3>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        default: hipLaunchKernelGGL(ball_query_msg_kernel<4>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
    }
    SVNET_CHECK_LAUNCH("ball_query_msg_kernel");
    return SVNET_OK;
}

extern "C" int svnet_group_points_msg_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N,
                                          int64_t S, int64_t scales, const int64_t* nsample, int64_t D, float* out0, float* out1, float* out2,
                                          float* out3, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && nsample, SVNET_E_ARG, "svnet_group_points_msg_f32: null xyz / new_xyz / idx / nsample");
    SVNET_REQUIRE(points || D == 0, SVNET_E_ARG, "svnet_group_points_msg_f32: null points with D %lld > 0", (long long)D);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_group_points_msg_f32: B %lld must be positive", (long long)B);
    MsgScales sc;
    SVNET_REQUIRE(msg_scales(N, S, scales, nullptr, nsample, D, sc), SVNET_E_UNSUPPORTED,
                  "svnet_group_points_msg_f32: N %lld, S %lld, scales %lld, D %lld: needs 1 <= scales <= %d, every 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1, D >= 0",
                  (long long)N, (long long)S, (long long)scales, (long long)D, SVNET_MSG_MAX_SCALES, (long long)SVNET_KNN_MAX_N);
    SVNET_REQUIRE(B <= 0x7fffffffll / S / sc.ktot, SVNET_E_UNSUPPORTED, "svnet_group_points_msg_f32: B %lld x S %lld x nsample %d rows > 2^31 - 1",
                  (long long)B, (long long)S, sc.ktot);
    const MsgRows outs = {{out0, out1, out2, out3}};
    const int64_t R = B * S * sc.ktot, W = 3 + D;
    bool vec = W % 4 == 0;
    for (int i = 0; i < sc.scales; ++i) {
        SVNET_REQUIRE(outs.p[i], SVNET_E_ARG, "svnet_group_points_msg_f32: null out%d with %d scales", i, sc.scales);
        vec = vec && (uintptr_t)outs.p[i] % 16 == 0;
    }
    if (!points) points = xyz;                                   // D = 0: never read
    const int64_t U = vec ? W / 4 : W;
    const int rpb = gm_rows(U);
    const unsigned blocks = (unsigned)svnet_cdiv(R, rpb);
    if (vec)
        hipLaunchKernelGGL(group_points_msg_kernel<true>, dim3(blocks), dim3(GM_THREADS), 0, (hipStream_t)stream, xyz, new_xyz, points, idx, N, S,
                           sc, (int)D, (int)U, rpb, R, outs);
    else
        hipLaunchKernelGGL(group_points_msg_kernel<false>, dim3(blocks), dim3(GM_THREADS), 0, (hipStream_t)stream, xyz, new_xyz, points, idx, N, S,
                           sc, (int)D, (int)U, rpb, R, outs);
    SVNET_CHECK_LAUNCH("group_points_msg_kernel");
    return SVNET_OK;
}

extern "C" int svnet_group_points_msg_bwd_f32(const float* dg0, const float* dg1, const float* dg2, const float* dg3, const int32_t* rev_start,
                                              const int32_t* rev_edge, int64_t B, int64_t N, int64_t S, int64_t scales, const int64_t* nsample,
                                              int64_t D, float* dpoints, void* stream) {
    SVNET_REQUIRE(rev_start && rev_edge && nsample && dpoints, SVNET_E_ARG, "svnet_group_points_msg_bwd_f32: null rev_start / rev_edge / nsample / dpoints");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_group_points_msg_bwd_f32: B %lld must be positive", (long long)B);
    MsgScales sc;
    SVNET_REQUIRE(D >= 1 && msg_scales(N, S, scales, nullptr, nsample, D, sc) && svnet_pointset_reverse_supported(S, sc.ktot, N), SVNET_E_UNSUPPORTED,
                  "svnet_group_points_msg_bwd_f32: N %lld, S %lld, scales %lld, D %lld: needs 1 <= scales <= %d, every 1 <= nsample <= N <= %lld, S * sum nsample <= 2^31 - 1, D >= 1",
                  (long long)N, (long long)S, (long long)scales, (long long)D, SVNET_MSG_MAX_SCALES, (long long)SVNET_KNN_MAX_N);
    SVNET_REQUIRE(B <= 0x7fffffffll / S / sc.ktot, SVNET_E_UNSUPPORTED, "svnet_group_points_msg_bwd_f32: B %lld x S %lld x nsample %d rows > 2^31 - 1",
                  (long long)B, (long long)S, sc.ktot);
    const MsgRows dg = {{const_cast<float*>(dg0), const_cast<float*>(dg1), const_cast<float*>(dg2), const_cast<float*>(dg3)}};
    for (int i = 0; i < sc.scales; ++i)
        SVNET_REQUIRE(dg.p[i], SVNET_E_ARG, "svnet_group_points_msg_bwd_f32: null dg%d with %d scales", i, sc.scales);
    const CloudGrid grid = cloud_grid(1, B * N, GM_THREADS / SVNET_WAVE);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_group_points_msg_bwd_f32: B %lld x N %lld / %d workgroups > 2^31 - 1", (long long)B,
                  (long long)N, GM_THREADS / SVNET_WAVE);
    hipLaunchKernelGGL(group_points_msg_bwd_kernel, dim3((unsigned)grid.blocks), dim3(GM_THREADS), 0, (hipStream_t)stream, dg, rev_start, rev_edge,
                       N, S, sc, (int)D, B * N, dpoints);
    SVNET_CHECK_LAUNCH("group_points_msg_bwd_kernel");
    return SVNET_OK;
}
