// Ball query and neighbourhood grouping for one radius (models/utils/pointnet_util.py:87-107 query_ball_point,
// 110-143 sample_and_group without its sampling) and for up to SVNET_MSG_MAX_SCALES radii around the same centres (:210-267
// PointNetSetAbstractionMsg.forward): the step that turns sampled centres into fixed-size local neighbourhoods - the third point-set
// helper of that file beside farthest point sampling (fps.hip) and the three-nearest-neighbour interpolation (propagate.hip).  The
// query and the grouping kernel are each stated ONCE, for 1 .. SVNET_MSG_MAX_SCALES scales; the single-scale entry points launch
// the one-scale form.  The gradient of the multi-scale grouping is here too; the single-scale one is in pointset_grad.hip.
//
// For one cloud, points xyz [N,3], centres new_xyz [S,3], optional attributes points [N,D] (channel-last), scales i = 0 .. R-1 with
// r2_i and nsample_i; the contract is in svnet_amd/group.py's docstring, tests/group_ref.py and tests/msg_ref.py restate it
// independently:
//   d_c = fl(new_xyz[s,c] - xyz[n,c]);  dist[s,n] = sq_len(d_0, d_1, d_2)            (pointset.h: the distance, single-rounded)
//   inside_i(s,n) = dist[s,n] <= r2_i                 (a NaN distance compares false: never inside)
//   list i of centre s = the first nsample_i inside_i points in ascending point index, slots past the number found = the first
//                        inside index; count[s,i] = min(found, nsample_i); an empty group: count 0, every slot 0
//   idx [S,Ktot], Ktot = sum nsample_i: a centre's row is its lists end to end, list i at columns off_i .. off_i + nsample_i - 1;
//                        one scale: idx [S,nsample], count [S]
//   grouped row of (s, slot j of list i), n = idx clamped into [0, N):  centred[c] = fl(xyz[n,c] - new_xyz[s,c]), attributes
//                        points[n,:] copied bit for bit;  svnet_group_points_f32 writes [centred | attributes] into out [S,nsample,3+D],
//                        svnet_group_points_msg_f32 [attributes | centred] - the reference's Msg order - into out_i [S,nsample_i,D+3]
//   gradient (R tensors) dpoints[n,c] = the ordered sum (pointset_grad.hip's header) of the upstream gradients' column c over the
//                        edges e = s Ktot + j that point to n, in ascending e: per centre scale 0's slots, then scale 1's, ...
// Every product, sum and difference is its own correctly rounded fp32 operation (pointset.h).
//
// ball_query<R>: one wave per centre at a time, BQ_CPW centres after each other per wave, four waves (32 centres) per workgroup, the
// workgroups of a cloud side by side.  The cloud's points pass through LDS in tiles of POINTSET_TILE points (pointset.h: stage_xyz,
// no padding), shared by the workgroup's 32 centres; lane l of a wave reads point n0 + l, a stride of three dwords across the
// lanes (odd: no bank conflict).  A step takes 64 candidates in index order and computes a candidate's distance once; every scale
// that is not yet full takes its own ballot of dist <= r2_i: the ballot is the step's membership mask, a lane's slot is found +
// (set lanes below it) (lanes_below, wave.h), so the list is written in order and coalesced, and `found` grows by the mask's
// population.  A full scale's ballot is skipped and the wave leaves a centre's loop as soon as all its scales are full - uniform per
// wave, no divergence - which is the point of the kernel: at PointNet++ radii most groups fill after a fraction of N.  `found` and
// the first inside index of every (centre, scale) are wave-uniform and survive the tile loop - R is a template argument so that they
// are indexed at compile time, the wave's index is taken with readfirstlane so that the compiler knows they are uniform: scalar
// registers and scalar branches - and a workgroup whose centres are all full skips the remaining tiles (the vote rides on
// the barrier the tile swap needs anyway).  One padding pass per list fills the slots past `found`.  Every index written is a
// candidate's own or 0: inside [0, N), always.
// group_points<VEC, XYZ_LAST, ONE>: a row gather over the B S Ktot rows of the index table.  A workgroup takes gp_rows(U) consecutive
// rows (one row = one (centre, slot) pair), resolves each row's source point and centre once into LDS (the index clamped into [0, N),
// never followed), then its threads run along the rows' columns flat - consecutive threads, consecutive addresses, whatever 3 + D
// is, several rows per wave when 3 + D is small.  With one scale table row r is output row r; with more a row's destination - row
// s nsample_i + (j - off_i) of out_i - is resolved with the source into a third LDS table, which the one-scale form does not have.
// When 3 + D is a multiple of 4 and every output is 16-byte aligned a thread writes one float4 (rows then start on 16-byte
// boundaries): the unit that holds the coordinates also holds the attribute beside them; with the coordinates first the attribute
// row is read shifted by three columns against the output (dword loads: it cannot be aligned with both).
// group_points_msg_bwd: a wave per destination point, lanes along the D columns, over the reverse lists (pointset_grad.hip) of the
// concatenated table; msg_row() finds an edge's row of its scale's upstream gradient.
#include "pointset.h"

namespace {

constexpr int GP_THREADS = 256;                                  // every kernel here: four waves
constexpr int BQ_CPW = 8;                                        // centres per wave, one after the other
constexpr int BQ_CENTRES = (GP_THREADS / SVNET_WAVE) * BQ_CPW;   // centres per workgroup
constexpr int GP_MAX_ROWS = 1024;                                // grouping: output rows per workgroup, at most
constexpr int GP_UNITS = 4096;                                   // grouping: floats or float4s per workgroup, about
static_assert(POINTSET_TILE % SVNET_WAVE == 0, "ball_query_kernel takes the tile in whole 64-candidate steps");

// ---- the scales of a call, handed to the kernels by value: no device copy.  off[i] = nsample[0] + .. + nsample[i-1], ktot their
// sum.  msg_scales fills one from the caller's host arrays (r2 may be null where no radius is needed); false unless
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

template <int R>
__global__ __launch_bounds__(GP_THREADS) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int64_t N,
                                                                int64_t S, int64_t chunks, MsgScales sc, int64_t* __restrict__ idx,
                                                                int* __restrict__ count) {
    __shared__ __align__(16) float tile[POINTSET_TILE * 3];
    const int t = threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t b = blockIdx.x / chunks;
    const int64_t s0 = (blockIdx.x % chunks) * BQ_CENTRES + wave * BQ_CPW;            // this wave's first centre
    const int mine = (int)(S - s0 < 0 ? 0 : S - s0 < BQ_CPW ? S - s0 : BQ_CPW);       // its centres: 0 .. BQ_CPW
    const float* pts = xyz + b * N * 3;
    const float* ctr = new_xyz + (b * S + s0) * 3;
    int64_t* rows = idx + (b * S + s0) * sc.ktot;

    int found[BQ_CPW][R], first[BQ_CPW][R];
#pragma unroll
    for (int c = 0; c < BQ_CPW; ++c)
#pragma unroll
        for (int i = 0; i < R; ++i) { found[c][i] = 0; first[c][i] = 0; }
    int pending = mine > 0;
    for (int64_t base = 0; base < N; base += POINTSET_TILE) {
        const int cnt = (int)(N - base < POINTSET_TILE ? N - base : POINTSET_TILE);
        if (base && !__syncthreads_or(pending)) break;           // the previous tile has been read by every wave; all full: done
        stage_xyz<GP_THREADS>(tile, pts + base * 3, cnt, t);
        __syncthreads();
        pending = 0;
#pragma unroll
        for (int c = 0; c < BQ_CPW; ++c) {
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
    for (int c = 0; c < BQ_CPW; ++c) {
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

// U = units per output row: (3 + D) / 4 float4s (VEC) or 3 + D floats; rows_per_block rows per workgroup; R = B * S * ktot rows.
// XYZ_LAST: a row is [attributes | centred xyz], else [centred xyz | attributes].  ONE: one scale, outs.p[0] is [R, 3 + D].
template <bool VEC, bool XYZ_LAST, bool ONE>
__global__ __launch_bounds__(GP_THREADS) void group_points_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                  const float* __restrict__ points, const int64_t* __restrict__ idx,
                                                                  int64_t N, int64_t S, MsgScales sc, int D, int U, int rows_per_block,
                                                                  int64_t R, MsgRows outs) {
    __shared__ int64_t s_src[GP_MAX_ROWS];                       // b * N + the row's point
    __shared__ int s_ctr[GP_MAX_ROWS];                           // b * S + the row's centre
    __shared__ float* s_dst[ONE ? 1 : GP_MAX_ROWS];              // the row of its scale's output (ONE: never touched, takes no LDS)
    const int t = threadIdx.x;
    const int W = 3 + D;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int rows = (int)(R - r0 < rows_per_block ? R - r0 : rows_per_block);
    for (int r = t; r < rows; r += GP_THREADS) {
        const int64_t cs = (r0 + r) / sc.ktot;
        s_src[r] = (cs / S) * N + clamp_index(idx[r0 + r], N);
        s_ctr[r] = (int)cs;
        if (!ONE) {
            const int j = (int)((r0 + r) % sc.ktot);
            float* out = outs.p[0];
            int ns = sc.nsample[0], off = 0;
#pragma unroll
            for (int i = 1; i < SVNET_MSG_MAX_SCALES; ++i)
                if (i < sc.scales && j >= sc.off[i]) { out = outs.p[i]; ns = sc.nsample[i]; off = sc.off[i]; }
            s_dst[r] = out + (cs * ns + (j - off)) * W;
        }
    }
    __syncthreads();
    const int total = rows * U;
    const int qstep = GP_THREADS / U, rstep = GP_THREADS % U;
    int row = t / U, col = t % U;
    for (int e = t; e < total; e += GP_THREADS) {
        const float* p = xyz + s_src[row] * 3;
        const float* q = new_xyz + (int64_t)s_ctr[row] * 3;
        const float* a = points + s_src[row] * D;                // (D = 0: never read)
        float* dst = ONE ? outs.p[0] + (r0 + row) * W : s_dst[row];
        if (VEC) {                                               // 3 + D a multiple of 4, hence D % 4 == 1
            const float* s = a + 4 * col - (XYZ_LAST ? 0 : 3);   // the unit's four columns, were they all attributes
            float4 v;
            if (col == (XYZ_LAST ? U - 1 : 0)) {
                const float d0 = p[0] - q[0], d1 = p[1] - q[1], d2 = p[2] - q[2];
                v = XYZ_LAST ? make_float4(s[0], d0, d1, d2) : make_float4(d0, d1, d2, s[3]);
            } else {
                v = make_float4(s[0], s[1], s[2], s[3]);
            }
            reinterpret_cast<float4*>(dst)[col] = v;
        } else {
            const int x = XYZ_LAST ? col - D : col;              // the coordinate of this column, where it holds one
            dst[col] = (XYZ_LAST ? x >= 0 : x < 3) ? p[x] - q[x] : a[XYZ_LAST ? col : col - 3];
        }
        col += rstep; row += qstep;
        if (col >= U) { col -= U; ++row; }
    }
}

// The gradient of the multi-scale grouping.  (The single-scale form is group_points_bwd_kernel of pointset_grad.hip: one statement of
// both was slower than either - DESIGN.md 4.22 - so each keeps its own.)  The lists are those of the concatenated table,
// E = S * ktot edges per cloud: edge e = s ktot + j lies in the scale i with off[i] <= j < off[i] + nsample[i], and its term is column c - the attributes
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

__global__ __launch_bounds__(GP_THREADS) void group_points_msg_bwd_kernel(MsgRows dg, const int32_t* __restrict__ rev_start,
                                                                           const int32_t* __restrict__ rev_edge, int64_t N, int64_t S,
                                                                           MsgScales sc, int D, int64_t BN, float* __restrict__ dpoints) {
    const int lane = lane_id();
    const int64_t bn = (int64_t)blockIdx.x * (GP_THREADS / SVNET_WAVE) + (threadIdx.x >> 6);
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
inline int gp_rows(int64_t U) {
    const int64_t r = GP_UNITS / U;
    return (int)(r < 1 ? 1 : r > GP_MAX_ROWS ? GP_MAX_ROWS : r);
}

// ---- what the single-scale and the multi-scale entry point of a pair share behind their own argument checks: the limits of the
// launch, reported under the caller's name `who`, and the launch.
int query(const char* who, const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, const MsgScales& sc, int64_t* idx,
          int* count, void* stream) {
    const CloudGrid grid = cloud_grid(B, S, BQ_CENTRES);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "%s: B %lld x ceil(S %lld / %d) workgroups > 2^31 - 1", who, (long long)B, (long long)S,
                  BQ_CENTRES);
    const dim3 blocks((unsigned)grid.blocks), threads(GP_THREADS);
    switch (sc.scales) {
        case 1: hipLaunchKernelGGL(ball_query_kernel<1>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        case 2: hipLaunchKernelGGL(ball_query_kernel<2>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        case 3: hipLaunchKernelGGL(ball_query_kernel<3>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
        default: hipLaunchKernelGGL(ball_query_kernel<4>, blocks, threads, 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks, sc, idx, count); break;
    }
    SVNET_CHECK_LAUNCH("ball_query_kernel");
    return SVNET_OK;
}

template <bool XYZ_LAST, bool ONE, typename... Args>
void launch_group(bool vec, unsigned blocks, void* stream, Args... args) {
    if (vec)
        hipLaunchKernelGGL((group_points_kernel<true, XYZ_LAST, ONE>), dim3(blocks), dim3(GP_THREADS), 0, (hipStream_t)stream, args...);
    else
        hipLaunchKernelGGL((group_points_kernel<false, XYZ_LAST, ONE>), dim3(blocks), dim3(GP_THREADS), 0, (hipStream_t)stream, args...);
}

// (the coordinates come first with one scale only: svnet_group_points_f32)
int group(const char* who, const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N, int64_t S,
          const MsgScales& sc, int64_t D, const MsgRows& outs, bool xyz_last, void* stream) {
    SVNET_REQUIRE(B <= 0x7fffffffll / S / sc.ktot, SVNET_E_UNSUPPORTED, "%s: B %lld x S %lld x nsample %d rows > 2^31 - 1", who, (long long)B,
                  (long long)S, sc.ktot);
    const int64_t R = B * S * sc.ktot, W = 3 + D;
    bool vec = W % 4 == 0;
    for (int i = 0; i < sc.scales; ++i) {
        SVNET_REQUIRE(outs.p[i], SVNET_E_ARG, "%s: null out%d with %d scales", who, i, sc.scales);
        vec = vec && (uintptr_t)outs.p[i] % 16 == 0;
    }
    if (!points) points = xyz;                                   // D = 0: never read
    const int64_t U = vec ? W / 4 : W;
    const int rpb = gp_rows(U);
    const unsigned blocks = (unsigned)svnet_cdiv(R, rpb);
    if (!xyz_last)
        launch_group<false, true>(vec, blocks, stream, xyz, new_xyz, points, idx, N, S, sc, (int)D, (int)U, rpb, R, outs);
    else if (sc.scales == 1)
        launch_group<true, true>(vec, blocks, stream, xyz, new_xyz, points, idx, N, S, sc, (int)D, (int)U, rpb, R, outs);
    else
        launch_group<true, false>(vec, blocks, stream, xyz, new_xyz, points, idx, N, S, sc, (int)D, (int)U, rpb, R, outs);
    SVNET_CHECK_LAUNCH("group_points_kernel");
    return SVNET_OK;
}

// the one scale of a single-scale call
MsgScales one_scale(float r2, int64_t nsample) {
    MsgScales sc{};
    sc.r2[0] = r2;
    sc.nsample[0] = sc.ktot = (int)nsample;
    sc.scales = 1;
    return sc;
}

}  // namespace

extern "C" int svnet_ball_query_tile(void) { return POINTSET_TILE; }

extern "C" int svnet_group_supported(int64_t N, int64_t S, int64_t nsample, int64_t D) {
    return N >= 1 && N <= SVNET_KNN_MAX_N && nsample >= 1 && nsample <= N && S >= 1 && S <= 0x7fffffffll && D >= 0 && D <= 0x7ffffff0ll ? 1 : 0;
}

extern "C" int svnet_group_msg_supported(int64_t N, int64_t S, int64_t scales, const int64_t* nsample, int64_t D) {
    if (!nsample || scales < 1 || scales > SVNET_MSG_MAX_SCALES) return 0;
    for (int64_t i = 0; i < scales; ++i)
        if (!svnet_group_supported(N, S, nsample[i], D)) return 0;
    return 1;
}

extern "C" int svnet_ball_query_f32(const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, float r2, int64_t nsample,
                                    int64_t* idx, int* count, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && count, SVNET_E_ARG, "svnet_ball_query_f32: null xyz / new_xyz / idx / count");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_ball_query_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(svnet_group_supported(N, S, nsample, 0), SVNET_E_UNSUPPORTED,
                  "svnet_ball_query_f32: N %lld, S %lld, nsample %lld: needs 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1",
                  (long long)N, (long long)S, (long long)nsample, (long long)SVNET_KNN_MAX_N);
    return query("svnet_ball_query_f32", xyz, new_xyz, B, N, S, one_scale(r2, nsample), idx, count, stream);
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
    return query("svnet_ball_query_msg_f32", xyz, new_xyz, B, N, S, sc, idx, count, stream);
}

extern "C" int svnet_group_points_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N,
                                      int64_t S, int64_t nsample, int64_t D, float* out, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && out, SVNET_E_ARG, "svnet_group_points_f32: null xyz / new_xyz / idx / out");
    SVNET_REQUIRE(points || D == 0, SVNET_E_ARG, "svnet_group_points_f32: null points with D %lld > 0", (long long)D);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_group_points_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(svnet_group_supported(N, S, nsample, D), SVNET_E_UNSUPPORTED,
                  "svnet_group_points_f32: N %lld, S %lld, nsample %lld, D %lld: needs 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1, D >= 0",
                  (long long)N, (long long)S, (long long)nsample, (long long)D, (long long)SVNET_KNN_MAX_N);
    return group("svnet_group_points_f32", xyz, new_xyz, points, idx, B, N, S, one_scale(0.f, nsample), D, {{out}}, false, stream);
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
    return group("svnet_group_points_msg_f32", xyz, new_xyz, points, idx, B, N, S, sc, D, {{out0, out1, out2, out3}}, true, stream);
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
    const CloudGrid grid = cloud_grid(1, B * N, GP_THREADS / SVNET_WAVE);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_group_points_msg_bwd_f32: B %lld x N %lld / %d workgroups > 2^31 - 1", (long long)B,
                  (long long)N, GP_THREADS / SVNET_WAVE);
    hipLaunchKernelGGL(group_points_msg_bwd_kernel, dim3((unsigned)grid.blocks), dim3(GP_THREADS), 0, (hipStream_t)stream, dg, rev_start, rev_edge,
                       N, S, sc, (int)D, B * N, dpoints);
    SVNET_CHECK_LAUNCH("group_points_msg_bwd_kernel");
    return SVNET_OK;
}
