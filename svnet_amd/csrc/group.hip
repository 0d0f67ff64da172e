// Ball query and neighbourhood grouping (models/utils/pointnet_util.py:87-107 query_ball_point, 110-143 sample_and_group without its
// sampling): the step that turns sampled centres into fixed-size local neighbourhoods - the third point-set helper of that file beside
// farthest point sampling (fps.hip) and the three-nearest-neighbour interpolation (propagate.hip).
//
// For one cloud, points xyz [N,3], centres new_xyz [S,3], optional attributes points [N,D] (channel-last); the contract is in
// svnet_amd/group.py's docstring, tests/group_ref.py restates it independently:
//   d_c = fl(new_xyz[s,c] - xyz[n,c]);  dist[s,n] = sq_len(d_0, d_1, d_2)            (pointset.h: the distance, single-rounded)
//   inside(s,n) = dist[s,n] <= r2                     (a NaN distance compares false: never inside)
//   idx[s,0..nsample-1] = the first nsample inside points in ascending point index, slots past the number found = the first inside
//                         index; count[s] = min(found, nsample); an empty group: count 0, every slot 0
//   out[s,j,0..2] = fl(xyz[idx[s,j],c] - new_xyz[s,c]);  out[s,j,3..] = points[idx[s,j],:] copied bit for bit
// Every product, sum and difference is its own correctly rounded fp32 operation (pointset.h).
//
// ball_query: one wave per centre at a time, BQ_CPW centres after each other per wave, four waves (32 centres) per workgroup, the
// workgroups of a cloud side by side.  The cloud's points pass through LDS in tiles of POINTSET_TILE points (pointset.h: stage_xyz,
// no padding), shared by the workgroup's 32 centres; lane l of a wave reads point n0 + l, a stride of three dwords across the
// lanes (odd: no bank conflict).  A step takes 64 candidates in index order: the ballot
// of `inside` is the step's membership mask, a lane's slot is found + (set lanes below it) (lanes_below, wave.h), so the row is
// written in order and coalesced, and `found` grows by the mask's population.  The wave leaves a centre's loop as soon as
// found >= nsample - uniform per wave, no divergence - which is the point of the kernel: at PointNet++ radii most groups fill after
// a fraction of N.  `found` and the first inside index of every centre are wave-uniform registers that survive the tile loop; a
// workgroup whose centres are all full skips the remaining tiles (the vote rides on the barrier the tile swap needs anyway).
// One padding pass per centre fills the slots past `found`.  Every index written is a candidate's own or 0: inside [0, N), always.
// group_points: a row gather.  A workgroup takes GP_ROWS(U) consecutive output rows (one row = one (centre, slot) pair), resolves
// each row's source point and centre once into LDS (the index clamped into [0, N), never followed), then its threads run along the
// rows' columns flat - consecutive threads, consecutive addresses, whatever 3 + D is, several rows per wave when 3 + D is small.
// When 3 + D is a multiple of 4 and `out` is 16-byte aligned a thread writes one float4 (rows then start on 16-byte boundaries; the
// attribute row is read with dword loads, shifted by three columns against the output it cannot be aligned with both).
#include "pointset.h"

namespace {

constexpr int BQ_THREADS = 256;
constexpr int BQ_CPW = 8;                                        // centres per wave, one after the other
constexpr int BQ_CENTRES = (BQ_THREADS / SVNET_WAVE) * BQ_CPW;   // centres per workgroup
constexpr int GP_THREADS = 256;
constexpr int GP_MAX_ROWS = 1024;                                // output rows per workgroup, at most
constexpr int GP_UNITS = 4096;                                   // floats or float4s per workgroup, about
static_assert(POINTSET_TILE % SVNET_WAVE == 0, "ball_query_kernel takes the tile in whole 64-candidate steps");

__global__ __launch_bounds__(BQ_THREADS) void ball_query_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz, int64_t N,
                                                                int64_t S, int64_t chunks, float r2, int nsample,
                                                                int64_t* __restrict__ idx, int* __restrict__ count) {
    __shared__ __align__(16) float tile[POINTSET_TILE * 3];
    const int t = threadIdx.x, lane = lane_id(), wave = t >> 6;
    const int64_t b = blockIdx.x / chunks;
    const int64_t s0 = (blockIdx.x % chunks) * BQ_CENTRES + wave * BQ_CPW;            // this wave's first centre
    const int mine = (int)(S - s0 < 0 ? 0 : S - s0 < BQ_CPW ? S - s0 : BQ_CPW);       // its centres: 0 .. BQ_CPW
    const float* pts = xyz + b * N * 3;
    const float* ctr = new_xyz + (b * S + s0) * 3;
    int64_t* rows = idx + (b * S + s0) * nsample;

    int found[BQ_CPW], first[BQ_CPW];
#pragma unroll
    for (int c = 0; c < BQ_CPW; ++c) { found[c] = 0; first[c] = 0; }
    int pending = mine > 0;
    for (int64_t base = 0; base < N; base += POINTSET_TILE) {
        const int cnt = (int)(N - base < POINTSET_TILE ? N - base : POINTSET_TILE);
        if (base && !__syncthreads_or(pending)) break;           // the previous tile has been read by every wave; all full: done
        stage_xyz<BQ_THREADS>(tile, pts + base * 3, cnt, t);
        __syncthreads();
        pending = 0;
#pragma unroll
        for (int c = 0; c < BQ_CPW; ++c) {
            if (c >= mine || found[c] >= nsample) continue;      // wave-uniform
            const float qx = ctr[3 * c], qy = ctr[3 * c + 1], qz = ctr[3 * c + 2];
            int64_t* row = rows + (int64_t)c * nsample;
            int f = found[c], g = first[c];
            for (int n0 = 0; n0 < cnt; n0 += SVNET_WAVE) {
                const int n = n0 + lane;
                bool inside = false;
                if (n < cnt) {
                    const float d0 = qx - tile[3 * n], d1 = qy - tile[3 * n + 1], d2 = qz - tile[3 * n + 2];
                    inside = sq_len(d0, d1, d2) <= r2;
                }
                const unsigned long long mask = __ballot(inside);
                if (mask) {
                    if (f == 0) g = (int)base + n0 + (int)__builtin_ctzll(mask);
                    const int slot = f + lanes_below(mask);
                    if (inside && slot < nsample) row[slot] = (int64_t)((int)base + n);
                    f += (int)__popcll(mask);
                    if (f >= nsample) break;
                }
            }
            found[c] = f; first[c] = g;
            pending |= f < nsample;
        }
    }
#pragma unroll
    for (int c = 0; c < BQ_CPW; ++c) {
        if (c >= mine) continue;
        const int f = found[c] < nsample ? found[c] : nsample;
        int64_t* row = rows + (int64_t)c * nsample;
        for (int j = f + lane; j < nsample; j += SVNET_WAVE) row[j] = first[c];      // first[c] = 0 when nothing was found
        if (lane == 0) count[b * S + s0 + c] = f;
    }
}

// U = units per output row: (3 + D) / 4 float4s (VEC) or 3 + D floats; rows_per_block rows per workgroup; R = B * S * nsample rows.
template <bool VEC>
__global__ __launch_bounds__(GP_THREADS) void group_points_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                  const float* __restrict__ points, const int64_t* __restrict__ idx,
                                                                  int64_t N, int64_t S, int nsample, int D, int U, int rows_per_block,
                                                                  int64_t R, float* __restrict__ out) {
    __shared__ int64_t s_src[GP_MAX_ROWS];      // b * N + the row's point
    __shared__ int s_ctr[GP_MAX_ROWS];          // b * S + the row's centre
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int rows = (int)(R - r0 < rows_per_block ? R - r0 : rows_per_block);
    for (int r = t; r < rows; r += GP_THREADS) {
        const int64_t cs = (r0 + r) / nsample;
        s_src[r] = (cs / S) * N + clamp_index(idx[r0 + r], N);
        s_ctr[r] = (int)cs;
    }
    __syncthreads();
    const int W = 3 + D, total = rows * U;
    const int qstep = GP_THREADS / U, rstep = GP_THREADS % U;
    int row = t / U, col = t % U;
    for (int e = t; e < total; e += GP_THREADS) {
        const float* p = xyz + s_src[row] * 3;
        const float* q = new_xyz + (int64_t)s_ctr[row] * 3;
        const float* a = points + s_src[row] * D;                // (D = 0: never read)
        float* dst = out + (r0 + row) * W;
        if (VEC) {
            float4 v;
            if (col == 0) {
                v.x = p[0] - q[0]; v.y = p[1] - q[1]; v.z = p[2] - q[2]; v.w = a[0];
            } else {
                const float* s = a + 4 * col - 3;
                v.x = s[0]; v.y = s[1]; v.z = s[2]; v.w = s[3];
            }
            reinterpret_cast<float4*>(dst)[col] = v;
        } else {
            dst[col] = col < 3 ? p[col] - q[col] : a[col - 3];
        }
        col += rstep; row += qstep;
        if (col >= U) { col -= U; ++row; }
    }
}

// output rows per workgroup of the grouping for U units per row
inline int gp_rows(int64_t U) {
    const int64_t r = GP_UNITS / U;
    return (int)(r < 1 ? 1 : r > GP_MAX_ROWS ? GP_MAX_ROWS : r);
}

}  // namespace

extern "C" int svnet_ball_query_tile(void) { return POINTSET_TILE; }

extern "C" int svnet_group_supported(int64_t N, int64_t S, int64_t nsample, int64_t D) {
    return N >= 1 && N <= SVNET_KNN_MAX_N && nsample >= 1 && nsample <= N && S >= 1 && S <= 0x7fffffffll && D >= 0 && D <= 0x7ffffff0ll ? 1 : 0;
}

extern "C" int svnet_ball_query_f32(const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, float r2, int64_t nsample,
                                    int64_t* idx, int* count, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && count, SVNET_E_ARG, "svnet_ball_query_f32: null xyz / new_xyz / idx / count");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_ball_query_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(svnet_group_supported(N, S, nsample, 0), SVNET_E_UNSUPPORTED,
                  "svnet_ball_query_f32: N %lld, S %lld, nsample %lld: needs 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1",
                  (long long)N, (long long)S, (long long)nsample, (long long)SVNET_KNN_MAX_N);
    const CloudGrid grid = cloud_grid(B, S, BQ_CENTRES);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_ball_query_f32: B %lld x ceil(S %lld / %d) workgroups > 2^31 - 1",
                  (long long)B, (long long)S, BQ_CENTRES);
    hipLaunchKernelGGL(ball_query_kernel, dim3((unsigned)grid.blocks), dim3(BQ_THREADS), 0, (hipStream_t)stream, xyz, new_xyz, N, S, grid.chunks,
                       r2, (int)nsample, idx, count);
    SVNET_CHECK_LAUNCH("ball_query_kernel");
    return SVNET_OK;
}

extern "C" int svnet_group_points_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N,
                                      int64_t S, int64_t nsample, int64_t D, float* out, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && out, SVNET_E_ARG, "svnet_group_points_f32: null xyz / new_xyz / idx / out");
    SVNET_REQUIRE(points || D == 0, SVNET_E_ARG, "svnet_group_points_f32: null points with D %lld > 0", (long long)D);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_group_points_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(svnet_group_supported(N, S, nsample, D), SVNET_E_UNSUPPORTED,
                  "svnet_group_points_f32: N %lld, S %lld, nsample %lld, D %lld: needs 1 <= nsample <= N <= %lld (the k-NN's limit on the points of a cloud), S >= 1, D >= 0",
                  (long long)N, (long long)S, (long long)nsample, (long long)D, (long long)SVNET_KNN_MAX_N);
    SVNET_REQUIRE(B <= 0x7fffffffll / S / nsample, SVNET_E_UNSUPPORTED, "svnet_group_points_f32: B %lld x S %lld x nsample %lld rows > 2^31 - 1",
                  (long long)B, (long long)S, (long long)nsample);
    const int64_t R = B * S * nsample, W = 3 + D;
    if (!points) points = xyz;                                   // D = 0: never read
    const bool vec = W % 4 == 0 && (uintptr_t)out % 16 == 0;
    const int64_t U = vec ? W / 4 : W;
    const int rpb = gp_rows(U);
    const unsigned blocks = (unsigned)svnet_cdiv(R, rpb);
    if (vec)
        hipLaunchKernelGGL(group_points_kernel<true>, dim3(blocks), dim3(GP_THREADS), 0, (hipStream_t)stream, xyz, new_xyz, points, idx, N, S,
                           (int)nsample, (int)D, (int)U, rpb, R, out);
    else
        hipLaunchKernelGGL(group_points_kernel<false>, dim3(blocks), dim3(GP_THREADS), 0, (hipStream_t)stream, xyz, new_xyz, points, idx, N, S,
                           (int)nsample, (int)D, (int)U, rpb, R, out);
    SVNET_CHECK_LAUNCH("group_points_kernel");
    return SVNET_OK;
}
