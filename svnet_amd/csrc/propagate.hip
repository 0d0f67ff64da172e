// Feature propagation from sampled points back to a dense cloud (models/utils/pointnet_util.py:281-308 PointNetFeaturePropagation.forward
// without its MLP): the three nearest sampled points of every query point, inverse-squared-distance weights, and the weighted sum of
// the sampled points' features - what carries [B,num_part,N] logits of an FPS-resampled pool (fps.hip) to the P points it came from.
//
// For one cloud, queries q [P,3], sampled points r [N,3], features f [D,N] (the contract is in svnet_amd/propagate.py's docstring,
// tests/propagate_ref.py restates it independently):
//   d_c = fl(q[p,c] - r[n,c]);  dist[p,n] = sq_len(d_0, d_1, d_2)                    (pointset.h: the distance, single-rounded)
//   (dist3_j, i_j), j = 0..2: the min(3, N) smallest dist[p,:], ascending, the lower index first among equals; a slot that no
//                             candidate took (N < 3; NaN and +inf distances) holds (+inf, 0)
//   rec_j = fl(1 / fl(dist3_j + fp32(1e-8)));  s = fl(fl(rec_0 + rec_1) + rec_2);  w_j = fl(rec_j / s)
//   out[d,p] = fl(fl(fl(f[d,i_0] w_0) + fl(f[d,i_1] w_1)) + fl(f[d,i_2] w_2))
// Every product, sum and quotient is its own correctly rounded fp32 operation (pointset.h).
//
// three_nn: one thread per query point, 256 per workgroup, the workgroups of a cloud side by side.  The cloud's sampled points pass
// through LDS in tiles of POINTSET_TILE points (pointset.h: stage_xyz, padded with NaN to whole groups of four); in the candidate
// loop every lane reads the SAME address - three ds_read_b128 broadcasts per four candidates and wave, no bank conflict - and the
// thread keeps its three best (distance, index) pairs in registers.  Candidates arrive in ascending index order and are inserted
// on a strict <, so among equal distances the lower index stays in front: the tie rule costs nothing.  A NaN distance compares
// false and is never inserted; the slots start at (+inf, 0), so every index written is inside [0, N) whatever the coordinates hold.
// three_interpolate: one thread per query point again, looping over the D channels: three gathers inside one 4 N-byte row per
// channel (L2-resident), one store per channel, coalesced along p.  An index outside [0, N) is clamped into it: nothing is read
// out of bounds whatever the caller hands in.
#include "pointset.h"

namespace {

constexpr int PROP_THREADS = 256;
constexpr float PROP_EPS = 1e-8f;                // pointnet_util.py:305
static_assert(POINTSET_TILE % 4 == 0, "three_nn_kernel reads the tile in groups of four points");

struct Best3 { float b0, b1, b2; int i0, i1, i2; };

// the candidate at offset (d0, d1, d2) with index g against the three best: a strict < at every level, so an equal distance stays behind
__device__ __forceinline__ void offer(Best3& s, float d0, float d1, float d2, int g) {
    const float dist = sq_len(d0, d1, d2);
    if (dist < s.b2) {
        if (dist < s.b1) {
            s.b2 = s.b1; s.i2 = s.i1;
            if (dist < s.b0) { s.b1 = s.b0; s.i1 = s.i0; s.b0 = dist; s.i0 = g; }
            else { s.b1 = dist; s.i1 = g; }
        } else {
            s.b2 = dist; s.i2 = g;
        }
    }
}

__global__ __launch_bounds__(PROP_THREADS) void three_nn_kernel(const float* __restrict__ query, const float* __restrict__ ref, int64_t P,
                                                                int64_t N, int64_t chunks, int64_t* __restrict__ idx,
                                                                float* __restrict__ dist3, float* __restrict__ weight) {
    __shared__ __align__(16) float tile[POINTSET_TILE * 3];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x / chunks;
    const int64_t p = (blockIdx.x % chunks) * PROP_THREADS + t;
    const bool real = p < P;
    const float* q = query + (b * P + (real ? p : 0)) * 3;
    const float* r = ref + b * N * 3;
    const float qx = q[0], qy = q[1], qz = q[2];

    Best3 best = {SVNET_INF, SVNET_INF, SVNET_INF, 0, 0, 0};
    for (int64_t base = 0; base < N; base += POINTSET_TILE) {
        const int cnt = (int)(N - base < POINTSET_TILE ? N - base : POINTSET_TILE);
        const int groups = (cnt + 3) >> 2;                       // four points = 48 B = three 16-byte reads
        if (base) __syncthreads();                               // the previous tile has been read by every wave
        stage_xyz<PROP_THREADS, 4>(tile, r + base * 3, cnt, t);  // (NaN padding to whole groups: never taken)
        __syncthreads();
        const float4* v = reinterpret_cast<const float4*>(tile);
        const int g0 = (int)base;
#pragma unroll 2
        for (int g = 0; g < groups; ++g) {
            const float4 a = v[3 * g], c = v[3 * g + 1], e = v[3 * g + 2];
            const int n = g0 + 4 * g;
            offer(best, qx - a.x, qy - a.y, qz - a.z, n);
            offer(best, qx - a.w, qy - c.x, qz - c.y, n + 1);
            offer(best, qx - c.z, qy - c.w, qz - e.x, n + 2);
            offer(best, qx - e.y, qy - e.z, qz - e.w, n + 3);
        }
    }
    if (!real) return;
    const float b0 = best.b0, b1 = best.b1, b2 = best.b2;
    const float r0 = 1.f / (b0 + PROP_EPS), r1 = 1.f / (b1 + PROP_EPS), r2 = 1.f / (b2 + PROP_EPS);
    const float s = (r0 + r1) + r2;
    const int64_t o = (b * P + p) * 3;
    idx[o + 0] = best.i0; idx[o + 1] = best.i1; idx[o + 2] = best.i2;
    dist3[o + 0] = b0; dist3[o + 1] = b1; dist3[o + 2] = b2;
    weight[o + 0] = r0 / s; weight[o + 1] = r1 / s; weight[o + 2] = r2 / s;
}

__global__ __launch_bounds__(PROP_THREADS) void three_interpolate_kernel(const float* __restrict__ feat, const int64_t* __restrict__ idx,
                                                                         const float* __restrict__ weight, int64_t D, int64_t N, int64_t P,
                                                                         int64_t chunks, float* __restrict__ out) {
    const int64_t b = blockIdx.x / chunks;
    const int64_t p = (blockIdx.x % chunks) * PROP_THREADS + threadIdx.x;
    if (p >= P) return;
    const int64_t o = (b * P + p) * 3;
    const int64_t i0 = clamp_index(idx[o + 0], N), i1 = clamp_index(idx[o + 1], N), i2 = clamp_index(idx[o + 2], N);
    const float w0 = weight[o + 0], w1 = weight[o + 1], w2 = weight[o + 2];
    const float* row = feat + b * D * N;
    float* dst = out + b * D * P + p;
#pragma unroll 4
    for (int64_t d = 0; d < D; ++d) {
        dst[d * P] = (row[i0] * w0 + row[i1] * w1) + row[i2] * w2;
        row += N;
    }
}

}  // namespace

extern "C" int svnet_propagate_tile(void) { return POINTSET_TILE; }

extern "C" int svnet_propagate_supported(int64_t P, int64_t N, int64_t D) {
    return P >= 1 && D >= 1 && N >= 1 && N <= SVNET_KNN_MAX_N && svnet_cdiv(P, PROP_THREADS) <= 0x7fffffffll ? 1 : 0;
}

extern "C" int svnet_three_nn_f32(const float* query, const float* ref, int64_t B, int64_t P, int64_t N, int64_t* idx, float* dist3,
                                  float* weight, void* stream) {
    SVNET_REQUIRE(query && ref && idx && dist3 && weight, SVNET_E_ARG, "svnet_three_nn_f32: null query / ref / idx / dist3 / weight");
    SVNET_REQUIRE(B >= 1 && P >= 1 && N >= 1, SVNET_E_ARG, "svnet_three_nn_f32: B %lld, P %lld, N %lld must be positive", (long long)B,
                  (long long)P, (long long)N);
    SVNET_REQUIRE(svnet_propagate_supported(P, N, 1), SVNET_E_UNSUPPORTED,
                  "svnet_three_nn_f32: N %lld > %lld (the k-NN's limit on the points of a cloud) or P %lld past a 32-bit grid", (long long)N,
                  (long long)SVNET_KNN_MAX_N, (long long)P);
    const CloudGrid grid = cloud_grid(B, P, PROP_THREADS);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_three_nn_f32: B %lld x ceil(P %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)P, PROP_THREADS);
    hipLaunchKernelGGL(three_nn_kernel, dim3((unsigned)grid.blocks), dim3(PROP_THREADS), 0, (hipStream_t)stream, query, ref, P, N,
                       grid.chunks, idx, dist3, weight);
    SVNET_CHECK_LAUNCH("three_nn_kernel");
    return SVNET_OK;
}

extern "C" int svnet_three_interpolate_f32(const float* feat, const int64_t* idx, const float* weight, int64_t B, int64_t D, int64_t N,
                                           int64_t P, float* out, void* stream) {
    SVNET_REQUIRE(feat && idx && weight && out, SVNET_E_ARG, "svnet_three_interpolate_f32: null feat / idx / weight / out");
    SVNET_REQUIRE(B >= 1 && D >= 1 && N >= 1 && P >= 1, SVNET_E_ARG, "svnet_three_interpolate_f32: B %lld, D %lld, N %lld, P %lld must be positive",
                  (long long)B, (long long)D, (long long)N, (long long)P);
    SVNET_REQUIRE(svnet_propagate_supported(P, N, D), SVNET_E_UNSUPPORTED,
                  "svnet_three_interpolate_f32: N %lld > %lld (the k-NN's limit on the points of a cloud) or P %lld past a 32-bit grid",
                  (long long)N, (long long)SVNET_KNN_MAX_N, (long long)P);
    const CloudGrid grid = cloud_grid(B, P, PROP_THREADS);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_three_interpolate_f32: B %lld x ceil(P %lld / %d) workgroups > 2^31 - 1",
                  (long long)B, (long long)P, PROP_THREADS);
    hipLaunchKernelGGL(three_interpolate_kernel, dim3((unsigned)grid.blocks), dim3(PROP_THREADS), 0, (hipStream_t)stream, feat, idx, weight, D,
                       N, P, grid.chunks, out);
    SVNET_CHECK_LAUNCH("three_interpolate_kernel");
    return SVNET_OK;
}
