// What the point-set helpers of models/utils/pointnet_util.py share on the device: farthest point sampling (fps.hip), the
// three-nearest-neighbour propagation (propagate.hip), ball query and grouping (group.hip).  Stated here once; the three files and
// the Python front ends (svnet_amd/_pointset.py) refer to it.  Internal: not part of the C interface (include/svnet_hip.h).
//
// Every file that includes this header is compiled with -ffp-contract=off (Makefile, NO_CONTRACT): each product, sum and difference
// is its own correctly rounded fp32 operation, so the host can restate the results bit for bit (tests/pointset_ref.py).
// The limit on the points of a cloud that propagate.hip and group.hip take is the k-NN's, SVNET_KNN_MAX_N (common.h).
#pragma once
#include "common.h"

// ---- the distance.  For the coordinate differences d_c = fl(a_c - b_c) of two points:
//   dist = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))
// five single-rounded operations in exactly this association order: every bit-for-bit claim of the three helpers (against each
// other, against the numpy restatements and against the reference's recorded results) rests on this one line.  It is the
// DIFFERENCE form: never negative, exactly 0 at a coincident point.  The reference's expanded form -2 a.b + |a|^2 + |b|^2 is
// deliberately not used: sampled points and centres coincide with points of the cloud, there the expanded form rounds to small
// values of either sign, and 1 / (dist + 1e-8) or a radius test turns that into garbage.  (On coordinates whose squares and products
// are exact in fp32 the two forms agree bit for bit.)  The function takes the differences, not the points: the callers subtract in
// their own direction, which the square does not see.
__device__ __forceinline__ float sq_len(float d0, float d1, float d2) { return (d0 * d0 + d1 * d1) + d2 * d2; }

// An index clamped into [0, N): what a kernel follows when the caller handed the index in.
__device__ __forceinline__ int64_t clamp_index(int64_t i, int64_t N) { return i < 0 ? 0 : i >= N ? N - 1 : i; }

// The quiet NaN a row read through an index outside the cloud holds, and +inf: bit patterns 0x7fc00000 and 0x7f800000.
constexpr float SVNET_QNAN = __builtin_nanf("");
constexpr float SVNET_INF = __builtin_inff();

// ---- the LDS tile of packed xyz.  The candidate loops of three_nn and ball_query pass a cloud's points through LDS in tiles of
// POINTSET_TILE points, packed as they lie in memory (12 B each, 24 KiB: no opt-in, six workgroups per CU).  stage_xyz is the refill
// by the T threads of a workgroup: `cnt` points from src, then NaN (a NaN distance compares false: never taken) up to the next
// multiple of PAD points.  The barriers on both sides of it belong to the caller.
constexpr int POINTSET_TILE = 2048;

template <int T, int PAD = 1>
__device__ __forceinline__ void stage_xyz(float* tile, const float* __restrict__ src, int cnt, int t) {
    const int fill = (int)((unsigned)(cnt + PAD - 1) / PAD) * (3 * PAD);
    for (int n = t; n < fill; n += T) tile[n] = PAD == 1 || n < cnt * 3 ? src[n] : SVNET_QNAN;
}

// ---- the launch geometry.  B clouds x ceil(items / per) workgroups side by side, cloud-major: a kernel takes its cloud as
// blockIdx.x / chunks and its share of the cloud's items from blockIdx.x % chunks.  blocks = 0 when they do not fit a 32-bit grid.
struct CloudGrid { int64_t chunks, blocks; };
static inline CloudGrid cloud_grid(int64_t B, int64_t items, int per) {
    const int64_t chunks = svnet_cdiv(items, per);
    return {chunks, B <= 0x7fffffffll / chunks ? B * chunks : 0};
}
