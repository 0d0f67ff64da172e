// The reduction over a long axis, split over workgroups: x viewed as [outer, R, inner], `chunks` row chunks per outer index on a grid
// (chunks, outer), each workgroup leaving per column a packed arg-max key (atomicMax) and / or an ordered partial sum, and a small
// second kernel that unpacks the keys and adds the chunks' sums in chunk order (no float atomics: bit-reproducible, which matters
// because the means feed sign() one layer later).  Stated here once: how the rows are cut (split_plan), when the path may be taken
// (split_eligible), what the workspace holds (split_workspace_bytes / split_workspace_carve), the finish (split_maxmean_finish,
// ordered_chunk_sum) and the row walk of the streaming kernels (row_ladder, split_fwd_columns).  pool.hip and vtail.hip refer to it;
// the key itself is pack_key / unpack_key (wave.h).  Internal: not part of the C interface (include/svnet_hip.h).
#pragma once
#include "common.h"

// ---- the plan: about `target` workgroups in all (chunks x outer), no chunk planned shorter than `least_rows` rows, rows per chunk a
// multiple of `row_multiple`; then as few chunks as cover R with those rows.  chunks >= 1, chunks * rows >= R.  outer > 0 and R > 0
// (every entry point checks them, or returns, before it plans).  The forward split kernels and svnet_pool_workspace_bytes share
// SPLIT_FWD_*: 8 workgroups per CU, 32 rows; every other caller states its parameters, and the reason for them, where it plans.
struct SplitPlan { int64_t chunks, rows; };
static inline SplitPlan split_plan(int64_t outer, int64_t R, int64_t target, int64_t least_rows, int64_t row_multiple = 1) {
    int64_t chunks = svnet_cdiv(target, outer);
    if (chunks > svnet_cdiv(R, least_rows)) chunks = svnet_cdiv(R, least_rows);
    if (chunks < 1) chunks = 1;
    const int64_t rows = svnet_cdiv(svnet_cdiv(R, chunks), row_multiple) * row_multiple;
    return {svnet_cdiv(R, rows), rows};
}
constexpr int64_t SPLIT_FWD_TARGET = 256 * 8, SPLIT_FWD_LEAST_ROWS = 32;

// ---- when the forward split path may be taken: a long axis, few outputs (the finish kernels divide in 32 bits), outer as grid.y
constexpr int64_t SPLIT_MIN_ROWS = 256;
static inline bool split_eligible(int64_t outer, int64_t R, int64_t inner) {
    return R >= SPLIT_MIN_ROWS && outer * inner < (1 << 20) && outer > 0 && outer <= 65535;
}

// ---- the workspace of `total` = outer * inner outputs: [arg-max keys: total x u64 | partial sums: chunks x total x f32], either
// part optional.  The keys start at 0 (below every packed key): the launcher's memset, or a caller's zero-filled block.
struct SplitWorkspace { unsigned long long* keys; float* part; };
static inline size_t split_workspace_bytes(int64_t total, int64_t chunks, bool keys, bool sums) {
    return (keys ? (size_t)total * 8 : 0) + (sums ? (size_t)(chunks * total) * sizeof(float) : 0);
}
static inline SplitWorkspace split_workspace_carve(void* workspace, int64_t total, bool keys, bool sums) {
    char* p = (char*)workspace;
    return {keys ? (unsigned long long*)p : nullptr, sums ? (float*)(p + split_workspace_bytes(total, 0, keys, false)) : nullptr};
}

// ---- the finish of a [max | mean] pass (pool.hip): values and arg-max out of the keys, mean = (the chunks' sums in order) / R, into
// rows of stride out_ld.  total < 2^20.
int split_maxmean_finish(const unsigned long long* keys, const float* part, int64_t chunks, int64_t total, int64_t R, float* out_max,
                         float* out_mean, int32_t* argmax, int64_t inner, int64_t out_ld, hipStream_t stream);

#ifdef __HIPCC__
// the chunks' partial sums of output e in chunk order - bit-reproducible - with eight loads in flight: one dependent L2 round trip per
// chunk made the 16 K-element finish 8 - 10 us long
__device__ __forceinline__ float ordered_chunk_sum(const float* __restrict__ part, int64_t chunks, int64_t total, int64_t e) {
    float s = 0.f;
    int64_t c = 0;
    for (; c + 7 < chunks; c += 8) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = part[(c + u) * total + e];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += t[u];
    }
    for (; c < chunks; ++c) s += part[c * total + e];
    return s;
}

// ---- the row walk of a thread that streams rows [r, r1) of its column: U rows requested (t = req(row)) before the first is used
// (use(row, t)), as long as U rows are left; a ladder of depths U... ends in 1.
template <int U, typename Req, typename Use>
__device__ __forceinline__ void walk_rows(int64_t& r, int64_t r1, const Req& req, const Use& use) {
    for (; r + (U - 1) < r1; r += U) {
        float t[U];
#pragma unroll
        for (int u = 0; u < U; ++u) t[u] = req(r + u);
#pragma unroll
        for (int u = 0; u < U; ++u) use(r + u, t[u]);
    }
}
template <int... U, typename Req, typename Use>
__device__ __forceinline__ void row_ladder(int64_t r, int64_t r1, const Req& req, const Use& use) {
    (walk_rows<U>(r, r1, req, use), ...);
}

// ---- the body of the forward split kernels, grid (chunks, outer), threads over columns: per column the running maximum of
// f(x) with its first row (MAX: a packed key, atomicMax into keys) and / or the sum of f(x) (MEAN: part[chunk][outer * inner]).
// `map.column(i)` is f for column i: the identity, or BatchNorm + activation with the column's four constants loaded once.
// DEEP: the 16 / 8 / 1 ladder instead of 8 / 1.  The max forms start from the first row (best = s = f(x[r0]), next row r0 + 1),
// the mean-only form from s = 0 at row r0: the order of the additions is part of the result.  The comparison is a bare '>' (the
// first row keeps a tie), so these kernels do NOT propagate NaN, unlike pool_fwd_kernel, which does as torch does.
struct MapIdentity {
    __device__ __forceinline__ auto column(int64_t) const { return [](float v) { return v; }; }
};
struct MapBnAct {       // (the same arithmetic, in the same order, as bn_act_fwd_kernel: the pooled values equal pooling its output)
    const float *mean, *invstd, *gamma, *beta;
    int act;
    float slope;
    __device__ __forceinline__ auto column(int64_t i) const {
        const float mu = mean[i], is = invstd[i], ga = gamma[i], be = beta[i];
        const int a = act;
        const float sl = slope;
        return [=](float v) { return act_apply((v - mu) * is * ga + be, a, sl); };
    }
};
template <bool MAX, bool MEAN, bool DEEP, typename Map>
__device__ __forceinline__ void split_fwd_columns(const float* __restrict__ x, int64_t R, int64_t inner, int64_t rows_per_chunk,
                                                  unsigned long long* __restrict__ keys, float* __restrict__ part, int64_t total,
                                                  const Map& map) {
    const int64_t o = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
    for (int64_t i = threadIdx.x; i < inner; i += blockDim.x) {
        const auto f = map.column(i);
        const float* p = x + o * R * inner + i;
        float best = MAX ? f(p[r0 * inner]) : 0.f, s = best;
        int64_t bi = r0;
        const auto req = [&](int64_t r) { return p[r * inner]; };
        const auto use = [&](int64_t r, float t) {
            const float z = f(t);
            if (MEAN) s += z;
            if (MAX && z > best) { best = z; bi = r; }
        };
        if (DEEP) row_ladder<16, 8, 1>(MAX ? r0 + 1 : r0, r1, req, use);
        else row_ladder<8, 1>(MAX ? r0 + 1 : r0, r1, req, use);
        if (MAX) atomicMax(&keys[o * inner + i], pack_key(best, bi));
        if (MEAN) part[(int64_t)blockIdx.x * total + o * inner + i] = s;
    }
}
#endif
