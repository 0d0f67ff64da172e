// Gradients of the two point-set operations that carry activations: three_interpolate (propagate.hip) with respect to feat, and
// group_points (group.hip) with respect to points.  Both backwards are scatters: here each is a reverse list per destination plus a
// per-destination sum in a fixed order - no float atomic anywhere, so two runs give the same bits (the store pass plus
// per-destination sum pass form; the "store pass" is the upstream gradient itself, which already holds one row per edge).
//
// For one cloud and a rectangular index table idx [R,K] int64 with targets in [0, N):
//   edge e = r K + j points to n(e) = clamp_index(idx[r,j], N)              (pointset.h: the clamp the forward kernels follow, so the
//                                                                            backward is the adjoint of what the forward computed)
//   list n = rev_edge[rev_start[n] .. rev_start[n+1]) holds every edge with n(e) = n exactly once, in ASCENDING e; nothing is skipped
//   three_interpolate backward (R = P, K = 3): with the list's edges e_1 < e_2 < ..., e_i = 3 p_i + j_i and
//       t_i = fl(dout[d,p_i] weight[p_i,j_i]):   dfeat[d,n] = fl(fl(fl(t_1 + t_2) + t_3) + ...), one term gives t_1, no term gives +0
//   group_points backward (R = S, K = nsample): t_i = dgrouped[s_i,j_i,3+c]:  dpoints[n,c] by the same sum
// Every product and sum is its own correctly rounded fp32 operation (pointset.h); tests/pointset_grad_ref.py restates the contract.
//
// reverse: a stable counting sort without atomics and without workspace.  A workgroup of four waves owns REV_TILE = 256 consecutive
// destinations of one cloud, a wave 64 of them, a lane one.  The cloud's edges pass through LDS in chunks of REV_CHUNK, clamped and
// narrowed to int32 once per workgroup; every wave reads a chunk 64 edges at a time in edge order, and the ballot of "this edge
// points into my 64 destinations" is walked from the lowest lane up: the lane that owns the target appends.  The walk IS the edge
// order, so the lists come out ascending by construction.  Two passes over the edges: the first counts (per lane, and the edges
// that point below the wave's destinations, which is where its first list starts), the second fills.  The price is that every
// workgroup reads the whole table: ceil(N / 256) reads of it per cloud, from L2.
// group backward: a wave per destination point, lanes along the D columns; a list's rows are contiguous, 4 (3 + D) bytes each.
// interpolate backward: a thread per destination point, consecutive lanes consecutive n, ITP_DCH channels per thread in registers so
// that a list's edges and weights are read once per ITP_DCH channels.  dout is channel-first: lanes along n keep the stores of
// dfeat coalesced, and a wave's gathers of dout[d,p] stay inside one 4 P-byte row per channel (cache-resident, every element read
// three times in all); lanes along d would touch 64 cache lines per load for 4 bytes each.
#include "pointset.h"

namespace {

constexpr int REV_THREADS = 256;
constexpr int REV_TILE = REV_THREADS;                 // destinations per workgroup: one per thread, 64 per wave
constexpr int REV_CHUNK = 2048;                       // edges per LDS chunk
constexpr int REV_NONE = 0x7fffffff;                  // the target of a slot past the last edge: below nothing, inside nothing
constexpr int GPB_THREADS = 256;                      // group backward: four destinations per workgroup
constexpr int ITP_THREADS = 256;
constexpr int ITP_DCH = 8;                            // channels per thread of the interpolate backward
static_assert(REV_CHUNK % REV_THREADS == 0 && REV_CHUNK % SVNET_WAVE == 0, "the chunk is staged and read in whole steps");

__device__ __forceinline__ int wave_exclusive_sum(int v, int lane) {
    int s = v;
#pragma unroll
    for (int o = 1; o < SVNET_WAVE; o <<= 1) {
        const int u = __shfl_up(s, o, SVNET_WAVE);
        if (lane >= o) s += u;
    }
    return s - v;
}

// FILL = false: the pass that counts; FILL = true: the pass that appends, `cur` the next free slot of this lane's list.
template <bool FILL>
__device__ __forceinline__ void reverse_pass(const int64_t* __restrict__ src, int64_t E, int64_t N, int n0, int t, int lane, int* tg,
                                             int& cnt, int& below, int cur, int32_t* __restrict__ out) {
    for (int64_t base = 0; base < E; base += REV_CHUNK) {
        if (base) __syncthreads();                               // the previous chunk has been read by every wave
#pragma unroll
        for (int i = 0; i < REV_CHUNK / REV_THREADS; ++i) {
            const int64_t e = base + i * REV_THREADS + t;
            tg[i * REV_THREADS + t] = e < E ? (int)clamp_index(src[e], N) : REV_NONE;
        }
        __syncthreads();
        const int steps = (int)((E - base < REV_CHUNK ? E - base : REV_CHUNK) + SVNET_WAVE - 1) / SVNET_WAVE;
        for (int s = 0; s < steps; ++s) {
            const int target = tg[s * SVNET_WAVE + lane];
            const int rel = target - n0;
            if (!FILL) below += (int)__popcll(__ballot(target < n0));
            unsigned long long m = __ballot(rel >= 0 && rel < SVNET_WAVE);
            while (m) {                                          // lowest lane first: ascending edge
                const int j = (int)__builtin_ctzll(m);
                m &= m - 1;
                const int owner = __shfl(rel, j, SVNET_WAVE);
                if (lane == owner) {
                    if (FILL) out[cur++] = (int32_t)(base + s * SVNET_WAVE + j);
                    else ++cnt;
                }
            }
        }
    }
}

__global__ __launch_bounds__(REV_THREADS) void pointset_reverse_kernel(const int64_t* __restrict__ idx, int64_t E, int64_t N, int64_t chunks,
                                                                       int32_t* __restrict__ rev_start, int32_t* __restrict__ rev_edge) {
    __shared__ int tg[REV_CHUNK];
    const int t = threadIdx.x, lane = lane_id();
    const int64_t b = blockIdx.x / chunks;
    const int n0 = (int)(blockIdx.x % chunks) * REV_TILE + (t & ~(SVNET_WAVE - 1));      // this wave's first destination
    const int n = n0 + lane;
    const int64_t* src = idx + b * E;
    int32_t* out = rev_edge + b * E;
    int cnt = 0, below = 0;
    reverse_pass<false>(src, E, N, n0, t, lane, tg, cnt, below, 0, out);
    const int start = below + wave_exclusive_sum(cnt, lane);
    if (n < N) {
        rev_start[b * (N + 1) + n] = start;
        if (n == N - 1) rev_start[b * (N + 1) + N] = start + cnt;                      // = E: every edge points somewhere
    }
    __syncthreads();
    reverse_pass<true>(src, E, N, n0, t, lane, tg, cnt, below, start, out);
}

// One wave per destination point (b, n); lanes along the D columns.
__global__ __launch_bounds__(GPB_THREADS) void group_points_bwd_kernel(const float* __restrict__ dgrouped, const int32_t* __restrict__ rev_start,
                                                                       const int32_t* __restrict__ rev_edge, int64_t N, int64_t E, int D,
                                                                       int64_t BN, float* __restrict__ dpoints) {
    const int lane = lane_id();
    const int64_t bn = (int64_t)blockIdx.x * (GPB_THREADS / SVNET_WAVE) + (threadIdx.x >> 6);
    if (bn >= BN) return;
    const int64_t b = bn / N, n = bn % N;
    const int32_t* st = rev_start + b * (N + 1) + n;
    const int lo = st[0], hi = st[1];
    const int32_t* list = rev_edge + b * E;
    const int W = 3 + D;
    const float* rows = dgrouped + b * E * W + 3;
    float* dst = dpoints + bn * D;
    for (int c = lane; c < D; c += SVNET_WAVE) {
        float acc = 0.f;                                         // an empty list: +0, written
        int i = lo;
        if (i < hi) acc = rows[(int64_t)list[i++] * W + c];      // the first term itself (a -0 stays a -0)
        for (; i + 4 <= hi; i += 4) {
            const float t0 = rows[(int64_t)list[i] * W + c], t1 = rows[(int64_t)list[i + 1] * W + c];
            const float t2 = rows[(int64_t)list[i + 2] * W + c], t3 = rows[(int64_t)list[i + 3] * W + c];
            acc = (((acc + t0) + t1) + t2) + t3;
        }
        for (; i < hi; ++i) acc += rows[(int64_t)list[i] * W + c];
        dst[c] = acc;
    }
}

// One thread per destination point n, ITP_DCH channels d0 .. d0 + ITP_DCH - 1 (blockIdx.y picks d0).
__global__ __launch_bounds__(ITP_THREADS) void three_interpolate_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ weight,
                                                                            const int32_t* __restrict__ rev_start,
                                                                            const int32_t* __restrict__ rev_edge, int64_t D, int64_t N,
                                                                            int64_t P, int64_t chunks, float* __restrict__ dfeat) {
    const int64_t b = blockIdx.x / chunks;
    const int64_t n = (blockIdx.x % chunks) * ITP_THREADS + threadIdx.x;
    if (n >= N) return;
    const int64_t d0 = (int64_t)blockIdx.y * ITP_DCH;
    const int nd = (int)(D - d0 < ITP_DCH ? D - d0 : ITP_DCH);
    const int32_t* st = rev_start + b * (N + 1) + n;
    const int lo = st[0], hi = st[1];
    const int32_t* list = rev_edge + b * 3 * P;
    const float* w = weight + b * 3 * P;
    const float* src = dout + (b * D + d0) * P;
    float acc[ITP_DCH];
#pragma unroll
    for (int u = 0; u < ITP_DCH; ++u) acc[u] = 0.f;              // an empty list: +0, written
    for (int i = lo; i < hi; ++i) {
        const int e = list[i];
        const float we = w[e];
        const float* col = src + e / 3;
#pragma unroll
        for (int u = 0; u < ITP_DCH; ++u) {
            if (u < nd) {
                const float term = col[(int64_t)u * P] * we;
                acc[u] = i == lo ? term : acc[u] + term;         // the first term itself (a -0 stays a -0)
            }
        }
    }
    float* dst = dfeat + (b * D + d0) * N + n;
#pragma unroll
    for (int u = 0; u < ITP_DCH; ++u)
        if (u < nd) dst[(int64_t)u * N] = acc[u];
}

}  // namespace

extern "C" int svnet_pointset_reverse_tile(void) { return REV_TILE; }
extern "C" int svnet_pointset_reverse_chunk(void) { return REV_CHUNK; }

extern "C" int svnet_pointset_reverse_supported(int64_t R, int64_t K, int64_t N) {
    return R >= 1 && K >= 1 && N >= 1 && N <= SVNET_KNN_MAX_N && R <= 0x7fffffffll / K ? 1 : 0;
}

extern "C" int svnet_pointset_reverse_i32(const int64_t* idx, int64_t B, int64_t R, int64_t K, int64_t N, int32_t* rev_start,
                                          int32_t* rev_edge, void* stream) {
    SVNET_REQUIRE(idx && rev_start && rev_edge, SVNET_E_ARG, "svnet_pointset_reverse_i32: null idx / rev_start / rev_edge");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_pointset_reverse_i32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(svnet_pointset_reverse_supported(R, K, N), SVNET_E_UNSUPPORTED,
                  "svnet_pointset_reverse_i32: R %lld, K %lld, N %lld: needs R >= 1, K >= 1, R * K <= 2^31 - 1 edges per cloud, 1 <= N <= %lld",
                  (long long)R, (long long)K, (long long)N, (long long)SVNET_KNN_MAX_N);
    const CloudGrid grid = cloud_grid(B, N, REV_TILE);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_pointset_reverse_i32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1",
                  (long long)B, (long long)N, REV_TILE);
    hipLaunchKernelGGL(pointset_reverse_kernel, dim3((unsigned)grid.blocks), dim3(REV_THREADS), 0, (hipStream_t)stream, idx, R * K, N,
                       grid.chunks, rev_start, rev_edge);
    SVNET_CHECK_LAUNCH("pointset_reverse_kernel");
    return SVNET_OK;
}

extern "C" int svnet_group_points_bwd_f32(const float* dgrouped, const int32_t* rev_start, const int32_t* rev_edge, int64_t B, int64_t N,
                                          int64_t S, int64_t nsample, int64_t D, float* dpoints, void* stream) {
    SVNET_REQUIRE(dgrouped && rev_start && rev_edge && dpoints, SVNET_E_ARG, "svnet_group_points_bwd_f32: null dgrouped / rev_start / rev_edge / dpoints");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_group_points_bwd_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(S >= 1 && nsample >= 1 && D >= 1 && D <= 0x7ffffff0ll && svnet_pointset_reverse_supported(S, nsample, N), SVNET_E_UNSUPPORTED,
                  "svnet_group_points_bwd_f32: N %lld, S %lld, nsample %lld, D %lld: needs 1 <= N <= %lld, S * nsample <= 2^31 - 1, D >= 1",
                  (long long)N, (long long)S, (long long)nsample, (long long)D, (long long)SVNET_KNN_MAX_N);
    const CloudGrid grid = cloud_grid(1, B * N, GPB_THREADS / SVNET_WAVE);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_group_points_bwd_f32: B %lld x N %lld / %d workgroups > 2^31 - 1", (long long)B,
                  (long long)N, GPB_THREADS / SVNET_WAVE);
    hipLaunchKernelGGL(group_points_bwd_kernel, dim3((unsigned)grid.blocks), dim3(GPB_THREADS), 0, (hipStream_t)stream, dgrouped, rev_start,
                       rev_edge, N, S * nsample, (int)D, B * N, dpoints);
    SVNET_CHECK_LAUNCH("group_points_bwd_kernel");
    return SVNET_OK;
}

extern "C" int svnet_three_interpolate_bwd_f32(const float* dout, const float* weight, const int32_t* rev_start, const int32_t* rev_edge,
                                               int64_t B, int64_t D, int64_t N, int64_t P, float* dfeat, void* stream) {
    SVNET_REQUIRE(dout && weight && rev_start && rev_edge && dfeat, SVNET_E_ARG,
                  "svnet_three_interpolate_bwd_f32: null dout / weight / rev_start / rev_edge / dfeat");
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_three_interpolate_bwd_f32: B %lld must be positive", (long long)B);
    SVNET_REQUIRE(D >= 1 && svnet_cdiv(D, ITP_DCH) <= 65535 && svnet_pointset_reverse_supported(P, 3, N), SVNET_E_UNSUPPORTED,
                  "svnet_three_interpolate_bwd_f32: D %lld, N %lld, P %lld: needs 1 <= D <= %d, 1 <= N <= %lld, 1 <= 3 P <= 2^31 - 1",
                  (long long)D, (long long)N, (long long)P, 65535 * ITP_DCH, (long long)SVNET_KNN_MAX_N);
    const CloudGrid grid = cloud_grid(B, N, ITP_THREADS);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_three_interpolate_bwd_f32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1",
                  (long long)B, (long long)N, ITP_THREADS);
    hipLaunchKernelGGL(three_interpolate_bwd_kernel, dim3((unsigned)grid.blocks, (unsigned)svnet_cdiv(D, ITP_DCH)), dim3(ITP_THREADS), 0,
                       (hipStream_t)stream, dout, weight, rev_start, rev_edge, D, N, P, grid.chunks, dfeat);
    SVNET_CHECK_LAUNCH("three_interpolate_bwd_kernel");
    return SVNET_OK;
}
