// Fused global set-abstraction level for inference: the eval-mode forward of a PointNetSetAbstraction with group_all
// (models/utils/pointnet_util.py:49-63 behind sample_and_group_all) - the concatenation [xyz | points] of ALL points of a cloud, the
// stack of 1x1 convolution + BatchNorm + ReLU and the max over the cloud - as two launches that write C_out floats per cloud and nothing
// else.  The contract is in include/svnet_hip.h ("fused global set-abstraction level") and svnet_amd/sa_global.py;
// tests/sa_global_ref.py restates it.  Two kernels:
//   sg_zero_kernel    +0 into the channels c_off .. c_off + C_L - 1 of every cloud: the start of the integer maxima below.
//   sa_global_kernel  a workgroup of four waves takes a tile of `rows` consecutive points of one cloud (64, 48, 32 or 16: the host's
//                     plan, the largest whose two activation buffers and table of maxima fit in LDS), so a cloud is split over
//                     ceil(N / rows) workgroups.  The columns xyz[c, p] and points[d, p] are read channel-first as they lie, coalesced
//                     along p; rows past N are zero rows.  The layers run through the layer engine of mlp_tile.h (shared with
//                     sa_fused.hip and fp_fused.hip), one barrier per layer.  The last layer is not stored: its ReLU outputs, >= +0,
//                     are folded over the lane's rows in registers - the rows past N left out: a zero row's output is the ReLU of the
//                     bias chain, which may exceed every real row's - then go by one integer LDS maximum on the bit pattern into
//                     the workgroup's table (the epilogue policy SgMax), and the table by one integer global maximum per column into
//                     out.  Non-negative floats order as their bit patterns and an integer maximum has no order: the bits do not
//                     depend on how a cloud is tiled or on which workgroup arrives first.  No float atomics.
// The folds are sa_fused.hip's (svnet_sa_fold_f32).  Built with -ffp-contract=off (Makefile, NO_CONTRACT).
#include "mlp_tile.h"

namespace {

constexpr int SG_THREADS = MLP_THREADS;
constexpr int SG_MAX_N = SVNET_KNN_MAX_N, SG_MAX_D = 1024, SG_MAX_WIDTH = 1024;      // the envelope (svnet_sa_global_supported)
constexpr int SG_ROWS[] = {64, 48, 32, 16};                      // whole 16-row tiles

// rows: points per workgroup; stride[p]: row stride of the activation buffer p and opad: the last width padded to whole column tiles
// (mlp_tile.h: mlp_strides, mlp_opad); lds = 4 rows (stride[0] + stride[1]) + 4 opad bytes.
struct SgPlan { int rows, stride[2], opad, lds; };

inline bool sg_plan(int64_t D, int64_t L, const int64_t* widths, SgPlan& pl) {
    if (!mlp_widths_ok(L, widths, SG_MAX_WIDTH) || D < 0 || D > SG_MAX_D) return false;
    pl = SgPlan{};
    pl.opad = mlp_opad(L, widths);
    mlp_strides(3 + D, L, widths, pl.stride);
    return mlp_rows(SG_ROWS, pl.stride, 4 * pl.opad, pl.rows, pl.lds);      // (true inside the envelope: 16 rows of 1028 + 1028 floats and 1024 maxima are 133 KB)
}

__global__ __launch_bounds__(SG_THREADS) void sg_zero_kernel(float* __restrict__ out, int64_t total, int CL, int64_t C_total, int64_t c_off) {
    for (int64_t e = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x; e < total; e += (int64_t)gridDim.x * SG_THREADS) {
        const int64_t b = e / CL;
        out[b * C_total + c_off + (e - b * CL)] = 0.f;
    }
}

// The last layer's epilogue (mlp_tile.h): the ReLU outputs, >= +0, of column o and rows row .. row + 3.  The engine walks a column
// tile's row tiles in ascending order, so the lane's running maximum m - bit patterns; +0 is the neutral start - collects the rows
// below nrows of all of them and goes into the table once, at the last row tile (rows >= last).
struct SgMax {
    static constexpr bool LAST = true;
    unsigned* smax;
    int nrows, last;
    unsigned m;
    __device__ __forceinline__ void operator()(int row, int o, const float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned u = __float_as_uint(v[i]);
            if (row + i < nrows && u > m) m = u;
        }
        if (row >= last) {
            if (m) atomicMax(smax + o, m);
            m = 0u;
        }
    }
};

__global__ __launch_bounds__(SG_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void sa_global_kernel(
    const float* __restrict__ xyz, const float* __restrict__ points, int64_t N, int D, int64_t chunks, MlpLevel lv, SgPlan pl,
    float* __restrict__ out, int64_t C_total, int64_t c_off) {
    extern __shared__ __align__(16) unsigned char sg_lds[];
    unsigned* smax = reinterpret_cast<unsigned*>(sg_lds);                       // [opad] bit patterns of the tile's maxima, all >= +0
    float* buf0 = reinterpret_cast<float*>(smax + pl.opad);                     // [rows][stride[0]]
    float* buf1 = buf0 + pl.rows * pl.stride[0];                                // [rows][stride[1]]

    const int t = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t b = blockIdx.x / chunks;
    const int64_t p0 = (blockIdx.x % chunks) * pl.rows;                         // this workgroup's first point
    const int nrows = (int)(N - p0 < pl.rows ? N - p0 : pl.rows);
    const int nrt = (nrows + 15) >> 4, r16 = nrt * 16;
    const int C0 = 3 + D, C0p = (C0 + 3) & ~3, OL = lv.C[lv.L];

    for (int o = t; o < OL; o += SG_THREADS) smax[o] = 0u;
    {                                                                           // buffer 0: row = [xyz[:, p] | points[:, p] | zeros to C0p]
        const int cstep = SG_THREADS / r16, col = t / r16, row = t - col * r16;      // (48 rows: five columns at a time, 16 threads idle)
        if (col < cstep) {
            const bool live = row < nrows;
            const int64_t p = p0 + (live ? row : 0);
            const float* xb = xyz + b * 3 * N + p;
            const float* pb = points + b * D * N + p;                           // (D = 0: never read)
            float* dstrow = buf0 + row * pl.stride[0];
#pragma unroll 4
            for (int c = col; c < C0p; c += cstep) {
                const int cc = c < C0 ? c : C0 - 1;
                const float v = cc < 3 ? xb[(int64_t)cc * N] : pb[(int64_t)(cc - 3) * N];
                dstrow[c] = live && c < C0 ? v : 0.f;
            }
        }
    }
    __syncthreads();
    mlp_stack<true>(nrt, lv, pl.stride, buf0, buf1, SgMax{smax, nrows, r16 - 16, 0u}, wave, lane);      // (the barrier: smax is read below)
    // across the workgroups of a cloud: an integer maximum on the bit patterns of out, which sg_zero_kernel set to +0
    unsigned* dst = reinterpret_cast<unsigned*>(out + b * C_total + c_off);
    for (int o = t; o < OL; o += SG_THREADS) {
        const unsigned m = smax[o];
        if (m) atomicMax(dst + o, m);
    }
}

}  // namespace

extern "C" int svnet_sa_global_rows_tile(int64_t D, int64_t L, const int64_t* widths) {
    SgPlan pl;
    return sg_plan(D, L, widths, pl) ? pl.rows : 0;
}

extern "C" int svnet_sa_global_supported(int64_t N, int64_t D, int64_t L, const int64_t* widths) {
    SgPlan pl;
    return N >= 1 && N <= SG_MAX_N && sg_plan(D, L, widths, pl) ? 1 : 0;
}

extern "C" int svnet_sa_global_f32(const float* xyz, const float* points, int64_t B, int64_t N, int64_t D, int64_t L, const int64_t* widths,
                                   const void* wf, const void* bf, float* out, int64_t C_total, int64_t c_off, void* stream) {
    SVNET_REQUIRE(xyz && widths && wf && bf && out, SVNET_E_ARG, "svnet_sa_global_f32: null xyz / widths / wf / bf / out");
    SVNET_REQUIRE(points || D == 0, SVNET_E_ARG, "svnet_sa_global_f32: null points with D %lld > 0", (long long)D);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_sa_global_f32: B %lld must be positive", (long long)B);
    SgPlan pl;
    SVNET_REQUIRE(svnet_sa_global_supported(N, D, L, widths) && sg_plan(D, L, widths, pl), SVNET_E_UNSUPPORTED,
                  "svnet_sa_global_f32: N %lld, D %lld, L %lld: needs 1 <= N <= %d, 0 <= D <= %d, 1 <= L <= %d, every 1 <= width <= %d",
                  (long long)N, (long long)D, (long long)L, SG_MAX_N, SG_MAX_D, SVNET_SA_MAX_LAYERS, SG_MAX_WIDTH);
    if (const int e = mlp_window("svnet_sa_global_f32", c_off, widths[L - 1], C_total)) return e;
    MlpLevel lv;
    if (const int e = mlp_level("svnet_sa_global_f32", 3 + D, L, widths, wf, bf, lv)) return e;
    const CloudGrid grid = cloud_grid(B, N, pl.rows);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_sa_global_f32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)N, pl.rows);
    if (const int e = mlp_lds_optin<&sa_global_kernel>("svnet_sa_global_f32", pl.lds)) return e;
    const int CL = (int)widths[L - 1];
    hipLaunchKernelGGL(sg_zero_kernel, dim3(svnet_grid(B * CL, SG_THREADS)), dim3(SG_THREADS), 0, (hipStream_t)stream, out, B * CL, CL, C_total, c_off);
    SVNET_CHECK_LAUNCH("sg_zero_kernel");
    hipLaunchKernelGGL(sa_global_kernel, dim3((unsigned)grid.blocks), dim3(SG_THREADS), (size_t)pl.lds, (hipStream_t)stream, xyz, mlp_optional(points, xyz), N,
                       (int)D, grid.chunks, lv, pl, out, C_total, c_off);
    SVNET_CHECK_LAUNCH("sa_global_kernel");
    return SVNET_OK;
}
