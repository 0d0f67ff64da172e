// Fused feature-propagation level for inference: the eval-mode forward of PointNetFeaturePropagation behind three_nn
// (models/utils/pointnet_util.py:84-92) - the interpolation of the sampled level's features, the concatenation with the skip features
// and the stack of 1x1 convolution + BatchNorm + ReLU - as ONE launch that writes C_out floats per dense point and nothing else.  The
// contract is in include/svnet_hip.h ("fused feature-propagation level") and svnet_amd/fp_fused.py; tests/fp_fused_ref.py restates it.
//   fp_fused_kernel  a workgroup of four waves takes a tile of `rows` consecutive points of one cloud (64, 32 or 16: the host's plan,
//                    the largest whose two activation buffers fit in LDS).  A thread keeps ONE row of the tile and walks its columns:
//                    the skip features points1[c, p], coalesced along p, and the interpolated ones, three gathers inside one
//                    4 S-byte row of points2 per channel with the row's indices and weights resolved once, in registers - in
//                    three_interpolate_kernel's arithmetic (propagate.hip).  Rows past N are zero rows.  The layers run through the
//                    layer engine of mlp_tile.h (shared with sa_fused.hip and sa_global.hip), one barrier between layers; the last
//                    layer's epilogue, the policy FpStore, is a channel-first global store: a lane holds one column of four
//                    consecutive points, 16 bytes.
// The folds are sa_fused.hip's (svnet_sa_fold_f32).  Built with -ffp-contract=off (Makefile, NO_CONTRACT).
#include "mlp_tile.h"

namespace {

constexpr int FP_THREADS = MLP_THREADS;
constexpr int FP_MAX_C0 = 1536, FP_MAX_S = SVNET_KNN_MAX_N;      // the envelope (svnet_fp_fused_supported)
constexpr int FP_ROWS[] = {64, 32, 16};                          // powers of two: a thread finds its row and column by mask and shift

// rows: points per workgroup, 64, 32 or 16, and shift = log2(rows); stride[p]: row stride of the activation buffer p (mlp_tile.h:
// mlp_strides); lds = 4 rows (stride[0] + stride[1]) bytes.
struct FpPlan { int rows, shift, stride[2], lds; };

inline bool fp_plan(int64_t D1, int64_t D2, int64_t L, const int64_t* widths, FpPlan& pl) {
    if (!mlp_widths_ok(L, widths) || D1 < 0 || D2 < 1 || D1 > FP_MAX_C0 || D2 > FP_MAX_C0 || D1 + D2 > FP_MAX_C0) return false;
    pl = FpPlan{};
    mlp_strides(D1 + D2, L, widths, pl.stride);
    if (!mlp_rows(FP_ROWS, pl.stride, 0, pl.rows, pl.lds)) return false;      // (not inside the envelope: 16 rows of 1540 + 260 floats are 113 KB)
    pl.shift = __builtin_ctz(pl.rows);
    return true;
}

// The last layer's epilogue (mlp_tile.h): column o of the tile's rows row .. row + 3 - four consecutive points of channel c_off + o.
// dst: out + (b C_total + c_off) N + the tile's first point.  wide: N is a multiple of 4 and out is 16-byte aligned, so are all four
// points' addresses, and the four are inside the cloud or outside it together.
struct FpStore {
    static constexpr bool LAST = true;
    float* dst;
    int64_t N;
    int nrows;
    bool wide;
    __device__ __forceinline__ void operator()(int row, int o, const float (&v)[4]) const {
        float* p = dst + (int64_t)o * N + row;
        if (wide) {
            if (row < nrows) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (row + i < nrows) p[i] = v[i];
        }
    }
};

__global__ __launch_bounds__(FP_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void fp_fused_kernel(
    const int64_t* __restrict__ idx, const float* __restrict__ weight, const float* __restrict__ points2, const float* __restrict__ points1,
    int64_t N, int S, int D1, int D2, int64_t chunks, MlpLevel lv, FpPlan pl, float* __restrict__ out, int64_t C_total, int64_t c_off, int wide) {
    extern __shared__ __align__(16) unsigned char fp_lds[];
    float* buf0 = reinterpret_cast<float*>(fp_lds);                             // [rows][stride[0]]
    float* buf1 = buf0 + pl.rows * pl.stride[0];                                // [rows][stride[1]]

    const int t = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t b = blockIdx.x / chunks;
    const int64_t p0 = (blockIdx.x % chunks) * pl.rows;                         // this workgroup's first point
    const int nrows = (int)(N - p0 < pl.rows ? N - p0 : pl.rows);
    const int nrt = (nrows + 15) >> 4;
    const int C0 = D1 + D2, C0p = (C0 + 3) & ~3;

    {                                                                           // buffer 0: row = [points1[:, p] | y | zeros to C0p]
        const int row = t & (pl.rows - 1), col = t >> pl.shift, cstep = FP_THREADS >> pl.shift;
        if (row < nrt * 16) {
            const bool live = row < nrows;
            const int64_t p = p0 + (live ? row : 0);
            float* dstrow = buf0 + row * pl.stride[0];
            const float* skip = points1 + b * D1 * N + p;
#pragma unroll 4
            for (int c = col; c < D1; c += cstep) {
                const float v = skip[(int64_t)c * N];
                dstrow[c] = live ? v : 0.f;
            }
            const int64_t e = (b * N + p) * 3;
            const int i0 = (int)clamp_index(idx[e + 0], S), i1 = (int)clamp_index(idx[e + 1], S), i2 = (int)clamp_index(idx[e + 2], S);
            const float w0 = weight[e + 0], w1 = weight[e + 1], w2 = weight[e + 2];
            const float* f = points2 + b * D2 * S;
            dstrow += D1;
#pragma unroll 4
            for (int d = col; d < D2; d += cstep) {
                const float* r = f + d * S;                                     // d S < 1536 x 32768
                const float y = (r[i0] * w0 + r[i1] * w1) + r[i2] * w2;        // three_interpolate_kernel's, never contracted
                dstrow[d] = live ? y : 0.f;
            }
            for (int d = D2 + col; d < C0p - D1; d += cstep) dstrow[d] = 0.f;
        }
    }
    __syncthreads();
    const FpStore store = {out + (b * C_total + c_off) * N + p0, N, nrows, wide != 0};
    mlp_stack<false>(nrt, lv, pl.stride, buf0, buf1, store, wave, lane);       // (no barrier behind the global stores)
}

}  // namespace

extern "C" int svnet_fp_fused_rows_tile(int64_t D1, int64_t D2, int64_t L, const int64_t* widths) {
    FpPlan pl;
    return fp_plan(D1, D2, L, widths, pl) ? pl.rows : 0;
}

extern "C" int svnet_fp_fused_supported(int64_t N, int64_t S, int64_t D1, int64_t D2, int64_t L, const int64_t* widths) {
    FpPlan pl;
    if (N < 1 || S < 1 || S > FP_MAX_S || !fp_plan(D1, D2, L, widths, pl)) return 0;
    return svnet_cdiv(N, pl.rows) <= 0x7fffffffll ? 1 : 0;
}

extern "C" int svnet_fp_fused_f32(const int64_t* idx, const float* weight, const float* points2, const float* points1, int64_t B, int64_t N,
                                  int64_t S, int64_t D1, int64_t D2, int64_t L, const int64_t* widths, const void* wf, const void* bf, float* out,
                                  int64_t C_total, int64_t c_off, void* stream) {
    SVNET_REQUIRE(idx && weight && points2 && widths && wf && bf && out, SVNET_E_ARG, "svnet_fp_fused_f32: null idx / weight / points2 / widths / wf / bf / out");
    SVNET_REQUIRE(points1 || D1 == 0, SVNET_E_ARG, "svnet_fp_fused_f32: null points1 with D1 %lld > 0", (long long)D1);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_fp_fused_f32: B %lld must be positive", (long long)B);
    FpPlan pl;
    SVNET_REQUIRE(svnet_fp_fused_supported(N, S, D1, D2, L, widths) && fp_plan(D1, D2, L, widths, pl), SVNET_E_UNSUPPORTED,
                  "svnet_fp_fused_f32: N %lld, S %lld, D1 %lld, D2 %lld, L %lld: needs N >= 1, 1 <= S <= %lld, D1 >= 0, D2 >= 1, D1 + D2 <= %d, 1 <= L <= %d, every 1 <= width <= %d",
                  (long long)N, (long long)S, (long long)D1, (long long)D2, (long long)L, (long long)FP_MAX_S, FP_MAX_C0, SVNET_SA_MAX_LAYERS,
                  MLP_MAX_WIDTH);
    if (const int e = mlp_window("svnet_fp_fused_f32", c_off, widths[L - 1], C_total)) return e;
    MlpLevel lv;
    if (const int e = mlp_level("svnet_fp_fused_f32", D1 + D2, L, widths, wf, bf, lv)) return e;
    const CloudGrid grid = cloud_grid(B, N, pl.rows);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_fp_fused_f32: B %lld x ceil(N %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)N, pl.rows);
    if (const int e = mlp_lds_optin<&fp_fused_kernel>("svnet_fp_fused_f32", pl.lds)) return e;
    const int wide = N % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    hipLaunchKernelGGL(fp_fused_kernel, dim3((unsigned)grid.blocks), dim3(FP_THREADS), (size_t)pl.lds, (hipStream_t)stream, idx, weight, points2,
                       mlp_optional(points1, points2), N, (int)S, (int)D1, (int)D2, grid.chunks, lv, pl, out, C_total, c_off, wide);
    SVNET_CHECK_LAUNCH("fp_fused_kernel");
    return SVNET_OK;
}
