// Fused set-abstraction level for inference: the eval-mode forward of PointNetSetAbstraction / PointNetSetAbstractionMsg after the
// query (models/utils/pointnet_util.py:166-267) - grouping, the stack of 1x1 convolution + BatchNorm + ReLU and the max over a group -
// as ONE launch that writes C_out floats per centre and nothing else.  The contract is in include/svnet_hip.h ("fused set-abstraction
// level") and svnet_amd/sa_fused.py; tests/sa_fused_ref.py restates it.  Two kernels:
//   sa_fold_kernel   BatchNorm's running statistics folded into a layer's weights and bias, every operation rounded once.
//   sa_fused_kernel  a workgroup takes a tile of SF_ROWS grouped rows - whole centres when a group has at most SF_ROWS slots, else the
//                    tiles of one centre one after the other - gathers them into LDS and runs the layers through the layer engine
//                    of mlp_tile.h (v_mfma_f32_16x16x4_f32, bit for bit a c-ascending fmaf chain that starts at the bias; the engine
//                    is shared with the other levels).  The last layer is not stored: its ReLU output, >= +0, goes into a per-centre
//                    column maximum by an integer LDS maximum on the bit patterns, which is order-free (the epilogue policy SaMax).
// Built with -ffp-contract=off (Makefile, NO_CONTRACT).
#include "mlp_tile.h"

namespace {

constexpr int SF_THREADS = MLP_THREADS;
constexpr int SF_ROWS = 64;                                      // grouped rows per tile: four 16-row MFMA tiles
constexpr int SF_MAX_C0 = 324, SF_MAX_WIDTH = MLP_MAX_WIDTH;     // the envelope (svnet_sa_fused_supported)
constexpr int SF_MAX_FLOATS = 2048;                              // the running maxima: centres per workgroup x padded last width, at most
constexpr int SF_LDS_MAX = MLP_LDS_MAX;
constexpr int SF_HEAD = SF_ROWS * 8 + SF_ROWS * 4 + (SF_ROWS + 4) * 4 + SF_ROWS * 4;      // s_src | s_ctr | s_start (+ total) | s_lim
static_assert(SF_HEAD % 16 == 0, "the float regions behind the row tables stay 16-byte aligned");

// cpw: centres per workgroup; stride[p]: row stride of the activation buffer p and opad: the last width padded to whole column tiles
// (mlp_tile.h: mlp_strides, mlp_opad).
struct SaPlan { int cpw, stride[2], opad, lds; };

inline bool sa_plan(int64_t N, int64_t S, int64_t K, int64_t D, int64_t L, const int64_t* widths, SaPlan& pl) {
    if (!mlp_widths_ok(L, widths) || !svnet_group_supported(N, S, K, D) || 3 + D > SF_MAX_C0) return false;
    pl = SaPlan{};
    pl.opad = mlp_opad(L, widths);
    mlp_strides(3 + D, L, widths, pl.stride);
    const int fixed = SF_HEAD + 4 * SF_ROWS * (pl.stride[0] + pl.stride[1]);
    int64_t room = (SF_LDS_MAX - fixed) / 4;                     // floats left for the maxima
    if (room > SF_MAX_FLOATS) room = SF_MAX_FLOATS;
    const int64_t fit = room / pl.opad, whole = SF_ROWS / K;
    if (fit < 1) return false;                                   // (not inside the envelope: 324 and 256 columns leave room for 3000)
    pl.cpw = (int)(whole < 1 ? 1 : whole < fit ? whole : fit);
    pl.lds = fixed + 4 * pl.cpw * pl.opad;
    return true;
}

__global__ __launch_bounds__(SF_THREADS) void sa_fold_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ rmean,
                                                             const float* __restrict__ rvar, int64_t OC, int C, float eps,
                                                             float* __restrict__ Wf, float* __restrict__ bf) {
    const int64_t e = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x;
    if (e >= OC) return;
    const int64_t o = e / C;
    const float invstd = 1.f / sqrtf(rvar[o] + eps);             // bn_eval_stats_kernel's (norm.hip)
    const float s = gamma[o] * invstd;
    Wf[e] = W[e] * s;
    if (e == o * C) bf[o] = (b[o] - rmean[o]) * s + beta[o];
}

// The last layer's epilogue (mlp_tile.h): the ReLU outputs, >= +0, of column o and rows row .. row + 3 go into the centres' maxima.
// Rows ascend, so a centre's rows are adjacent: one maximum per run of equal centres; -1 marks a row past the tile's.
struct SaMax {
    static constexpr bool LAST = true;
    const int* s_ctr;
    unsigned* smax;
    int opad;
    __device__ __forceinline__ void operator()(int row, int o, const float (&v)[4]) const {
        const int4 cv = *reinterpret_cast<const int4*>(s_ctr + row);
        const int ctr[4] = {cv.x, cv.y, cv.z, cv.w};
        int cur = ctr[0];
        float m = v[0];
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            if (ctr[i] != cur) {
                if (cur >= 0) atomicMax(smax + cur * opad + o, __float_as_uint(m));
                cur = ctr[i];
                m = v[i];
            } else {
                m = m > v[i] ? m : v[i];
            }
        }
        if (cur >= 0) atomicMax(smax + cur * opad + o, __float_as_uint(m));
    }
};

__global__ __launch_bounds__(SF_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void sa_fused_kernel(const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                              const float* __restrict__ points, const int64_t* __restrict__ idx, int64_t idx_ld,
                                                              const int* __restrict__ count, int64_t count_ld, int64_t N, int64_t S, int K,
                                                              int D, int64_t chunks, MlpLevel lv, SaPlan pl, int xyz_last,
                                                              float* __restrict__ out, int64_t C_total, int64_t c_off) {
    extern __shared__ __align__(16) unsigned char sf_lds[];
    int64_t* s_src = reinterpret_cast<int64_t*>(sf_lds);                        // [SF_ROWS] b * N + the row's point
    int* s_ctr = reinterpret_cast<int*>(sf_lds + SF_ROWS * 8);                  // [SF_ROWS] the row's centre in the workgroup, -1: no row
    int* s_start = s_ctr + SF_ROWS;                                             // [SF_ROWS + 4] a centre's first row; [SF_ROWS]: all rows
    int* s_lim = s_start + SF_ROWS + 4;                                         // [SF_ROWS] a centre's rows
    unsigned* smax = reinterpret_cast<unsigned*>(sf_lds + SF_HEAD);             // [cpw][opad] bit patterns of the maxima, all >= +0
    float* buf0 = reinterpret_cast<float*>(smax + pl.cpw * pl.opad);
    float* buf1 = buf0 + SF_ROWS * pl.stride[0];

    const int t = threadIdx.x, lane = lane_id();
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int64_t b = blockIdx.x / chunks;
    const int64_t s0 = (blockIdx.x % chunks) * pl.cpw;                          // this workgroup's first centre
    const int ncen = (int)(S - s0 < pl.cpw ? S - s0 : pl.cpw);
    const int C0 = 3 + D, C0p = (C0 + 3) & ~3, OL = lv.C[lv.L];

    if (wave == 0) {                                                            // the centres' row counts and their running sum
        int lim = 0;
        if (lane < ncen) {
            lim = K;
            if (count) {
                const int c = count[(b * S + s0 + lane) * count_ld];
                lim = c < 1 ? 1 : c < K ? c : K;
            }
        }
        int inc = lim;
#pragma unroll
        for (int o = 1; o < SVNET_WAVE; o <<= 1) {
            const int v = __shfl_up(inc, o, SVNET_WAVE);
            if (lane >= o) inc += v;
        }
        s_lim[lane] = lim;
        s_start[lane] = inc - lim;
        if (lane == SVNET_WAVE - 1) s_start[SF_ROWS] = inc;
    }
    for (int e = t; e < ncen * pl.opad; e += SF_THREADS) smax[e] = 0u;
    __syncthreads();
    const int total = __builtin_amdgcn_readfirstlane(s_start[SF_ROWS]);        // >= 1; at most SF_ROWS unless cpw = 1

    for (int base = 0; base < total; base += SF_ROWS) {
        const int nrows = total - base < SF_ROWS ? total - base : SF_ROWS;
        const int nrt = (nrows + 15) >> 4;
        if (wave == 0) {                                                        // the rows' points: one wave, its LDS writes keep their order
            s_ctr[lane] = -1;
            int c = 0, j = base + lane;                                         // one centre, tile by tile
            bool on = lane < nrows;
            if (K < SF_ROWS) {                                                  // whole centres: lane = centre * K + slot
                c = lane / K;
                j = lane - c * K;
                on = c < ncen && j < s_lim[c];
            }
            if (on) {
                const int r = K < SF_ROWS ? s_start[c] + j : lane;
                s_src[r] = b * N + clamp_index(idx[(b * S + s0 + c) * idx_ld + j], N);
                s_ctr[r] = c;
            }
        }
        __syncthreads();
        {                                                                       // the centred rows, zero where there is no row or column
            const int totalE = nrt * 16 * C0p;
            const int qstep = SF_THREADS / C0p, rstep = SF_THREADS % C0p;
            int row = t / C0p, col = t % C0p;
            for (int e = t; e < totalE; e += SF_THREADS) {
                const int c = s_ctr[row];
                float v = 0.f;
                if (c >= 0 && col < C0) {
                    const int64_t src = s_src[row];
                    const int x = xyz_last ? col - D : col;                     // the coordinate, where 0 <= x < 3
                    if (x >= 0 && x < 3) v = xyz[src * 3 + x] - new_xyz[(b * S + s0 + c) * 3 + x];
                    else v = points[src * D + (xyz_last ? col : col - 3)];
                }
                buf0[row * pl.stride[0] + col] = v;
                col += rstep; row += qstep;
                if (col >= C0p) { col -= C0p; ++row; }
            }
        }
        __syncthreads();
        mlp_stack<true>(nrt, lv, pl.stride, buf0, buf1, SaMax{s_ctr, smax, pl.opad}, wave, lane);      // (the barrier: smax, and the next tile's tables)
    }
    // channel-first: the workgroup's centres of a channel lie side by side
    float* dst = out + (b * C_total + c_off) * S + s0;
    for (int e = t; e < ncen * OL; e += SF_THREADS) {
        const int o = e / ncen, sl = e - o * ncen;
        dst[(int64_t)o * S + sl] = __uint_as_float(smax[sl * pl.opad + o]);
    }
}

}  // namespace

extern "C" int svnet_sa_fused_rows_tile(void) { return SF_ROWS; }

extern "C" int svnet_sa_fused_supported(int64_t N, int64_t S, int64_t K, int64_t D, int64_t L, const int64_t* widths) {
    SaPlan pl;
    return sa_plan(N, S, K, D, L, widths, pl) ? 1 : 0;
}

extern "C" int svnet_sa_fold_f32(const float* W, const float* b, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, int64_t O, int64_t C, float eps, float* Wf, float* bf, void* stream) {
    SVNET_REQUIRE(W && b && gamma && beta && running_mean && running_var && Wf && bf, SVNET_E_ARG,
                  "svnet_sa_fold_f32: null W / b / gamma / beta / running_mean / running_var / Wf / bf");
    SVNET_REQUIRE(O >= 1 && C >= 1, SVNET_E_ARG, "svnet_sa_fold_f32: O %lld and C %lld must be positive", (long long)O, (long long)C);
    SVNET_REQUIRE(O <= 0x7fffffffll / C, SVNET_E_UNSUPPORTED, "svnet_sa_fold_f32: O %lld x C %lld weights > 2^31 - 1", (long long)O, (long long)C);
    hipLaunchKernelGGL(sa_fold_kernel, dim3((unsigned)svnet_cdiv(O * C, SF_THREADS)), dim3(SF_THREADS), 0, (hipStream_t)stream, W, b, gamma, beta,
                       running_mean, running_var, O * C, (int)C, eps, Wf, bf);
    SVNET_CHECK_LAUNCH("sa_fold_kernel");
    return SVNET_OK;
}

extern "C" int svnet_sa_fused_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t idx_ld, const int* count,
                                  int64_t count_ld, int64_t B, int64_t N, int64_t S, int64_t K, int64_t D, int64_t L, const int64_t* widths,
                                  const void* wf, const void* bf, int xyz_last, float* out, int64_t C_total, int64_t c_off, void* stream) {
    SVNET_REQUIRE(xyz && new_xyz && idx && widths && wf && bf && out, SVNET_E_ARG, "svnet_sa_fused_f32: null xyz / new_xyz / idx / widths / wf / bf / out");
    SVNET_REQUIRE(points || D == 0, SVNET_E_ARG, "svnet_sa_fused_f32: null points with D %lld > 0", (long long)D);
    SVNET_REQUIRE(B >= 1, SVNET_E_ARG, "svnet_sa_fused_f32: B %lld must be positive", (long long)B);
    SaPlan pl;
    SVNET_REQUIRE(sa_plan(N, S, K, D, L, widths, pl), SVNET_E_UNSUPPORTED,
                  "svnet_sa_fused_f32: N %lld, S %lld, K %lld, D %lld, L %lld: needs 1 <= K <= N <= %lld, S >= 1, 0 <= D <= %d, 1 <= L <= %d, every 1 <= width <= %d",
                  (long long)N, (long long)S, (long long)K, (long long)D, (long long)L, (long long)SVNET_KNN_MAX_N, SF_MAX_C0 - 3,
                  SVNET_SA_MAX_LAYERS, SF_MAX_WIDTH);
    SVNET_REQUIRE(idx_ld >= K && (!count || count_ld >= 1), SVNET_E_ARG, "svnet_sa_fused_f32: idx_ld %lld < K %lld, or count_ld %lld < 1",
                  (long long)idx_ld, (long long)K, (long long)count_ld);
    if (const int e = mlp_window("svnet_sa_fused_f32", c_off, widths[L - 1], C_total)) return e;
    SVNET_REQUIRE(B <= 0x7fffffffll / S / idx_ld, SVNET_E_UNSUPPORTED, "svnet_sa_fused_f32: B %lld x S %lld x idx_ld %lld indices > 2^31 - 1",
                  (long long)B, (long long)S, (long long)idx_ld);
    MlpLevel lv;
    if (const int e = mlp_level("svnet_sa_fused_f32", 3 + D, L, widths, wf, bf, lv)) return e;
    const CloudGrid grid = cloud_grid(B, S, pl.cpw);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_sa_fused_f32: B %lld x ceil(S %lld / %d) workgroups > 2^31 - 1", (long long)B,
                  (long long)S, pl.cpw);
    if (const int e = mlp_lds_optin<&sa_fused_kernel>("svnet_sa_fused_f32", pl.lds)) return e;
    hipLaunchKernelGGL(sa_fused_kernel, dim3((unsigned)grid.blocks), dim3(SF_THREADS), (size_t)pl.lds, (hipStream_t)stream, xyz, new_xyz,
                       mlp_optional(points, xyz), idx, idx_ld, count, count_ld, N, S, (int)K, (int)D, grid.chunks, lv, pl, xyz_last, out, C_total, c_off);
    SVNET_CHECK_LAUNCH("sa_fused_kernel");
    return SVNET_OK;
}
