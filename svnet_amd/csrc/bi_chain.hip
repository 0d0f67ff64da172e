// The shared binary MLP of BiPointNet (models/bipointnet.py: BiSTN3d, BiSTNkd, BiPointNetEncoder in eval mode) as ONE chain per launch:
// up to four layers over the points of a cloud, the first optionally full precision, the others ternary-sign activations against
// ternary-sign weights, and an epilogue that either writes the last layer or keeps its maximum over the cloud.
//
// The contract is in include/svnet_hip.h (fused binary chain) and restated in numpy in tests/bi_ref.py.  Two facts carry the design:
//   sign(hardtanh(y)) = sign(y)      between binary layers only one sign per (point, channel) survives: it is written to LDS as an int8
//                                    straight from the accumulators, never to memory;
//   t = fmaf(d, a, b) is monotone in the integer count d, so the maximum over the points is the affine of an integer extreme:
//                                    max d where a >= 0, min d where a < 0, applied once per (tile, channel).
//   bi_fold_kernel     one workgroup: the float64 sum of W in a stated order, m = fl(S / (O K)), the ternary signs sgn(fl(W - m)) as the
//                      chain's packed int8 (rows padded to 32 outputs, columns to 32 inputs, zero filled) and / or as floats, a | b.
//   bi_chain_kernel    a workgroup = 4 waves takes BC_ROWS consecutive points of one cloud.  Two LDS regions ping-pong: the x tile
//                      (floats when a transform or an fp layer reads it, signs else), the transformed tile, then each layer's signs
//                      [row][channel] with a row stride of (widest binary input rounded to 32) + 16 bytes.  A binary layer walks its
//                      outputs in blocks of 32: wave w takes blocks w, w + 4, ..; per k-step of 32 inputs one 16-byte weight fragment
//                      from memory (the next one requested before the products of this one) against the four 32-row fragments of
//                      the tile on v_mfma_i32_32x32x32_i8 (binlinear_mfma.hip's operand map: lane (r, h) holds row / column r,
//                      positions 16 h .. 16 h + 15; accumulator i is row (i & 3) + 8 (i >> 2) + 4 h of column r).  A lane therefore
//                      holds ONE output channel and 16 rows of it: the extreme over the rows is 16 integer compares in registers, one
//                      half swap, and the next row block.  The fp prefix (3 -> 64, a transform of at most 64 x 64) is the stated fmaf
//                      chain on the vector unit, c ascending.
//   bi_chain_finish_kernel   clouds of more than one tile: the maximum over the tiles' partials, then the offset.  Order-free.
// int8 MFMA against bit-plane popcount at K = 64 / 128: DESIGN.md 4.35.  Built with -ffp-contract=off (Makefile, NO_CONTRACT).
#include "common.h"

#include <limits.h>

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

constexpr int BC_THREADS = 256;
constexpr int BC_ROWS = 128;                      // points per workgroup: four 32-row MFMA blocks
constexpr int BC_MAX_L = 4, BC_MAX_C0F = 64, BC_MAX_FPW = 512, BC_MAX_K = 512, BC_MAX_LAST = 2048, BC_MAX_B = 65535;
constexpr int BC_RED = 2 * BC_MAX_FPW * 4;        // bytes behind the regions: the two half-tile maxima of an fp layer that is pooled
constexpr int BC_LDS_MAX = 2 * BC_ROWS * (BC_MAX_K + 16) + BC_RED;
constexpr int FOLD_THREADS = 1024;
constexpr int FOLD_MAX_WEIGHTS = 1 << 24;       // one workgroup folds a layer: the fully connected 256 -> 4096 is 2^20

inline int64_t up32(int64_t v) { return (v + 31) / 32 * 32; }

struct BiLayer {
    const void* w;        // binary: packed int8 [up32(O)][up32(K)]; fp: Wf [O][K] floats
    const float* ab;      // binary: a [O] | b [O]; fp: bf [O]
    int K, O;
};
struct BiPlan {
    int L, first_fp, stride, region, lds, tiles;
    BiLayer layer[BC_MAX_L];
};

// The limits (svnet_bi_chain_supported) and the LDS plan.  widths: the L layer widths; C0: the input width.
inline bool bi_plan(int64_t C0, int64_t N, int64_t L, const int64_t* widths, int first_fp, int has_trans, BiPlan& pl) {
    if (!widths || L < 1 || L > BC_MAX_L || N < 1 || N > SVNET_KNN_MAX_N || C0 < 1) return false;
    if ((has_trans || first_fp) && C0 > BC_MAX_C0F) return false;
    int64_t in = C0, kmax = 0;
    for (int64_t l = 0; l < L; ++l) {
        if (widths[l] < 1) return false;
        if (l == 0 && first_fp) {
            if (widths[0] > BC_MAX_FPW) return false;
        } else {
            if (in > BC_MAX_K) return false;
            if (in > kmax) kmax = in;
        }
        in = widths[l];
    }
    if (in > BC_MAX_LAST) return false;
    pl = BiPlan{};
    pl.L = (int)L;
    pl.first_fp = first_fp ? 1 : 0;
    pl.stride = kmax ? (int)up32(kmax) + 16 : 0;
    int64_t region = (int64_t)BC_ROWS * pl.stride;
    if ((has_trans || first_fp) && region < C0 * BC_ROWS * 4) region = C0 * BC_ROWS * 4;
    if (region < 16) region = 16;
    pl.region = (int)((region + 15) / 16 * 16);
    pl.lds = 2 * pl.region + BC_RED;
    pl.tiles = (int)svnet_cdiv(N, BC_ROWS);
    return pl.lds <= BC_LDS_MAX;
}

__device__ __forceinline__ int8_t sgn8(float t) { return (int8_t)((t > 0.f) - (t < 0.f)); }

__global__ __launch_bounds__(FOLD_THREADS) void bi_fold_kernel(const float* __restrict__ W, const float* __restrict__ scale,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const float* __restrict__ rmean, const float* __restrict__ rvar, int O, int K,
                                                               float eps, int8_t* __restrict__ w_i8, float* __restrict__ s_f32,
                                                               float* __restrict__ ab) {
    __shared__ double sh[FOLD_THREADS];
    const int tid = threadIdx.x;
    const int total = O * K;
    // S: lane t adds W[t], W[t + 1024], .. in that order; then the halving tree sh[i] += sh[i + s], s = 512 .. 1
    double acc = 0.0;
    for (int e = tid; e < total; e += FOLD_THREADS) acc += (double)W[e];
    sh[tid] = acc;
    __syncthreads();
    for (int s = FOLD_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const float m = (float)(sh[0] / (double)total);
    if (w_i8) {
        const int Kp = (int)(((int64_t)K + 31) / 32 * 32), Op = (int)(((int64_t)O + 31) / 32 * 32);
        for (int e = tid; e < Op * Kp; e += FOLD_THREADS) {
            const int o = e / Kp, k = e - o * Kp;
            w_i8[e] = (o < O && k < K) ? sgn8(W[(int64_t)o * K + k] - m) : (int8_t)0;
        }
    }
    if (s_f32)
        for (int e = tid; e < total; e += FOLD_THREADS) s_f32[e] = (float)sgn8(W[e] - m);
    const float sc = scale[0];
    for (int o = tid; o < O; o += FOLD_THREADS) {
        if (gamma) {
            const float invstd = 1.f / sqrtf(rvar[o] + eps);          // sa_fold_kernel's (sa_fused.hip)
            const float s = gamma[o] * invstd;
            ab[o] = sc * s;
            ab[O + o] = beta[o] - rmean[o] * s;
        } else {
            ab[o] = sc;
            ab[O + o] = 0.f;
        }
    }
}

struct ChainArgs {
    const float* x;
    const float* T;
    int C0, N, pool, clamp;
    float offset;
    float* part;
    float* out;
};

// The maximum of channel o over this tile's rows: the cloud's when it has one tile, else a partial for bi_chain_finish_kernel.
__device__ __forceinline__ void emit_max(const ChainArgs& g, const BiPlan& pl, int b, int tile, int O, int o, float m) {
    if (pl.tiles == 1) g.out[(int64_t)b * O + o] = m + g.offset;
    else g.part[((int64_t)b * pl.tiles + tile) * O + o] = m;
}

__device__ __forceinline__ float clamp1(float t, int clamp) { return clamp ? fminf(fmaxf(t, -1.f), 1.f) : t; }

template <bool POOL>
// One fp layer on the vector unit: thread = (row, output parity), the stated chain t = bf[o]; c ascending t = fmaf(u[c], Wf[o,c], t).
__device__ __forceinline__ void fp_layer(const ChainArgs& g, const BiPlan& pl, const BiLayer& ly, bool last, const unsigned char* cur,
                                         unsigned char* nxt, float* red, int b, int tile, int rows, int tid) {
    const float* uf = reinterpret_cast<const float*>(cur);
    const float* Wf = reinterpret_cast<const float*>(ly.w);
    const int row = tid & (BC_ROWS - 1), K = ly.K, O = ly.O;
    const int half = (tid >> 6) & 1;
    for (int o = tid >> 7; o < O; o += 2) {                          // (wave-uniform o: the weights are scalar loads)
        float t = ly.ab[o];
        for (int c = 0; c < K; ++c) t = fmaf(uf[c * BC_ROWS + row], Wf[o * K + c], t);
        if (!last) {
            nxt[row * pl.stride + o] = (unsigned char)sgn8(t);
        } else if (!POOL) {
            if (row < rows) g.out[((int64_t)b * O + o) * g.N + (int64_t)tile * BC_ROWS + row] = clamp1(t, g.clamp);
        } else {
            const float v = wave_max(row < rows ? t : -INFINITY);
            if ((tid & 63) == 0) red[half * BC_MAX_FPW + o] = v;
        }
    }
    if (last && POOL) {
        __syncthreads();
        for (int o = tid; o < O; o += BC_THREADS) emit_max(g, pl, b, tile, O, o, fmaxf(red[o], red[BC_MAX_FPW + o]));
    }
}

template <bool POOL>
// One binary layer on the int8 matrix cores.  d = the exact integer count, t = fmaf((float)d, a, b).
__device__ __forceinline__ void bin_layer(const ChainArgs& g, const BiPlan& pl, const BiLayer& ly, bool last, const unsigned char* cur,
                                          unsigned char* nxt, int b, int tile, int rows, int wave, int lane) {
    const int r = lane & 31, h = lane >> 5;
    const int O = ly.O, Kp = (ly.K + 31) / 32 * 32, KS = Kp / 32, stride = pl.stride;
    const int8_t* w8 = reinterpret_cast<const int8_t*>(ly.w);
    // The wave's blocks and, inside a block, groups of four k-steps, as ONE sequence q: the four weight fragments of group q + 1 are
    // requested before the sixteen products of group q, so a request flies across them and across a block's epilogue.  A k-step past
    // the layer's (K is rounded to 32, a group to 128) multiplies a zero fragment.
    const int G = (KS + 3) >> 2;
    const int nq = ((O + 31) / 32 - wave + 3) / 4 * G;
    if (nq <= 0) return;
    auto load_group = [&](int q, i32x4 (&f)[4]) {
        const int j = q / G, gi = q - j * G;
        const int8_t* wrow = w8 + (int64_t)((wave + 4 * j) * 32 + r) * Kp + 16 * h;      // (rows up to up32(O) exist: zero filled)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sk = 4 * gi + t;
            const i32x4 v = *reinterpret_cast<const i32x4*>(wrow + 32 * min(sk, KS - 1));
            f[t] = sk < KS ? v : i32x4{0, 0, 0, 0};
        }
    };
    i32x4 bc[4], bn[4];
    load_group(0, bc);
    i32x16 acc[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[rb][i] = 0;
    int gi = 0, ob = wave;
    for (int q = 0; q < nq; ++q) {
        load_group(min(q + 1, nq - 1), bn);                          // unconditional: the last group re-reads its own
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int sk = min(4 * gi + t, KS - 1);
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {                         // (straight line: rows past the cloud are multiplied and never read)
                const i32x4 af = *reinterpret_cast<const i32x4*>(cur + (rb * 32 + r) * stride + 32 * sk + 16 * h);
                acc[rb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af, bc[t], acc[rb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) bc[t] = bn[t];
        if (++gi < G) continue;
        gi = 0;
        const int o = ob * 32 + r;
        const bool oin = o < O;
        const float a = oin ? ly.ab[o] : 0.f, bb = oin ? ly.ab[O + o] : 0.f;
        if (!last) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                if (oin) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        nxt[row * stride + o] = (unsigned char)sgn8(fmaf((float)acc[rb][i], a, bb));
                    }
                }
            }
        } else if (!POOL) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                if (rb * 32 < rows && oin) {
                    float* dst = g.out + ((int64_t)b * O + o) * g.N + (int64_t)tile * BC_ROWS;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (row < rows) dst[row] = clamp1(fmaf((float)acc[rb][i], a, bb), g.clamp);
                    }
                }
            }
        } else {
            int dmax = INT_MIN, dmin = INT_MAX;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                if (rb * 32 < rows) {
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = rb * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        if (row < rows) {                            // rows past the cloud never enter the extreme
                            dmax = max(dmax, acc[rb][i]);
                            dmin = min(dmin, acc[rb][i]);
                        }
                    }
                }
            }
            dmax = max(dmax, (int)lane_half_swap((uint32_t)dmax));
            dmin = min(dmin, (int)lane_half_swap((uint32_t)dmin));
            // (a row 4 h + .. below `rows` exists in one half at least: row 0; a half without one holds the neutral elements)
            if (h == 0 && oin) emit_max(g, pl, b, tile, O, o, fmaf((float)(a < 0.f ? dmin : dmax), a, bb));
        }
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rb][i] = 0;
        ob += 4;
    }
}

template <bool POOL>
__global__ __launch_bounds__(BC_THREADS, 2) void bi_chain_kernel(ChainArgs g, BiPlan pl) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bc_lds[];      // [region 0 | region 1 | red]
    unsigned char* cur = bc_lds;
    unsigned char* nxt = bc_lds + pl.region;
    float* red = reinterpret_cast<float*>(bc_lds + 2 * pl.region);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, b = blockIdx.y;
    const int n0 = tile * BC_ROWS;
    const int rows = min(BC_ROWS, g.N - n0);
    const int C0 = g.C0;
    const float* xb = g.x + (int64_t)b * C0 * g.N + n0;
    const bool floats = g.T != nullptr || pl.first_fp;

    // ---- the x tile, channel-first as it lies: floats [c][row] (rows past the cloud +0), or its signs [row][c]
    for (int e = tid; e < C0 * BC_ROWS; e += BC_THREADS) {
        const int c = e >> 7, row = e & (BC_ROWS - 1);
        const float v = row < rows ? xb[(int64_t)c * g.N + row] : 0.f;
        if (floats) reinterpret_cast<float*>(cur)[e] = v;
        else cur[row * pl.stride + c] = (unsigned char)sgn8(v);
    }
    __syncthreads();
    // ---- the transform, bmm(x^T, T): u[n,j] = +0; c ascending u = fmaf(x[c,n], T[c,j], u)
    if (g.T) {
        const float* xs = reinterpret_cast<const float*>(cur);
        const float* Tb = g.T + (int64_t)b * C0 * C0;
        const int row = tid & (BC_ROWS - 1);
        for (int j = tid >> 7; j < C0; j += 2) {
            float u = 0.f;
            for (int c = 0; c < C0; ++c) u = fmaf(xs[c * BC_ROWS + row], Tb[c * C0 + j], u);
            if (pl.first_fp) reinterpret_cast<float*>(nxt)[j * BC_ROWS + row] = u;
            else nxt[row * pl.stride + j] = (unsigned char)sgn8(u);
        }
        __syncthreads();
        unsigned char* t = cur; cur = nxt; nxt = t;
    }
    // ---- the layers (the plan is a kernel argument: a layer's descriptor is a scalar load at a computed offset)
    for (int l = 0; l < pl.L; ++l) {
        const BiLayer ly = pl.layer[l];
        const bool last = l == pl.L - 1;
        if (l == 0 && pl.first_fp) fp_layer<POOL>(g, pl, ly, last, cur, nxt, red, b, tile, rows, tid);
        else bin_layer<POOL>(g, pl, ly, last, cur, nxt, b, tile, rows, wave, lane);
        if (!last) {
            __syncthreads();
            unsigned char* t = cur; cur = nxt; nxt = t;
        }
    }
}

__global__ __launch_bounds__(256) void bi_chain_finish_kernel(const float* __restrict__ part, int64_t BO, int O, int tiles, float offset,
                                                              float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= BO) return;
    const int64_t b = e / O, o = e - b * O;
    const float* p = part + b * tiles * O + o;
    float m = p[0];
    for (int t = 1; t < tiles; ++t) m = fmaxf(m, p[(int64_t)t * O]);
    out[e] = m + offset;
}

}  // namespace

extern "C" size_t svnet_bi_packed_bytes(int64_t O, int64_t K) {
    return (O >= 1 && K >= 1 && O <= BC_MAX_LAST && K <= BC_MAX_K) ? (size_t)(up32(O) * up32(K)) : 0;
}

extern "C" int svnet_bi_fold_f32(const float* W, const float* scale, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, int64_t O, int64_t K, float eps, int8_t* w_i8, float* s_f32, float* ab, void* stream) {
    SVNET_REQUIRE(W && scale && ab && (w_i8 || s_f32), SVNET_E_ARG, "svnet_bi_fold_f32: null W / scale / ab, or neither w_i8 nor s_f32");
    const bool any = gamma || beta || running_mean || running_var, all = gamma && beta && running_mean && running_var;
    SVNET_REQUIRE(!any || all, SVNET_E_ARG, "svnet_bi_fold_f32: pass gamma, beta, running_mean and running_var, or none of them");
    SVNET_REQUIRE(O >= 1 && K >= 1, SVNET_E_ARG, "svnet_bi_fold_f32: O %lld and K %lld must be positive", (long long)O, (long long)K);
    SVNET_REQUIRE(O * K <= FOLD_MAX_WEIGHTS && (!w_i8 || (O <= BC_MAX_LAST && K <= BC_MAX_K)), SVNET_E_UNSUPPORTED,
                  "svnet_bi_fold_f32: O %lld, K %lld: needs O K <= %d, and O <= %d, K <= %d for the packed form", (long long)O, (long long)K,
                  FOLD_MAX_WEIGHTS, BC_MAX_LAST, BC_MAX_K);
    hipLaunchKernelGGL(bi_fold_kernel, dim3(1), dim3(FOLD_THREADS), 0, (hipStream_t)stream, W, scale, gamma, beta, running_mean, running_var,
                       (int)O, (int)K, eps, w_i8, s_f32, ab);
    SVNET_CHECK_LAUNCH("bi_fold_kernel");
    return SVNET_OK;
}

extern "C" int svnet_bi_chain_supported(int64_t C0, int64_t N, int64_t L, const int64_t* widths, int first_fp, int has_trans) {
    BiPlan pl;
    return bi_plan(C0, N, L, widths, first_fp, has_trans, pl) ? 1 : 0;
}

extern "C" int svnet_bi_chain_rows_tile(void) { return BC_ROWS; }

extern "C" size_t svnet_bi_chain_workspace_bytes(int64_t B, int64_t N, int64_t O) {
    if (B < 1 || B > BC_MAX_B || N < 1 || N > SVNET_KNN_MAX_N || O < 1 || O > BC_MAX_LAST) return 0;
    const int64_t tiles = svnet_cdiv(N, BC_ROWS);
    return tiles > 1 ? (size_t)(B * tiles * O) * sizeof(float) : 0;
}

extern "C" int svnet_bi_chain_f32(const float* x, const float* trans, int64_t B, int64_t C0, int64_t N, int64_t L, const int64_t* widths,
                                  int first_fp, const void* w, const void* ab, int pool, int clamp, float offset, void* workspace,
                                  size_t workspace_bytes, float* out, void* stream) {
    SVNET_REQUIRE(x && widths && w && ab && out, SVNET_E_ARG, "svnet_bi_chain_f32: null x / widths / w / ab / out");
    SVNET_REQUIRE(B >= 1 && B <= BC_MAX_B, SVNET_E_ARG, "svnet_bi_chain_f32: B %lld outside 1 .. %d", (long long)B, BC_MAX_B);
    BiPlan pl;
    SVNET_REQUIRE(bi_plan(C0, N, L, widths, first_fp, trans != nullptr, pl), SVNET_E_UNSUPPORTED,
                  "svnet_bi_chain_f32: C0 %lld, N %lld, L %lld: needs 1 <= N <= %d, 1 <= L <= %d, C0 <= %d with a transform or an fp first layer "
                  "(its width <= %d), every binary input width <= %d, the last width <= %d",
                  (long long)C0, (long long)N, (long long)L, SVNET_KNN_MAX_N, BC_MAX_L, BC_MAX_C0F, BC_MAX_FPW, BC_MAX_K, BC_MAX_LAST);
    const void* const* wl = reinterpret_cast<const void* const*>(w);
    const void* const* abl = reinterpret_cast<const void* const*>(ab);
    int64_t in = C0;
    for (int l = 0; l < (int)L; ++l) {
        SVNET_REQUIRE(wl[l] && abl[l], SVNET_E_ARG, "svnet_bi_chain_f32: null weights or a | b of layer %d", l);
        pl.layer[l] = BiLayer{wl[l], reinterpret_cast<const float*>(abl[l]), (int)in, (int)widths[l]};
        in = widths[l];
    }
    const int64_t O = in;
    const size_t need = pool ? svnet_bi_chain_workspace_bytes(B, N, O) : 0;
    SVNET_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), SVNET_E_ARG,
                  "svnet_bi_chain_f32: the workspace holds %zu bytes, the tiles' partial maxima need %zu", workspace_bytes, need);
    bool ok = true;
    SVNET_LDS_OPTIN(ok, BC_LDS_MAX, "bi_chain_kernel", reinterpret_cast<const void*>(&bi_chain_kernel<false>),
                    reinterpret_cast<const void*>(&bi_chain_kernel<true>));
    if (!ok) return SVNET_E_LAUNCH;
    const ChainArgs g{x, trans, (int)C0, (int)N, pool ? 1 : 0, clamp ? 1 : 0, offset, reinterpret_cast<float*>(workspace), out};
    if (pool) hipLaunchKernelGGL(bi_chain_kernel<true>, dim3((unsigned)pl.tiles, (unsigned)B), dim3(BC_THREADS), (size_t)pl.lds, (hipStream_t)stream, g, pl);
    else hipLaunchKernelGGL(bi_chain_kernel<false>, dim3((unsigned)pl.tiles, (unsigned)B), dim3(BC_THREADS), (size_t)pl.lds, (hipStream_t)stream, g, pl);
    SVNET_CHECK_LAUNCH("bi_chain_kernel");
    if (pool && pl.tiles > 1) {
        hipLaunchKernelGGL(bi_chain_finish_kernel, dim3((unsigned)svnet_cdiv(B * O, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float*>(workspace), B * O, (int)O, pl.tiles, offset, out);
        SVNET_CHECK_LAUNCH("bi_chain_finish_kernel");
    }
    return SVNET_OK;
}
