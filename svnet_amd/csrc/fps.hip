// Farthest point sampling (models/utils/pointnet_util.py:63-84 farthest_point_sample) and the gather + pc_normalize (data.py:15-20) that
// data.py:203-256 ModelNet40_v2(uniform=True) applies to the selection: what turns a pool of ~10 000-point clouds into the
// [M,num_points,3] pool a BatchLoader takes, without leaving the device.
//
// The sampler's result is a list of integer indices fixed by the fp32 rounding sequence and a tie rule (the derivation is in
// svnet_amd/data.py's docstring, tests/fps_ref.py restates it independently):
//   mind[p] = fp32(1e10);  f = start
//   npoint times:  idx[i] = f;  d_c = fl(x[p,c] - x[f,c]);  dist = sq_len(d_0, d_1, d_2)   (pointset.h: the distance, single-rounded);
//                  mind[p] = dist < mind[p] ? dist : mind[p];  f = the SMALLEST p with mind[p] == max mind
//
// Shape of the sampler: one workgroup per cloud, grid M.  Thread t keeps points p = j T + t (j = 0 .. PPL-1) and their mind in
// registers for the whole loop; the loop is npoint DEPENDENT iterations, so the workgroup is sized for the shortest iteration, not for
// occupancy.  One iteration: (1) the new centroid's three coordinates, read at a wave-uniform address from the cloud's copy in LDS
// (tiers 0-3) or from global memory (tier 4: 16384 x 12 B do not fit); (2) PPL updates of mind and the lane's best (value, j);
// (3) an argmax butterfly over the wave (argmax_group, wave.h: no LDS); (4) lane 0 of every wave puts the wave's best
// into one of TWO sets of LDS slots, ONE barrier, every wave reads the W slots (lane l reads slot l % W) and runs the butterfly over
// them.  Writing set i & 1 in iteration i needs no second barrier: whoever writes set b again in iteration i + 2 has passed the
// barrier of iteration i + 1, which every thread reaches only after its read of iteration i.
// Every comparison is on (value, global index) and prefers the lower index on equal values: a lane walks its points in ascending
// index order with a strict >, the butterflies compare the pair.  Padding points (p >= P) carry mind = -1 and coordinates 0: their
// distance is >= 0, so they stay at -1, below every real point's mind >= 0.
#include "pointset.h"

namespace {

constexpr int64_t FPS_MAX_P = 16384;
constexpr float FPS_FAR = 1e10f;            // pointnet_util.py:74
constexpr float FPS_PAD = -1.f;

// tier -> (threads, points per lane, cloud in LDS); a P takes the first tier whose threads x points per lane covers it
constexpr int FPS_TIERS = 5;
constexpr int FPS_THREADS[FPS_TIERS] = {64, 256, 1024, 1024, 1024};
constexpr int FPS_PPL[FPS_TIERS] = {1, 4, 4, 10, 16};

struct FpsSlot { float v; int i; };

template <int T, int PPL, bool LDS_XYZ>
__global__ __launch_bounds__(T) void fps_kernel(const float* __restrict__ xyz, int64_t P, int64_t npoint,
                                                const int64_t* __restrict__ start, int64_t* __restrict__ idx) {
    constexpr int W = T / SVNET_WAVE;
    extern __shared__ __align__(16) unsigned char fps_lds[];
    FpsSlot* slots = reinterpret_cast<FpsSlot*>(fps_lds);                      // [2][W]
    float* cloud = reinterpret_cast<float*>(fps_lds + 2 * W * sizeof(FpsSlot));    // [P][3] when LDS_XYZ
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m = blockIdx.x;
    const float* src = xyz + m * P * 3;
    int64_t* out = idx + m * npoint;

    float x[PPL], y[PPL], z[PPL], mind[PPL];
#pragma unroll
    for (int j = 0; j < PPL; ++j) {
        const int p = j * T + t;
        const bool real = p < P;
        x[j] = real ? src[(int64_t)p * 3 + 0] : 0.f;
        y[j] = real ? src[(int64_t)p * 3 + 1] : 0.f;
        z[j] = real ? src[(int64_t)p * 3 + 2] : 0.f;
        mind[j] = real ? FPS_FAR : FPS_PAD;
    }
    if (LDS_XYZ) {
        for (int q = t; q < (int)P * 3; q += T) cloud[q] = src[q];
        __syncthreads();
    }

    // a start outside the cloud is clamped into it (the Python front end refuses it; here it must only never index past the cloud)
    int64_t s = start[m];
    s = s < 0 ? 0 : s >= P ? P - 1 : s;
    int f = (int)s;
    for (int64_t i = 0; i < npoint; ++i) {
        if (t == 0) out[i] = f;
        if (i + 1 == npoint) break;
        float cx, cy, cz;
        if (LDS_XYZ) {
            cx = cloud[f * 3 + 0]; cy = cloud[f * 3 + 1]; cz = cloud[f * 3 + 2];
        } else {
            cx = src[(int64_t)f * 3 + 0]; cy = src[(int64_t)f * 3 + 1]; cz = src[(int64_t)f * 3 + 2];
        }
        float bv = FPS_PAD - 1.f;
        int bj = 0;
#pragma unroll
        for (int j = 0; j < PPL; ++j) {
            const float d0 = x[j] - cx, d1 = y[j] - cy, d2 = z[j] - cz;
            const float dist = sq_len(d0, d1, d2);
            mind[j] = dist < mind[j] ? dist : mind[j];
            if (mind[j] > bv) { bv = mind[j]; bj = j; }
        }
        int bi = bj * T + t;
        argmax_group<64>(bv, bi, lane);
        if (W > 1) {
            FpsSlot* set = slots + (i & 1) * W;
            if (lane == 0) set[wave] = FpsSlot{bv, bi};
            __syncthreads();
            const FpsSlot r = set[lane & (W - 1)];
            bv = r.v;
            bi = r.i;
            argmax_group<W>(bv, bi, lane);
        }
        f = __builtin_amdgcn_readfirstlane(bi);
    }
}

constexpr int GATHER_THREADS = 256;

// out[m,n,:] = data[m, idx[m,n], :] (+ seg), one workgroup per cloud; with `normalize` the pc_normalize of the selection:
//   c = fp32(float64 mean), the sum in a FIXED order: thread t adds its points n = t, t + 256, .. in ascending order to 0.0, the 64
//       partials of a wave are combined by the xor butterfly 32, 16, .. 1, the four wave sums as ((w0 + w1) + w2) + w3, then / N
//   d = fl(p - c);  m = sqrt(max_n sq_len(d0, d1, d2)) (sqrt is monotone: the max of the roots);  out = fl(d / m)
// An index outside 0 .. P-1 reads nothing: its row is NaN and its seg -1 (and, normalised, so is the whole cloud).
__global__ __launch_bounds__(GATHER_THREADS) void pool_gather_kernel(const float* __restrict__ data, const int64_t* __restrict__ seg,
                                                                     const int64_t* __restrict__ idx, int64_t P, int64_t N, int normalize,
                                                                     float* __restrict__ out, int64_t* __restrict__ seg_out) {
    constexpr int W = GATHER_THREADS / SVNET_WAVE;
    __shared__ double wsum[3][W];
    __shared__ float wmax[W];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t m = blockIdx.x;
    const float* src = data + m * P * 3;
    const int64_t* id = idx + m * N;
    float* dst = out + m * N * 3;

    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (normalize) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int64_t n = t; n < N; n += GATHER_THREADS) {
            const int64_t p = id[n];
            const bool ok = p >= 0 && p < P;
            s0 += ok ? (double)src[p * 3 + 0] : (double)SVNET_QNAN;
            s1 += ok ? (double)src[p * 3 + 1] : (double)SVNET_QNAN;
            s2 += ok ? (double)src[p * 3 + 2] : (double)SVNET_QNAN;
        }
        s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
        if (lane == 0) { wsum[0][wave] = s0; wsum[1][wave] = s1; wsum[2][wave] = s2; }
        __syncthreads();
        const double n_ = (double)N;
        c0 = (float)((((wsum[0][0] + wsum[0][1]) + wsum[0][2]) + wsum[0][3]) / n_);
        c1 = (float)((((wsum[1][0] + wsum[1][1]) + wsum[1][2]) + wsum[1][3]) / n_);
        c2 = (float)((((wsum[2][0] + wsum[2][1]) + wsum[2][2]) + wsum[2][3]) / n_);
    }
    float scale = 1.f;
    if (normalize) {
        float r2 = 0.f;                                         // every squared norm is >= 0 (or NaN, which the max below keeps)
        bool bad = false;
        for (int64_t n = t; n < N; n += GATHER_THREADS) {
            const int64_t p = id[n];
            if (p >= 0 && p < P) {
                const float d0 = src[p * 3 + 0] - c0, d1 = src[p * 3 + 1] - c1, d2 = src[p * 3 + 2] - c2;
                const float q = sq_len(d0, d1, d2);
                r2 = q > r2 ? q : r2;
            } else {
                bad = true;
            }
        }
        if (bad) r2 = SVNET_QNAN;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(r2, off, 64);
            r2 = (o > r2 || o != o) ? o : r2;
        }
        if (lane == 0) wmax[wave] = r2;
        __syncthreads();
        r2 = wmax[0];
#pragma unroll
        for (int w = 1; w < W; ++w) r2 = (wmax[w] > r2 || wmax[w] != wmax[w]) ? wmax[w] : r2;
        scale = sqrtf(r2);
    }
    for (int64_t n = t; n < N; n += GATHER_THREADS) {
        const int64_t p = id[n];
        float v0 = SVNET_QNAN, v1 = SVNET_QNAN, v2 = SVNET_QNAN;
        int64_t sg = -1;
        if (p >= 0 && p < P) {
            v0 = src[p * 3 + 0]; v1 = src[p * 3 + 1]; v2 = src[p * 3 + 2];
            if (normalize) {
                v0 = (v0 - c0) / scale;
                v1 = (v1 - c1) / scale;
                v2 = (v2 - c2) / scale;
            }
            if (seg_out) sg = seg[m * P + p];
        }
        dst[n * 3 + 0] = v0;
        dst[n * 3 + 1] = v1;
        dst[n * 3 + 2] = v2;
        if (seg_out) seg_out[m * N + n] = sg;
    }
}

// out[m,n,:] = attr[m, idx[m,n], :] for rows of A floats: one thread per output float, GATHER_THREADS consecutive floats of a cloud's
// [N,A] block per workgroup (cloud_grid: cloud-major), so the stores are coalesced and the A threads of a row read A consecutive
// floats through one index.  A pure copy: the bits of the pool.  An index outside 0 .. P-1 reads nothing and gives NaN.
__global__ __launch_bounds__(GATHER_THREADS) void pool_gather_attr_kernel(const float* __restrict__ attr, const int64_t* __restrict__ idx,
                                                                          int64_t P, int64_t N, uint32_t A, uint32_t chunks,
                                                                          float* __restrict__ out) {
    const int64_t m = blockIdx.x / chunks;
    const uint32_t e = (blockIdx.x % chunks) * (uint32_t)GATHER_THREADS + threadIdx.x;         // element of the cloud's [N,A] block
    if (e >= (uint32_t)N * A) return;
    const uint32_t n = e / A, c = e - n * A;
    const int64_t p = idx[m * N + n];
    out[m * N * A + e] = p >= 0 && p < P ? attr[(m * P + p) * A + c] : SVNET_QNAN;
}

static size_t fps_lds_bytes(int tier, int64_t P) {
    const size_t slots = 2 * (size_t)(FPS_THREADS[tier] / SVNET_WAVE) * sizeof(FpsSlot);
    return slots + (tier < 4 ? (size_t)P * 3 * sizeof(float) : 0);
}

template <int T, int PPL, bool LDS_XYZ>
static void fps_launch(const float* xyz, int64_t M, int64_t P, int64_t npoint, const int64_t* start, int64_t* idx, size_t lds,
                       hipStream_t stream) {
    hipLaunchKernelGGL((fps_kernel<T, PPL, LDS_XYZ>), dim3((unsigned)M), dim3(T), lds, stream, xyz, P, npoint, start, idx);
}

}  // namespace

extern "C" int svnet_fps_tier(int64_t P) {
    if (P < 1 || P > FPS_MAX_P) return -1;
    for (int tier = 0; tier < FPS_TIERS; ++tier)
        if (P <= (int64_t)FPS_THREADS[tier] * FPS_PPL[tier]) return tier;
    return -1;
}

extern "C" int svnet_fps_supported(int64_t P, int64_t npoint) {
    return svnet_fps_tier(P) >= 0 && npoint >= 1 && npoint <= P ? 1 : 0;
}

extern "C" int svnet_fps_f32(const float* xyz, int64_t M, int64_t P, int64_t npoint, const int64_t* start, int64_t* idx, void* stream) {
    SVNET_REQUIRE(xyz && start && idx, SVNET_E_ARG, "svnet_fps_f32: null xyz / start / idx");
    SVNET_REQUIRE(M >= 1 && P >= 1 && npoint >= 1, SVNET_E_ARG, "svnet_fps_f32: M %lld, P %lld, npoint %lld must be positive", (long long)M,
                  (long long)P, (long long)npoint);
    SVNET_REQUIRE(npoint <= P, SVNET_E_ARG, "svnet_fps_f32: npoint %lld > P %lld", (long long)npoint, (long long)P);
    SVNET_REQUIRE(M <= 0x7fffffffll, SVNET_E_ARG, "svnet_fps_f32: M %lld > 2^31 - 1 (one workgroup per cloud)", (long long)M);
    SVNET_REQUIRE(svnet_fps_supported(P, npoint), SVNET_E_UNSUPPORTED, "svnet_fps_f32: P %lld > %lld (a lane keeps at most 16 points)",
                  (long long)P, (long long)FPS_MAX_P);
    const int tier = svnet_fps_tier(P);
    const size_t lds = fps_lds_bytes(tier, P);
    hipStream_t st = (hipStream_t)stream;
    switch (tier) {
        case 0: fps_launch<64, 1, true>(xyz, M, P, npoint, start, idx, lds, st); break;
        case 1: fps_launch<256, 4, true>(xyz, M, P, npoint, start, idx, lds, st); break;
        case 2: fps_launch<1024, 4, true>(xyz, M, P, npoint, start, idx, lds, st); break;
        case 3: {
            // 10240 points x 12 B = 120 KiB: past the 64 KiB a launch gets without an opt-in
            bool ok;
            const void* const kernel = reinterpret_cast<const void*>(&fps_kernel<1024, 10, true>);
            SVNET_LDS_OPTIN(ok, fps_lds_bytes(3, (int64_t)FPS_THREADS[3] * FPS_PPL[3]), "svnet_fps_f32", kernel);
            if (!ok) return SVNET_E_LAUNCH;
            fps_launch<1024, 10, true>(xyz, M, P, npoint, start, idx, lds, st);
            break;
        }
        default: fps_launch<1024, 16, false>(xyz, M, P, npoint, start, idx, lds, st); break;
    }
    SVNET_CHECK_LAUNCH("fps_kernel");
    return SVNET_OK;
}

extern "C" int svnet_pool_gather_f32(const float* data, const int64_t* seg, const int64_t* idx, int64_t M, int64_t P, int64_t N,
                                     int normalize, float* out, int64_t* seg_out, void* stream) {
    SVNET_REQUIRE(data && idx && out, SVNET_E_ARG, "svnet_pool_gather_f32: null data / idx / out");
    SVNET_REQUIRE((seg_out == nullptr) || seg, SVNET_E_ARG, "svnet_pool_gather_f32: seg_out without a seg (null)");
    SVNET_REQUIRE(M >= 1 && P >= 1 && N >= 1, SVNET_E_ARG, "svnet_pool_gather_f32: M %lld, P %lld, N %lld must be positive", (long long)M,
                  (long long)P, (long long)N);
    SVNET_REQUIRE(M <= 0x7fffffffll, SVNET_E_ARG, "svnet_pool_gather_f32: M %lld > 2^31 - 1 (one workgroup per cloud)", (long long)M);
    hipLaunchKernelGGL(pool_gather_kernel, dim3((unsigned)M), dim3(GATHER_THREADS), 0, (hipStream_t)stream, data, seg, idx, P, N,
                       normalize ? 1 : 0, out, seg_out);
    SVNET_CHECK_LAUNCH("pool_gather_kernel");
    return SVNET_OK;
}

extern "C" int svnet_pool_gather_attr_f32(const float* attr, const int64_t* idx, int64_t M, int64_t P, int64_t N, int64_t A, float* out,
                                          void* stream) {
    SVNET_REQUIRE(attr && idx && out, SVNET_E_ARG, "svnet_pool_gather_attr_f32: null attr / idx / out");
    SVNET_REQUIRE(M >= 1 && P >= 1 && N >= 1, SVNET_E_ARG, "svnet_pool_gather_attr_f32: M %lld, P %lld, N %lld must be positive",
                  (long long)M, (long long)P, (long long)N);
    SVNET_REQUIRE(A >= 1 && A <= SVNET_BATCH_MAX_ATTR, SVNET_E_ARG, "svnet_pool_gather_attr_f32: A %lld outside 1 .. %d", (long long)A,
                  SVNET_BATCH_MAX_ATTR);
    SVNET_REQUIRE(N <= 0x7fffffffll / A, SVNET_E_UNSUPPORTED, "svnet_pool_gather_attr_f32: N %lld x A %lld > 2^31 - 1", (long long)N,
                  (long long)A);
    const CloudGrid grid = cloud_grid(M, N * A, GATHER_THREADS);
    SVNET_REQUIRE(grid.blocks > 0, SVNET_E_UNSUPPORTED, "svnet_pool_gather_attr_f32: M %lld x ceil(N A / %d) workgroups > 2^31 - 1",
                  (long long)M, GATHER_THREADS);
    hipLaunchKernelGGL(pool_gather_attr_kernel, dim3((unsigned)grid.blocks), dim3(GATHER_THREADS), 0, (hipStream_t)stream, attr, idx, P, N,
                       (uint32_t)A, (uint32_t)grid.chunks, out);
    SVNET_CHECK_LAUNCH("pool_gather_attr_kernel");
    return SVNET_OK;
}
