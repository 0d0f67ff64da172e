// Epoch metrics accumulated on the device: what the reference gathers on the host per batch and hands to sklearn / numpy once per
// epoch (main_cls_dgcnn.py:187-251, main_partseg_dgcnn.py:185-279, utils.py:68-91) - predictions, the cal_loss terms, the per-shape
// part IoUs - as counts in a caller-owned state that the host reads ONCE per epoch.
//
//   state (int64 words): conf[C*C] (true x predicted) | rows | invalid | loss_sum (the bits of a float64)
//
// Integers are added with integer atomics (order-independent).  The loss is never added atomically: every workgroup stores ONE
// float64 partial (its waves in a fixed order), and a one-workgroup finishing launch of the same C call adds the partials in a fixed
// order onto loss_sum - the hand-off is a kernel boundary of the stream, and two identical passes give identical bits.
// The per-row loss term is cal_loss's, formed by the functions of smooth_ce.h that the loss kernels (loss.hip) call too.
//
// The prediction of a row is the LOWEST index among its maxima, a NaN counting as the maximum (torch.max(dim) on the CPU).
#include <float.h>

#include "smooth_ce.h"

namespace {

typedef unsigned long long u64;

constexpr int METRICS_THREADS = 256;
constexpr int64_t METRICS_CLS_MAX_BLOCKS = 1024;   // 4 rows per workgroup: more than 4096 rows are walked grid-stride
constexpr int64_t METRICS_LDS_CONF_MAX = 64;       // the workgroup's confusion counts live in LDS up to 64 x 64 (16 KiB)
constexpr int64_t METRICS_MAX_PART = 4096;         // three histograms of num_part counters in LDS
constexpr int METRICS_REG_PART = 64;               // a point's logits are kept in registers up to 64 channels

__device__ __forceinline__ u64* state_rows(u64* state, int64_t C) { return state + C * C; }

// ---- classification: one wave per row
__global__ __launch_bounds__(METRICS_THREADS) void metrics_cls_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                      int64_t count, int64_t C, float eps, u64* __restrict__ state,
                                                                      double* __restrict__ partial) {
    __shared__ double wsum[4];
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const SmoothCe d(eps, C);
    double local = 0.0;
    u64 rows = 0, invalid = 0;
    for (int64_t r = wave; r < count; r += nwaves) {
        const float* row = logits + r * C;
        float best = -FLT_MAX, mx = -FLT_MAX;
        int64_t bi = INT64_MAX;
        for (int64_t c = lane; c < C; c += 64) {
            const float v = row[c];
            mx = fmaxf(mx, v);
            if (bi == INT64_MAX || ranks_before_nan_first(v, c, best, bi)) { best = v; bi = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mx = fmaxf(mx, __shfl_xor(mx, o, 64));
            const float ov = __shfl_xor(best, o, 64);
            const int64_t oi = __shfl_xor(bi, o, 64);
            if (oi != INT64_MAX && (bi == INT64_MAX || ranks_before_nan_first(ov, oi, best, bi))) { best = ov; bi = oi; }
        }
        const int64_t t = target[r];
        if (t < 0 || t >= C) {          // the loader's -1 poison, or anything else outside the classes: indexes nothing
            ++invalid;
            continue;
        }
        float se = 0.f;
        for (int64_t c = lane; c < C; c += 64) se += expf(row[c] - mx);
        se = wave_sum(se);
        const float lse = smooth_ce_lse(se, mx);
        float part = 0.f;
        for (int64_t c = lane; c < C; c += 64) smooth_ce_add(part, d.soft(c, t), smooth_ce_logp(row[c], lse));
        local += (double)wave_sum(part);
        ++rows;
        if (lane == 0) atomicAdd(&state[t * C + bi], (u64)1);
    }
    if (lane == 0) {
        wsum[threadIdx.x >> 6] = local;
        if (rows) atomicAdd(state_rows(state, C), rows);
        if (invalid) atomicAdd(state_rows(state, C) + 1, invalid);
    }
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ---- part segmentation: one thread per point, gridDim.y = the valid clouds, gridDim.x workgroups per cloud
struct SegArgs {
    const float* logits; const int64_t* seg; const int64_t* label; const int64_t* part_start; const int64_t* part_num;
    int64_t P, N, num_cat;
    float eps;
    u64* state; double* partial; unsigned* iu;
    int lds_conf;
};

// REG: the point's P <= METRICS_REG_PART logits are loaded once (coalesced along n, every load independent of the others) and kept in
// registers for the three passes of the loss; otherwise the later passes read them again (the workgroup's slab is cache resident).
template <bool REG>
__global__ __launch_bounds__(METRICS_THREADS) void metrics_seg_kernel(const SegArgs a) {
    extern __shared__ __align__(16) unsigned char metrics_lds[];
    double* wsum = reinterpret_cast<double*>(metrics_lds);                   // [4]
    unsigned* cnt = reinterpret_cast<unsigned*>(wsum + 4);                   // [4]: rows, invalid
    unsigned* hp = cnt + 4;                                                  // [P] points predicted as p
    unsigned* hs = hp + a.P;                                                 // [P] points labelled p
    unsigned* hi = hs + a.P;                                                 // [P] both
    unsigned* lconf = hi + a.P;                                              // [P*P] when lds_conf
    const int t = threadIdx.x, b = blockIdx.y;
    const int P = (int)a.P;
    const int64_t N = a.N, n = (int64_t)blockIdx.x * METRICS_THREADS + t;
    const int nlds = 4 + 3 * P + (a.lds_conf ? P * P : 0);
    for (int i = t; i < nlds; i += METRICS_THREADS) cnt[i] = 0u;
    __syncthreads();

    const SmoothCe d(a.eps, P);
    float term = 0.f;
    bool valid = false, inside = n < N;
    if (inside) {
        const float* x = a.logits + (int64_t)b * P * N + n;
        float v[REG ? METRICS_REG_PART : 1];
        float best = 0.f, mx = -FLT_MAX;
        int pred = 0;
        if constexpr (REG) {
#pragma unroll
            for (int c = 0; c < METRICS_REG_PART; ++c)
                if (c < P) v[c] = x[(int64_t)c * N];
#pragma unroll
            for (int c = 0; c < METRICS_REG_PART; ++c)
                if (c < P) {
                    const float w = v[c];
                    mx = fmaxf(mx, w);
                    if (c == 0 || ranks_before_nan_first(w, c, best, pred)) { best = w; pred = c; }
                }
        } else {
            for (int c = 0; c < P; ++c) {
                const float w = x[(int64_t)c * N];
                mx = fmaxf(mx, w);
                if (c == 0 || ranks_before_nan_first(w, c, best, pred)) { best = w; pred = c; }
            }
        }
        atomicAdd(&hp[pred], 1u);
        const int64_t sg = a.seg[(int64_t)b * N + n];
        valid = sg >= 0 && sg < P;
        if (valid) {
            const int s = (int)sg;
            atomicAdd(&hs[s], 1u);
            if (s == pred) atomicAdd(&hi[s], 1u);
            if (a.lds_conf) atomicAdd(&lconf[s * P + pred], 1u);
            else atomicAdd(&a.state[(int64_t)s * P + pred], (u64)1);
            float se = 0.f;
            if constexpr (REG) {
#pragma unroll
                for (int c = 0; c < METRICS_REG_PART; ++c)
                    if (c < P) se += expf(v[c] - mx);
            } else {
                for (int c = 0; c < P; ++c) se += expf(x[(int64_t)c * N] - mx);
            }
            const float lse = smooth_ce_lse(se, mx);
            if constexpr (REG) {
#pragma unroll
                for (int c = 0; c < METRICS_REG_PART; ++c)
                    if (c < P) smooth_ce_add(term, d.soft(c, s), smooth_ce_logp(v[c], lse));
            } else {
                for (int c = 0; c < P; ++c) smooth_ce_add(term, d.soft(c, s), smooth_ce_logp(x[(int64_t)c * N], lse));
            }
        }
    }
    const double wl = wave_sum((double)term);
    const u64 vmask = __ballot(valid), imask = __ballot(inside && !valid);
    if ((t & 63) == 0) {
        wsum[t >> 6] = wl;
        if (vmask) atomicAdd(&cnt[0], (unsigned)__popcll(vmask));
        if (imask) atomicAdd(&cnt[1], (unsigned)__popcll(imask));
    }
    __syncthreads();
    if (t == 0) {
        a.partial[(int64_t)b * gridDim.x + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        if (cnt[0]) atomicAdd(state_rows(a.state, P), (u64)cnt[0]);
        if (cnt[1]) atomicAdd(state_rows(a.state, P) + 1, (u64)cnt[1]);
    }
    if (a.lds_conf)
        for (int e = t; e < P * P; e += METRICS_THREADS)
            if (lconf[e]) atomicAdd(&a.state[e], (u64)lconf[e]);
    // the cloud's intersection / union counts of its category's parts: integers, added to the per-cloud scratch
    const int64_t lab = a.label[b];
    if (lab >= 0 && lab < a.num_cat) {
        const int64_t ps = a.part_start[lab], pn = a.part_num[lab];
        if (ps >= 0 && pn >= 1 && ps <= P - pn) {
            unsigned* iu = a.iu + (int64_t)b * 2 * P;
            for (int p = (int)ps + t; p < (int)(ps + pn); p += METRICS_THREADS) {
                const unsigned I = hi[p], U = hp[p] + hs[p] - I;
                if (I) atomicAdd(&iu[p], I);
                if (U) atomicAdd(&iu[P + p], U);
            }
        }
    }
}

// One workgroup behind the counting launch: loss_sum += the partials (fixed order), and for the seg form the shape IoU of every
// valid cloud (utils.py:68-91: part IoU 1 when the union is empty, the mean over the category's parts summed in ascending part order).
__global__ __launch_bounds__(METRICS_THREADS) void metrics_finish_kernel(const double* __restrict__ partial, int64_t npartial,
                                                                         u64* __restrict__ state, int64_t C, const unsigned* __restrict__ iu,
                                                                         const int64_t* __restrict__ label, const int64_t* __restrict__ part_start,
                                                                         const int64_t* __restrict__ part_num, int64_t num_cat, int64_t count,
                                                                         int64_t first, double* __restrict__ shape_iou,
                                                                         int64_t* __restrict__ shape_cat) {
    __shared__ double red[METRICS_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = t; i < npartial; i += METRICS_THREADS) s += partial[i];
    red[t] = s;
    __syncthreads();
    for (int w = METRICS_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) {
        double* loss_sum = reinterpret_cast<double*>(state_rows(state, C) + 2);
        *loss_sum += red[0];
    }
    if (!iu) return;
    for (int64_t b = t; b < count; b += METRICS_THREADS) {
        const int64_t lab = label[b];
        double iou = __longlong_as_double(0x7ff8000000000000ll);
        int64_t cat = SVNET_METRICS_CAT_INVALID;
        if (lab >= 0 && lab < num_cat) {
            const int64_t ps = part_start[lab], pn = part_num[lab];
            if (ps >= 0 && pn >= 1 && ps <= C - pn) {
                const unsigned* cu = iu + b * 2 * C;
                double sum = 0.0;
                for (int64_t p = ps; p < ps + pn; ++p) {
                    const unsigned I = cu[p], U = cu[C + p];
                    sum += U == 0u ? 1.0 : (double)I / (double)U;
                }
                iou = sum / (double)pn;
                cat = lab;
            }
        }
        shape_iou[first + b] = iou;
        shape_cat[first + b] = cat;
    }
}

__global__ __launch_bounds__(METRICS_THREADS) void metrics_reset_kernel(u64* __restrict__ state, int64_t words, double* __restrict__ shape_iou,
                                                                        int64_t* __restrict__ shape_cat, int64_t capacity) {
    const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = i0; i < words; i += step) state[i] = 0;
    for (int64_t i = i0; i < capacity; i += step) {
        shape_iou[i] = __longlong_as_double(0x7ff8000000000000ll);
        shape_cat[i] = SVNET_METRICS_CAT_EMPTY;
    }
}

static inline int64_t cls_blocks(int64_t rows) {
    const int64_t b = svnet_cdiv(rows, 4);
    return b < 1 ? 1 : b > METRICS_CLS_MAX_BLOCKS ? METRICS_CLS_MAX_BLOCKS : b;
}
static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t svnet_metrics_state_bytes(int64_t C) {
    return C < 2 ? 0 : (size_t)(C * C + 3) * 8;
}

extern "C" size_t svnet_metrics_workspace_bytes(int64_t B, int64_t C, int64_t N) {
    if (B < 1 || C < 2 || N < 0) return 0;
    if (N == 0) return align16((size_t)cls_blocks(B) * sizeof(double));
    return align16((size_t)B * (size_t)svnet_cdiv(N, METRICS_THREADS) * sizeof(double)) + (size_t)B * 2 * (size_t)C * sizeof(unsigned);
}

extern "C" int svnet_metrics_reset(void* state, int64_t C, double* shape_iou, int64_t* shape_cat, int64_t capacity, void* stream) {
    SVNET_REQUIRE(state, SVNET_E_ARG, "svnet_metrics_reset: null state");
    SVNET_REQUIRE(C >= 2, SVNET_E_ARG, "svnet_metrics_reset: C %lld < 2", (long long)C);
    SVNET_REQUIRE(capacity >= 0 && (capacity == 0 || (shape_iou && shape_cat)), SVNET_E_ARG,
                  "svnet_metrics_reset: capacity %lld with null shape_iou / shape_cat", (long long)capacity);
    const int64_t words = C * C + 3;
    hipLaunchKernelGGL(metrics_reset_kernel, dim3(svnet_grid(words > capacity ? words : capacity, METRICS_THREADS, 256)),
                       dim3(METRICS_THREADS), 0, (hipStream_t)stream, (u64*)state, words, shape_iou, shape_cat, capacity);
    SVNET_CHECK_LAUNCH("metrics_reset_kernel");
    return SVNET_OK;
}

extern "C" int svnet_metrics_cls_f32(const float* logits, const int64_t* target, int64_t R, int64_t C, int64_t count, float eps,
                                     void* state, void* workspace, size_t workspace_bytes, void* stream) {
    SVNET_REQUIRE(logits && target && state, SVNET_E_ARG, "svnet_metrics_cls_f32: null logits / target / state");
    SVNET_REQUIRE(R >= 1 && C >= 2, SVNET_E_ARG, "svnet_metrics_cls_f32: R %lld < 1 or C %lld < 2", (long long)R, (long long)C);
    SVNET_REQUIRE(count >= 0 && count <= R, SVNET_E_ARG, "svnet_metrics_cls_f32: count %lld outside 0 .. R = %lld", (long long)count,
                  (long long)R);
    SVNET_REQUIRE(eps >= 0.f && eps < 1.f, SVNET_E_ARG, "svnet_metrics_cls_f32: eps %g outside [0, 1)", (double)eps);
    SVNET_REQUIRE(workspace && workspace_bytes >= svnet_metrics_workspace_bytes(R, C, 0), SVNET_E_WORKSPACE,
                  "svnet_metrics_cls_f32: workspace of %zu bytes required", svnet_metrics_workspace_bytes(R, C, 0));
    if (count == 0) return SVNET_OK;
    const int64_t blocks = cls_blocks(count);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(metrics_cls_kernel, dim3((unsigned)blocks), dim3(METRICS_THREADS), 0, st, logits, target, count, C, eps,
                       (u64*)state, (double*)workspace);
    SVNET_CHECK_LAUNCH("metrics_cls_kernel");
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(METRICS_THREADS), 0, st, (const double*)workspace, blocks, (u64*)state, C,
                       (const unsigned*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, (const int64_t*)nullptr, (int64_t)0,
                       (int64_t)0, (int64_t)0, (double*)nullptr, (int64_t*)nullptr);
    SVNET_CHECK_LAUNCH("metrics_finish_kernel");
    return SVNET_OK;
}

extern "C" int svnet_metrics_seg_f32(const float* logits, const int64_t* seg, const int64_t* label, int64_t B, int64_t num_part,
                                     int64_t N, const int64_t* part_start, const int64_t* part_num, int64_t num_cat, int64_t count,
                                     int64_t first, float eps, void* state, double* shape_iou, int64_t* shape_cat, int64_t capacity,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    SVNET_REQUIRE(logits && seg && label && part_start && part_num && state && shape_iou && shape_cat, SVNET_E_ARG,
                  "svnet_metrics_seg_f32: null logits / seg / label / part_start / part_num / state / shape_iou / shape_cat");
    SVNET_REQUIRE(B >= 1 && num_part >= 2 && N >= 1 && num_cat >= 1, SVNET_E_ARG,
                  "svnet_metrics_seg_f32: B %lld, num_part %lld, N %lld, num_cat %lld", (long long)B, (long long)num_part, (long long)N,
                  (long long)num_cat);
    SVNET_REQUIRE(count >= 0 && count <= B, SVNET_E_ARG, "svnet_metrics_seg_f32: count %lld outside 0 .. B = %lld", (long long)count,
                  (long long)B);
    SVNET_REQUIRE(first >= 0 && capacity >= 0, SVNET_E_ARG, "svnet_metrics_seg_f32: first %lld or capacity %lld negative", (long long)first,
                  (long long)capacity);
    SVNET_REQUIRE(eps >= 0.f && eps < 1.f, SVNET_E_ARG, "svnet_metrics_seg_f32: eps %g outside [0, 1)", (double)eps);
    SVNET_REQUIRE(first <= capacity - count, SVNET_E_UNSUPPORTED, "svnet_metrics_seg_f32: first %lld + count %lld > capacity %lld",
                  (long long)first, (long long)count, (long long)capacity);
    SVNET_REQUIRE(num_part <= METRICS_MAX_PART && B <= 65535 && N <= (int64_t)1 << 31, SVNET_E_UNSUPPORTED,
                  "svnet_metrics_seg_f32: num_part %lld > %lld, B %lld > 65535 or N %lld > 2^31", (long long)num_part,
                  (long long)METRICS_MAX_PART, (long long)B, (long long)N);
    SVNET_REQUIRE(workspace && workspace_bytes >= svnet_metrics_workspace_bytes(B, num_part, N), SVNET_E_WORKSPACE,
                  "svnet_metrics_seg_f32: workspace of %zu bytes required", svnet_metrics_workspace_bytes(B, num_part, N));
    if (count == 0) return SVNET_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t chunks = svnet_cdiv(N, METRICS_THREADS);
    SegArgs a;
    a.logits = logits; a.seg = seg; a.label = label; a.part_start = part_start; a.part_num = part_num;
    a.P = num_part; a.N = N; a.num_cat = num_cat; a.eps = eps;
    a.state = (u64*)state;
    a.partial = (double*)workspace;
    a.iu = reinterpret_cast<unsigned*>((char*)workspace + align16((size_t)B * (size_t)chunks * sizeof(double)));
    a.lds_conf = num_part <= METRICS_LDS_CONF_MAX ? 1 : 0;
    // the per-cloud counts are added to by every workgroup of the cloud: zero before the launch, on the stream
    if (hipMemsetAsync(a.iu, 0, (size_t)count * 2 * (size_t)num_part * sizeof(unsigned), st) != hipSuccess) {
        svnet_set_error("svnet_metrics_seg_f32: hipMemsetAsync of the per-cloud counts failed");
        return SVNET_E_LAUNCH;
    }
    const size_t lds = 4 * sizeof(double) + (size_t)(4 + 3 * num_part + (a.lds_conf ? num_part * num_part : 0)) * sizeof(unsigned);
    const dim3 grid((unsigned)chunks, (unsigned)count);
    if (num_part <= METRICS_REG_PART) hipLaunchKernelGGL(metrics_seg_kernel<true>, grid, dim3(METRICS_THREADS), lds, st, a);
    else hipLaunchKernelGGL(metrics_seg_kernel<false>, grid, dim3(METRICS_THREADS), lds, st, a);
    SVNET_CHECK_LAUNCH("metrics_seg_kernel");
    hipLaunchKernelGGL(metrics_finish_kernel, dim3(1), dim3(METRICS_THREADS), 0, st, (const double*)workspace, chunks * count, (u64*)state,
                       num_part, (const unsigned*)a.iu, label, part_start, part_num, num_cat, count, first, shape_iou, shape_cat);
    SVNET_CHECK_LAUNCH("metrics_finish_kernel");
    return SVNET_OK;
}
