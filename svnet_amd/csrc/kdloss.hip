// Knowledge distillation (Hinton et al.) fused with the label-smoothed cross entropy of cal_loss (utils.py:33-50): one launch per
// layout reads the student's and the teacher's logits once and writes the loss terms and d L / d student.
//
//   ce_r   = -sum_c soft_rc * log_softmax(s_r)_c            soft_rc = 1 - eps at c == y_r, eps / (C - 1) elsewhere
//   logp_r = log_softmax(t_r / T), logq_r = log_softmax(s_r / T), p = exp(logp)
//   kl_r   = sum_c p_rc * (logp_rc - logq_rc)
//   L      = (1 - alpha) * mean_r ce_r + alpha * T * T * mean_r kl_r
//   dL/ds_rc = [(1 - alpha) * (softmax(s_r)_c - soft_rc) + alpha * T * (exp(logq_rc) - p_rc)] / R
//
// logp and logq are (x - max) / T - log(sum exp((x - max) / T)): a teacher probability that underflows to 0 meets a FINITE
// logp - logq, so its term is 0 and never NaN.  Targets are compared with the class index, never used as one (cal_loss's contract).
//
// rows layout [R,C]:           one wave per row, lanes over classes - smooth_ce_kernel's (pool.hip) walk, grid and partial order; the CE
//                              half of the gradient is computed by the same fp32 sequence, so alpha = 0 reproduces its dlogits bit for bit.
// channel-major layout [B,C,N]: a workgroup of 4 waves owns 64 consecutive points; lane = point (consecutive addresses along N for every
//                              class: each wave-level load and store is one 256-byte run), wave g = classes g, g + 4, g + 8, ...  Up to
//                              KD_CM_REG_CLASSES classes both logit vectors stay in registers between the three passes (max, sums,
//                              gradient) - every byte is read once and written once; past that the passes re-read global memory.
//                              The four waves meet in LDS for the per-point max and sums.  No transposed copy exists anywhere.
//
// Every workgroup stores ONE (ce, kl) pair of partial sums (waves and lanes added in a fixed order) and a one-wave finishing launch of
// the same call adds the pairs in a fixed order: no float atomics, {L, CE, KL} and dlogits are bit-identical from run to run.
#include <float.h>

#include "common.h"

namespace {

constexpr int KD_THREADS = 256;
constexpr int KD_WAVES = KD_THREADS / SVNET_WAVE;
constexpr int64_t KD_ROWS_MAX_BLOCKS = 1024;          // rows layout: 4 rows per workgroup, more than 4096 rows are walked grid-stride
constexpr int64_t KD_CM_MAX_BLOCKS = 4096;            // channel-major: 64 points per workgroup, more than 262 144 points grid-stride
constexpr int KD_CM_CPT = 16;                         // channel-major: classes a thread keeps in registers
constexpr int64_t KD_CM_REG_CLASSES = (int64_t)KD_CM_CPT * KD_WAVES;
constexpr int64_t KD_MAX_C = 65536;
constexpr int64_t KD_MAX_ROWS = 2147483647;           // rows / points (element offsets are 64-bit)
static_assert(2 * KD_CM_MAX_BLOCKS <= SVNET_KD_WORKSPACE_FLOATS && 2 * KD_ROWS_MAX_BLOCKS <= SVNET_KD_WORKSPACE_FLOATS, "workspace");

struct KdScalars {
    float eps;            // label smoothing
    float inv_t;          // 1 / T
    float w_ce, w_kd;     // gradient weights: 1 - alpha, alpha * T
};
// the smoothed target and 1 / rows, formed on the device exactly as smooth_ce_kernel forms them
struct KdDerived {
    float on, off, inv_r;
    __device__ KdDerived(float eps, int64_t C, int64_t rows) : on(1.f - eps), off(eps / (float)(C - 1)), inv_r(1.f / (float)rows) {}
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- rows layout: one wave per row
__global__ __launch_bounds__(KD_THREADS) void kd_rows_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                                                             const int64_t* __restrict__ target, int64_t R, int64_t C, KdScalars k,
                                                             float* __restrict__ partial, float* __restrict__ dlogits) {
    __shared__ float wsum[2][KD_WAVES];
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const KdDerived d(k.eps, C, R);
    float local_ce = 0.f, local_kl = 0.f;
    for (int64_t r = wave; r < R; r += nwaves) {
        const float* srow = student + r * C;
        const float* trow = teacher + r * C;
        float mx = -FLT_MAX, mt = -FLT_MAX;
        for (int64_t c = lane; c < C; c += 64) {
            mx = fmaxf(mx, srow[c]);
            mt = fmaxf(mt, trow[c]);
        }
        mx = wave_max(mx);
        mt = wave_max(mt);
        float se = 0.f, sq = 0.f, sp = 0.f;
        for (int64_t c = lane; c < C; c += 64) {
            const float x = srow[c] - mx;
            se += expf(x);
            sq += expf(x * k.inv_t);
            sp += expf((trow[c] - mt) * k.inv_t);
        }
        se = wave_sum(se);
        sq = wave_sum(sq);
        sp = wave_sum(sp);
        const float lse = logf(se) + mx, lsq = logf(sq), lsp = logf(sp);
        const int64_t t = target[r];
        float part = 0.f, kl = 0.f;
        for (int64_t c = lane; c < C; c += 64) {
            const float x = srow[c];
            const float logp = x - lse;                              // (smooth_ce_kernel's sequence: same bits)
            const float soft = (c == t) ? d.on : d.off;
            part -= soft * logp;
            const float lq = (x - mx) * k.inv_t - lsq;
            const float lp = (trow[c] - mt) * k.inv_t - lsp;
            const float p = expf(lp);
            kl += p * (lp - lq);
            if (dlogits) dlogits[r * C + c] = (k.w_ce * (expf(logp) - soft) + k.w_kd * (expf(lq) - p)) * d.inv_r;
        }
        local_ce += wave_sum(part);
        local_kl += wave_sum(kl);
    }
    if (lane == 0) {
        wsum[0][threadIdx.x >> 6] = local_ce;
        wsum[1][threadIdx.x >> 6] = local_kl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = ((wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3])) * d.inv_r;
        partial[2 * blockIdx.x + 1] = ((wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3])) * d.inv_r;
    }
}

// ---- channel-major layout: lane = point, wave = class residue.  REG: both logit vectors of the thread's classes live in registers.
template <bool REG>
__global__ __launch_bounds__(KD_THREADS) void kd_cm_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                                                           const int64_t* __restrict__ target, int64_t P, int64_t C, int64_t N,
                                                           KdScalars k, float* __restrict__ partial, float* __restrict__ dlogits) {
    __shared__ float red[3][KD_WAVES][SVNET_WAVE];     // per-point partials of the four class residues
    __shared__ float fin[2][KD_WAVES][SVNET_WAVE];
    // (g as a scalar: the class offsets c * N become scalar too - as lane values the REG form held 149 VGPRs of addresses, now 86)
    const int lane = threadIdx.x & 63, g = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t tiles = (P + SVNET_WAVE - 1) / SVNET_WAVE;
    constexpr int CPT = REG ? KD_CM_CPT : 1;
    const KdDerived d(k.eps, C, P);
    float block_ce = 0.f, block_kl = 0.f;              // (thread 0 .. 63 of wave 0 only)
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t p = tile * SVNET_WAVE + lane;
        const bool valid = p < P;
        const int64_t b = valid ? p / N : 0, n = valid ? p - b * N : 0;
        const float* sp_ = student + b * C * N + n;    // class c of this point: + c * N
        const float* tp_ = teacher + b * C * N + n;
        float sv[CPT], tv[CPT];
        float mx = -FLT_MAX, mt = -FLT_MAX;
        if (REG) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int64_t c = g + (int64_t)KD_WAVES * j;
                const bool in = valid && c < C;
                sv[j] = in ? sp_[c * N] : -FLT_MAX;
                tv[j] = in ? tp_[c * N] : -FLT_MAX;
                mx = fmaxf(mx, sv[j]);
                mt = fmaxf(mt, tv[j]);
            }
        } else if (valid) {
            for (int64_t c = g; c < C; c += KD_WAVES) {
                mx = fmaxf(mx, sp_[c * N]);
                mt = fmaxf(mt, tp_[c * N]);
            }
        }
        red[0][g][lane] = mx;
        red[1][g][lane] = mt;
        __syncthreads();
        mx = fmaxf(fmaxf(red[0][0][lane], red[0][1][lane]), fmaxf(red[0][2][lane], red[0][3][lane]));
        mt = fmaxf(fmaxf(red[1][0][lane], red[1][1][lane]), fmaxf(red[1][2][lane], red[1][3][lane]));
        __syncthreads();
        float se = 0.f, sq = 0.f, sp = 0.f;
        if (REG) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                if (valid && g + (int64_t)KD_WAVES * j < C) {
                    const float x = sv[j] - mx;
                    se += expf(x);
                    sq += expf(x * k.inv_t);
                    sp += expf((tv[j] - mt) * k.inv_t);
                }
            }
        } else if (valid) {
            for (int64_t c = g; c < C; c += KD_WAVES) {
                const float x = sp_[c * N] - mx;
                se += expf(x);
                sq += expf(x * k.inv_t);
                sp += expf((tp_[c * N] - mt) * k.inv_t);
            }
        }
        red[0][g][lane] = se;
        red[1][g][lane] = sq;
        red[2][g][lane] = sp;
        __syncthreads();
        se = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
        sq = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
        sp = (red[2][0][lane] + red[2][1][lane]) + (red[2][2][lane] + red[2][3][lane]);
        // (an invalid lane's sums are 0: its logs are never used)
        const float lse = logf(se) + mx, lsq = logf(sq), lsp = logf(sp);
        const int64_t t = valid ? target[p] : -1;
        float part = 0.f, kl = 0.f;
        float* dp_ = dlogits ? dlogits + b * C * N + n : nullptr;
        auto one = [&](int64_t c, float x, float y) {
            const float logp = x - lse;
            const float soft = (c == t) ? d.on : d.off;
            part -= soft * logp;
            const float lq = (x - mx) * k.inv_t - lsq;
            const float lp = (y - mt) * k.inv_t - lsp;
            const float pr = expf(lp);
            kl += pr * (lp - lq);
            if (dp_) dp_[c * N] = (k.w_ce * (expf(logp) - soft) + k.w_kd * (expf(lq) - pr)) * d.inv_r;
        };
        if (REG) {
#pragma unroll
            for (int j = 0; j < CPT; ++j) {
                const int64_t c = g + (int64_t)KD_WAVES * j;
                if (valid && c < C) one(c, sv[j], tv[j]);
            }
        } else if (valid) {
            for (int64_t c = g; c < C; c += KD_WAVES) one(c, sp_[c * N], tp_[c * N]);
        }
        fin[0][g][lane] = part;
        fin[1][g][lane] = kl;
        __syncthreads();                                // (also fences red[] against the next tile's first writes)
        if (g == 0) {
            const float ce_pt = (fin[0][0][lane] + fin[0][1][lane]) + (fin[0][2][lane] + fin[0][3][lane]);
            const float kl_pt = (fin[1][0][lane] + fin[1][1][lane]) + (fin[1][2][lane] + fin[1][3][lane]);
            block_ce += wave_sum(ce_pt);
            block_kl += wave_sum(kl_pt);
        }
        __syncthreads();                                // fin[] is rewritten by the next tile
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = block_ce * d.inv_r;
        partial[2 * blockIdx.x + 1] = block_kl * d.inv_r;
    }
}

// result = {L, CE, KL}: the workgroups' (ce, kl) pairs added in a fixed order
__global__ void kd_finish_kernel(const float* __restrict__ partial, int n, float w_ce, float w_kl, float* __restrict__ result) {
    float ce = 0.f, kl = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) {
        ce += partial[2 * i];
        kl += partial[2 * i + 1];
    }
    ce = wave_sum(ce);
    kl = wave_sum(kl);
    if (threadIdx.x == 0) {
        result[0] = w_ce * ce + w_kl * kl;
        result[1] = ce;
        result[2] = kl;
    }
}

bool kd_rows_of(int layout, int64_t B, int64_t N, int64_t* rows) {
    if (layout == SVNET_KD_ROWS) {
        if (B < 1 || B > KD_MAX_ROWS || N != 1) return false;
        *rows = B;
        return true;
    }
    if (layout != SVNET_KD_CHANNEL_MAJOR || B < 1 || N < 1 || B > KD_MAX_ROWS || N > KD_MAX_ROWS || B > KD_MAX_ROWS / N) return false;
    *rows = B * N;
    return true;
}

}  // namespace

extern "C" int svnet_kd_tier(int layout, int64_t B, int64_t C, int64_t N) {
    int64_t rows = 0;
    if (!kd_rows_of(layout, B, N, &rows) || C < 2 || C > KD_MAX_C) return -1;
    const bool rows_layout = layout == SVNET_KD_ROWS;
    const int many_classes = C > (rows_layout ? (int64_t)SVNET_WAVE : KD_CM_REG_CLASSES) ? 1 : 0;
    const int strided = rows > (rows_layout ? KD_ROWS_MAX_BLOCKS * KD_WAVES : KD_CM_MAX_BLOCKS * SVNET_WAVE) ? 2 : 0;
    return many_classes | strided;
}

extern "C" int svnet_kd_supported(int layout, int64_t B, int64_t C, int64_t N) { return svnet_kd_tier(layout, B, C, N) >= 0 ? 1 : 0; }

extern "C" int svnet_kd_loss_f32(int layout, const float* student, const float* teacher, const int64_t* target, int64_t B, int64_t C,
                                 int64_t N, float eps, float alpha, float T, float* result, float* dlogits, float* workspace,
                                 int64_t workspace_floats, void* stream) {
    SVNET_REQUIRE(student && teacher && target && result, SVNET_E_ARG, "svnet_kd_loss_f32: null pointer");
    SVNET_REQUIRE(T > 0.f && alpha >= 0.f && alpha <= 1.f, SVNET_E_ARG, "svnet_kd_loss_f32: T %g must be > 0 and alpha %g in [0, 1]",
                  (double)T, (double)alpha);
    const int tier = svnet_kd_tier(layout, B, C, N);
    SVNET_REQUIRE(tier >= 0, SVNET_E_UNSUPPORTED,
                  "svnet_kd_loss_f32: layout %d, B %lld, C %lld, N %lld is not taken (layout 0 [R,C]: N = 1; layout 1 [B,C,N]; 2 <= C <= %lld, "
                  "1 <= rows <= %lld)", layout, (long long)B, (long long)C, (long long)N, (long long)KD_MAX_C, (long long)KD_MAX_ROWS);
    SVNET_REQUIRE(workspace && workspace_floats >= SVNET_KD_WORKSPACE_FLOATS, SVNET_E_WORKSPACE,
                  "svnet_kd_loss_f32: workspace of %d floats required", SVNET_KD_WORKSPACE_FLOATS);
    int64_t rows = 0;
    kd_rows_of(layout, B, N, &rows);
    hipStream_t st = (hipStream_t)stream;
    const KdScalars k = {eps, 1.f / T, 1.f - alpha, alpha * T};
    int blocks;
    if (layout == SVNET_KD_ROWS) {
        blocks = (int)svnet_grid(rows * 64, KD_THREADS, KD_ROWS_MAX_BLOCKS);
        hipLaunchKernelGGL(kd_rows_kernel, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, k, workspace, dlogits);
        SVNET_CHECK_LAUNCH("kd_rows_kernel");
    } else {
        blocks = (int)svnet_grid(rows, SVNET_WAVE, KD_CM_MAX_BLOCKS);
        if (tier & 1)
            hipLaunchKernelGGL(kd_cm_kernel<false>, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, N, k, workspace, dlogits);
        else
            hipLaunchKernelGGL(kd_cm_kernel<true>, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, N, k, workspace, dlogits);
        SVNET_CHECK_LAUNCH("kd_cm_kernel");
    }
    hipLaunchKernelGGL(kd_finish_kernel, dim3(1), dim3(64), 0, st, workspace, blocks, 1.f - alpha, alpha * T * T, result);
    SVNET_CHECK_LAUNCH("kd_finish_kernel");
    return SVNET_OK;
}
