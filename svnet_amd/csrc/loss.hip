// The losses: the label-smoothed cross entropy of cal_loss (utils.py:33-50), alone (svnet_smooth_ce_f32) and fused with knowledge
// distillation (Hinton et al., svnet_kd_loss_f32): one launch per layout reads the student's - and the teacher's - logits once and
// writes the loss terms and d L / d student.  The cross entropy's fp32 sequence is smooth_ce.h's, in every kernel here.
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
// rows layout [R,C]:           smooth_ce_kernel<KD>, one wave per row, lanes over classes.  KD = false is cal_loss: no teacher, one
//                              partial per workgroup.  KD = true adds the teacher's sums to the same loops and a second partial; the CE
//                              half of its gradient is the same code, so alpha = 0 reproduces cal_loss's dlogits bit for bit.
// channel-major layout [B,C,N]: a workgroup of 4 waves owns 64 consecutive points; lane = point (consecutive addresses along N for every
//                              class: each wave-level load and store is one 256-byte run), wave g = classes g, g + 4, g + 8, ...  Up to
//                              KD_CM_REG_CLASSES classes both logit vectors stay in registers between the three passes (max, sums,
//                              gradient) - every byte is read once and written once; past that the passes re-read global memory.
//                              The four waves meet in LDS for the per-point max and sums.  No transposed copy exists anywhere.
//
// Every workgroup stores ONE partial sum per loss term (waves and lanes added in a fixed order) and a one-wave finishing launch of
// the same call adds them in a fixed order: no float atomics, the loss, {L, CE, KL} and dlogits are bit-identical from run to run.
#include <float.h>

#include "smooth_ce.h"

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

// ---- rows layout: one wave per row.  KD = false is cal_loss alone: the teacher, its sums, the KL term and the second partial are
// compiled out (teacher is not read, of k only eps).  Every workgroup writes its partial(s) - four waves added in a fixed order.
template <bool KD>
__global__ __launch_bounds__(KD_THREADS) void smooth_ce_kernel(const float* __restrict__ student, const float* __restrict__ teacher,
                                                               const int64_t* __restrict__ target, int64_t R, int64_t C, KdScalars k,
                                                               float* __restrict__ partial, float* __restrict__ dlogits) {
    __shared__ float wsum[KD ? 2 : 1][KD_WAVES];
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const SmoothCe d(k.eps, C, R);
    float local_ce = 0.f, local_kl = 0.f;
    for (int64_t r = wave; r < R; r += nwaves) {
        const float* srow = student + r * C;
        const float* trow = KD ? teacher + r * C : nullptr;
        float mx = -FLT_MAX, mt = -FLT_MAX;
        for (int64_t c = lane; c < C; c += 64) {
            mx = fmaxf(mx, srow[c]);
            if constexpr (KD) mt = fmaxf(mt, trow[c]);
        }
        mx = wave_max(mx);
        if constexpr (KD) mt = wave_max(mt);
        float se = 0.f, sq = 0.f, sp = 0.f;
        for (int64_t c = lane; c < C; c += 64) {
            const float x = srow[c] - mx;
            se += expf(x);
            if constexpr (KD) {
                sq += expf(x * k.inv_t);
                sp += expf((trow[c] - mt) * k.inv_t);
            }
        }
        se = wave_sum(se);
        if constexpr (KD) {
            sq = wave_sum(sq);
            sp = wave_sum(sp);
        }
        const float lse = smooth_ce_lse(se, mx), lsq = KD ? logf(sq) : 0.f, lsp = KD ? logf(sp) : 0.f;
        const int64_t t = target[r];
        float part = 0.f, kl = 0.f;
        for (int64_t c = lane; c < C; c += 64) {
            const float x = srow[c];
            const float logp = smooth_ce_logp(x, lse);
            const float soft = d.soft(c, t);
            smooth_ce_add(part, soft, logp);
            if constexpr (KD) {
                const float lq = (x - mx) * k.inv_t - lsq;
                const float lp = (trow[c] - mt) * k.inv_t - lsp;
                const float p = expf(lp);
                kl += p * (lp - lq);
                if (dlogits) dlogits[r * C + c] = (k.w_ce * smooth_ce_grad(logp, soft) + k.w_kd * (expf(lq) - p)) * d.inv_r;
            } else {
                if (dlogits) dlogits[r * C + c] = smooth_ce_grad(logp, soft) * d.inv_r;
            }
        }
        local_ce += wave_sum(part);
        if constexpr (KD) local_kl += wave_sum(kl);
    }
    if (lane == 0) {
        wsum[0][threadIdx.x >> 6] = local_ce;
        if constexpr (KD) wsum[1][threadIdx.x >> 6] = local_kl;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[(KD ? 2 : 1) * blockIdx.x] = ((wsum[0][0] + wsum[0][1]) + (wsum[0][2] + wsum[0][3])) * d.inv_r;
        if constexpr (KD) partial[2 * blockIdx.x + 1] = ((wsum[1][0] + wsum[1][1]) + (wsum[1][2] + wsum[1][3])) * d.inv_r;
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
    const SmoothCe d(k.eps, C, P);
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
        const float lse = smooth_ce_lse(se, mx), lsq = logf(sq), lsp = logf(sp);
        const int64_t t = valid ? target[p] : -1;
        float part = 0.f, kl = 0.f;
        float* dp_ = dlogits ? dlogits + b * C * N + n : nullptr;
        auto one = [&](int64_t c, float x, float y) {
            const float logp = smooth_ce_logp(x, lse);
            const float soft = d.soft(c, t);
            smooth_ce_add(part, soft, logp);
            const float lq = (x - mx) * k.inv_t - lsq;
            const float lp = (y - mt) * k.inv_t - lsp;
            const float pr = expf(lp);
            kl += pr * (lp - lq);
            if (dp_) dp_[c * N] = (k.w_ce * smooth_ce_grad(logp, soft) + k.w_kd * (expf(lq) - pr)) * d.inv_r;
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

// One wave adds the workgroups' partials in a fixed order.  KD: (ce, kl) pairs, result = {L, CE, KL}; otherwise result[0] = the loss.
template <bool KD>
__global__ void smooth_ce_finish_kernel(const float* __restrict__ partial, int n, float w_ce, float w_kl, float* __restrict__ result) {
    float ce = 0.f, kl = 0.f;
    for (int i = threadIdx.x; i < n; i += 64) {
        ce += partial[KD ? 2 * i : i];
        if constexpr (KD) kl += partial[2 * i + 1];
    }
    ce = wave_sum(ce);
    if constexpr (KD) kl = wave_sum(kl);
    if (threadIdx.x == 0) {
        if constexpr (KD) {
            result[0] = w_ce * ce + w_kl * kl;
            result[1] = ce;
            result[2] = kl;
        } else {
            result[0] = ce;
        }
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

extern "C" int svnet_smooth_ce_f32(const float* logits, const int64_t* target, int64_t R, int64_t C, float eps, float* loss,
                                   float* dlogits, float* workspace, int64_t workspace_floats, void* stream) {
    SVNET_REQUIRE(logits && target && loss && R > 0 && C > 1, SVNET_E_ARG, "svnet_smooth_ce_f32: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const int blocks = svnet_grid(R * 64, KD_THREADS, KD_ROWS_MAX_BLOCKS);
    SVNET_REQUIRE(workspace && workspace_floats >= blocks, SVNET_E_ARG, "svnet_smooth_ce_f32: workspace of 1024 floats required");
    const KdScalars k = {eps, 0.f, 0.f, 0.f};
    hipLaunchKernelGGL(smooth_ce_kernel<false>, dim3(blocks), dim3(KD_THREADS), 0, st, logits, (const float*)nullptr, target, R, C, k,
                       workspace, dlogits);
    SVNET_CHECK_LAUNCH("smooth_ce_kernel<false>");
    hipLaunchKernelGGL(smooth_ce_finish_kernel<false>, dim3(1), dim3(64), 0, st, workspace, blocks, 0.f, 0.f, loss);
    SVNET_CHECK_LAUNCH("smooth_ce_finish_kernel<false>");
    return SVNET_OK;
}

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
        hipLaunchKernelGGL(smooth_ce_kernel<true>, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, k, workspace, dlogits);
        SVNET_CHECK_LAUNCH("smooth_ce_kernel<true>");
    } else {
        blocks = (int)svnet_grid(rows, SVNET_WAVE, KD_CM_MAX_BLOCKS);
        if (tier & 1)
            hipLaunchKernelGGL(kd_cm_kernel<false>, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, N, k, workspace, dlogits);
        else
            hipLaunchKernelGGL(kd_cm_kernel<true>, dim3(blocks), dim3(KD_THREADS), 0, st, student, teacher, target, rows, C, N, k, workspace, dlogits);
        SVNET_CHECK_LAUNCH("kd_cm_kernel");
    }
    hipLaunchKernelGGL(smooth_ce_finish_kernel<true>, dim3(1), dim3(64), 0, st, workspace, blocks, 1.f - alpha, alpha * T * T, result);
    SVNET_CHECK_LAUNCH("smooth_ce_finish_kernel<true>");
    return SVNET_OK;
}
