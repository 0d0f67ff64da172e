// Label-smoothed cross entropy (cal_loss, utils.py:33-50), element by element: the ONE statement of its fp32 sequence.
//
//   soft_c = 1 - eps at c == target, eps / (C - 1) elsewhere
//   mx = max_c x_c,  se = sum_c expf(x_c - mx),  lse = logf(se) + mx,  logp_c = x_c - lse
//   loss_row = -sum_c soft_c * logp_c,  d loss / d x_c = (expf(logp_c) - soft_c) / rows
//
// Every kernel that forms the loss (loss.hip: cal_loss and both distillation layouts; metrics.hip: both epoch-metrics kernels) walks
// its own layout and calls these for the arithmetic, so the results agree bit for bit by construction: the alpha = 0 distillation
// gradient with cal_loss's, the metrics' loss term with the bound tests/metrics_ref.py derives from this sequence.  Nothing here
// knows a layout, a reduction order or a launch geometry.  Device code only; no file that includes this has a -ffp-contract rule.
#pragma once
#include "common.h"

#ifdef __HIPCC__
// the smoothed target and the row weight, formed on the device (the epoch metrics sum rows and do not use inv_r).  I is the caller's
// class index type - int64_t in the row and channel-major walks, int in metrics_seg_kernel - so no walk pays for a widening.
struct SmoothCe {
    float on, off, inv_r;
    template <typename I>
    __device__ SmoothCe(float eps, I C, I rows = 1) : on(1.f - eps), off(eps / (float)(C - 1)), inv_r(1.f / (float)rows) {}
    // soft target of class c in a row whose target is t: compared, never used as an index
    template <typename I>
    __device__ __forceinline__ float soft(I c, I t) const { return c == t ? on : off; }
};
__device__ __forceinline__ float smooth_ce_lse(float se, float mx) { return logf(se) + mx; }
__device__ __forceinline__ float smooth_ce_logp(float x, float lse) { return x - lse; }
__device__ __forceinline__ void smooth_ce_add(float& part, float soft, float logp) { part -= soft * logp; }
__device__ __forceinline__ float smooth_ce_grad(float logp, float soft) { return expf(logp) - soft; }
#endif
