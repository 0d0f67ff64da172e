// The arithmetic of a vector-neuron level (VNLinearLeakyReLU in eval mode, models/vn_layers.py:50-78), element by element: the ONE
// statement of its fp32 sequence.  vn_edge.hip and vn_tail.hip walk their own layouts and call these, so the edge levels and the tail
// agree bit for bit by construction; nothing here knows a layout, a tiling or a launch geometry.  The contract in prose is in
// svnet_amd/vn_fused.py; tests/vn_ref.py restates it.  Both files that include this (Makefile, NO_CONTRACT) are
// built with -ffp-contract=off; every operation its own rounding, fmaf where the contract has one.  Internal: not part of the C interface.
#pragma once
#include "pointset.h"

constexpr float VN_EPS = 1e-6f;                   // EPS of models/vn_layers.py:14
constexpr int VN_MAX_N = SVNET_KNN_MAX_N;         // what the two envelopes share: the points of a cloud, and a direction row per
static inline bool vn_dir_rows_ok(int64_t O, int64_t Od) { return Od == O || Od == 1; }      // output channel or one for all

// ---- BatchNorm's running statistics folded into the affine s, t of one channel
__device__ __forceinline__ void vn_bn_fold(float gamma, float beta, float rmean, float rvar, float eps, float& s, float& t) {
    const float invstd = 1.f / sqrtf(rvar + eps);                    // sa_fold_kernel's (sa_fused.hip)
    s = gamma * invstd;
    t = beta - rmean * s;
}

// ---- p, d [3] of one (point or edge, channel) -> y [3]
__device__ __forceinline__ void vn_norm_leaky(float p0, float p1, float p2, float d0, float d1, float d2, float so, float to, float slope,
                                              float one_minus, float (&y)[3]) {
    // the norm through BatchNorm's folded affine
    const float q = fmaf(p2, p2, fmaf(p1, p1, p0 * p0));
    const float r = sqrtf(q) + VN_EPS;
    const float g = fmaf(r, so, to) / r;
    const float u0 = p0 * g, u1 = p1 * g, u2 = p2 * g;
    // the leaky rule
    const float dot = fmaf(u2, d2, fmaf(u1, d1, u0 * d0));
    const float dd = fmaf(d2, d2, fmaf(d1, d1, d0 * d0));
    float w0 = u0, w1 = u1, w2 = u2;
    if (!(dot >= 0.f)) {
        const float c = -(dot / (dd + VN_EPS));
        w0 = fmaf(c, d0, u0);
        w1 = fmaf(c, d1, u1);
        w2 = fmaf(c, d2, u2);
    }
    y[0] = fmaf(slope, u0, one_minus * w0);
    y[1] = fmaf(slope, u1, one_minus * w1);
    y[2] = fmaf(slope, u2, one_minus * w2);
}
