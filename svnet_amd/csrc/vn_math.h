// The arithmetic of a vector-neuron level (VNLinearLeakyReLU in eval mode, models/vn_layers.py:50-78), element by element: the ONE
// statement of its fp32 sequence.  vn_edge.hip, vn_edge2.hip, vn_cross.hip and vn_tail.hip walk their own layouts and call these, so the levels and the tail
// agree bit for bit by construction; nothing here knows a layout, a tiling or a launch geometry.  The contract in prose is in
// svnet_amd/vn_fused.py; tests/vn_ref.py restates it.  Every file that includes this (Makefile, NO_CONTRACT) is
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

// ---- p [3] of one (point or edge, channel) -> u [3]: the norm through BatchNorm's folded affine.  A VNLinear followed by a VNBatchNorm
// (the norm-only point layer of vn_tail.hip) ends here.
__device__ __forceinline__ void vn_norm(float p0, float p1, float p2, float so, float to, float (&u)[3]) {
    const float q = fmaf(p2, p2, fmaf(p1, p1, p0 * p0));
    const float r = sqrtf(q) + VN_EPS;
    const float g = fmaf(r, so, to) / r;
    u[0] = p0 * g;
    u[1] = p1 * g;
    u[2] = p2 * g;
}

// ---- u (the normed p), d [3] -> y [3]: the leaky rule
__device__ __forceinline__ void vn_leaky(float u0, float u1, float u2, float d0, float d1, float d2, float slope, float one_minus, float (&y)[3]) {
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

// ---- p, d [3] of one (point or edge, channel) -> y [3]: the two halves in order
__device__ __forceinline__ void vn_norm_leaky(float p0, float p1, float p2, float d0, float d1, float d2, float so, float to, float slope,
                                              float one_minus, float (&y)[3]) {
    float u[3];
    vn_norm(p0, p1, p2, so, to, u);
    vn_leaky(u[0], u[1], u[2], d0, d1, d2, slope, one_minus, y);
}
