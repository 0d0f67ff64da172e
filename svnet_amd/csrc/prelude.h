// Point-level prelude shared by the backward of both fused edge layers (edgeblock_bwd.hip, xyzblock.hip):
//   gy[p,o] = Gs * lrelu'(y*) ; red[0:Os] += gy ; red[Os:2Os] += gy * xhat*      (y*, xhat* at the pooled edge)
//   dgate[b,c] += sum_d Gv*(Av*mv + Bv*mvn) ; redv[0:Ov] += Gv*gate*mv ; redv[Ov:2Ov] += Gv*gate*mvn
// A workgroup owns rows_per_block points of ONE cloud; its 256 threads are (row group, channel), partial sums meet in
// LDS and leave as one atomic per output per workgroup (the outputs are shared by the whole grid, and same-address
// float atomics serialise at the memory side).
#pragma once
#include "common.h"

template <typename SelT>
__device__ __forceinline__ void svnet_prelude_body(const float* __restrict__ gs, const float* __restrict__ gv,
                                                   const SelT* __restrict__ sel_max, const SelT* __restrict__ sel_min,
                                                   const float* __restrict__ mv, const float* __restrict__ mvn,
                                                   const float* __restrict__ coef, const float* __restrict__ scale1 /* or null */,
                                                   const float* __restrict__ gate, int64_t P, int64_t N, int Os, int Ov, float slope,
                                                   int64_t rows_per_block, float* __restrict__ gy, float* __restrict__ red,
                                                   float* __restrict__ redv, float* __restrict__ dgate,
                                                   const float* __restrict__ gs2, int64_t gs2_ld, const float* __restrict__ gv2,
                                                   int64_t gv2_ld, float* __restrict__ gv_sum) {
    // Second gradient source (gs2 / gv2, rows of stride gs2_ld / gv2_ld - column slices of the gradient of svcat([x1, .., xn]), read where
    // they lie): the layer's output feeds the next layer AND the concatenation, and autograd used to add the two gradients with a
    // strided elementwise kernel per tensor in front of every layer's backward (and to copy the slice when it was the only one).
    // gs (gv) may be NULL when the concatenation is the only consumer; with two vector sources their sum is left in gv_sum for the
    // kernels that follow.
    __shared__ float lred[2 * 128 + 3 * 64];
    const float* A1 = coef; const float* B1 = coef + Os; const float* MY = coef + 2 * Os; const float* IY = coef + 3 * Os;
    const float* Av = coef + 4 * Os; const float* Bv = Av + Ov;
    const int tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * rows_per_block, p1 = min(P, p0 + rows_per_block);
    const int64_t b = p0 / N;                                   // rows_per_block divides N: one cloud per workgroup
    for (int i = tid; i < 2 * Os + 3 * Ov; i += blockDim.x) lred[i] = 0.f;
    __syncthreads();
    {
        int cw = 32;
        while (cw < Os) cw <<= 1;
        const int o = tid & (cw - 1), rg = tid / cw, RG = blockDim.x / cw;
        if (o < Os) {
            const float a = A1[o], bb = B1[o], sc = scale1 ? scale1[o] : 1.f, my = MY[o], iy = IY[o];
            float r1 = 0.f, r2 = 0.f;
            const SelT* __restrict__ selp = a >= 0.f ? sel_max : sel_min;
            int64_t p = p0 + rg;
            // eight rows' loads in flight per thread (one row at a time was a memory latency per row: 32 in a row at Os = 128)
            for (; p + 7 * RG < p1; p += 8 * RG) {
                float sv[8], gv8[8];
                float g28[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    sv[u] = (float)selp[(p + u * RG) * Os + o];
                    gv8[u] = gs ? gs[(p + u * RG) * Os + o] : 0.f;
                    g28[u] = gs2 ? gs2[(p + u * RG) * gs2_ld + o] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) gv8[u] += g28[u];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const float y = a * sv[u] + bb;
                    const float g = gv8[u] * act_grad(y, 1, slope);
                    gy[(p + u * RG) * Os + o] = g;
                    r1 += g;
                    r2 += g * (sc * sv[u] - my) * iy;
                }
            }
            for (; p < p1; p += RG) {
                const float sel = (float)selp[p * Os + o];
                const float y = a * sel + bb;
                const float g = ((gs ? gs[p * Os + o] : 0.f) + (gs2 ? gs2[p * gs2_ld + o] : 0.f)) * act_grad(y, 1, slope);
                gy[p * Os + o] = g;
                r1 += g;
                r2 += g * (sc * sel - my) * iy;
            }
            atomicAdd(&lred[o], r1);
            atomicAdd(&lred[Os + o], r2);
        }
    }
    {
        int cw = 32;
        while (cw < Ov) cw <<= 1;
        const int c = tid & (cw - 1), rg = tid / cw, RG = blockDim.x / cw;
        if (c < Ov) {
            const float av = Av[c], bv = Bv[c], gt = gate[b * Ov + c];
            float ra = 0.f, rb = 0.f, gsum = 0.f;
            int64_t p = p0 + rg;
            for (; p + 3 * RG < p1; p += 4 * RG) {                   // four rows = 36 loads in flight
                float g4[4][3], h4[4][3], a4[4][3], n4[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        const int64_t q = ((p + u * RG) * 3 + d) * Ov + c;
                        g4[u][d] = gv ? gv[q] : 0.f; a4[u][d] = mv[q]; n4[u][d] = mvn[q];
                        h4[u][d] = gv2 ? gv2[((p + u * RG) * 3 + d) * gv2_ld + c] : 0.f;      // (raw: added after all requests are out)
                    }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int d = 0; d < 3; ++d) g4[u][d] += h4[u][d];
                if (gv_sum) {
#pragma unroll
                    for (int u = 0; u < 4; ++u)
#pragma unroll
                        for (int d = 0; d < 3; ++d) gv_sum[((p + u * RG) * 3 + d) * Ov + c] = g4[u][d];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        gsum += g4[u][d] * (av * a4[u][d] + bv * n4[u][d]);
                        ra += g4[u][d] * gt * a4[u][d];
                        rb += g4[u][d] * gt * n4[u][d];
                    }
            }
            for (; p < p1; p += RG) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const int64_t q = (p * 3 + d) * Ov + c;
                    const float g = (gv ? gv[q] : 0.f) + (gv2 ? gv2[(p * 3 + d) * gv2_ld + c] : 0.f), a = mv[q], n = mvn[q];
                    if (gv_sum) gv_sum[q] = g;
                    gsum += g * (av * a + bv * n);
                    ra += g * gt * a;
                    rb += g * gt * n;
                }
            }
            atomicAdd(&lred[2 * Os + c], ra);
            atomicAdd(&lred[2 * Os + Ov + c], rb);
            atomicAdd(&lred[2 * Os + 2 * Ov + c], gsum);
        }
    }
    __syncthreads();
    // (slices: see SVNET_RED_SLICES in svnet_hip.h - the coeffs kernel adds them up)
    const int slice = (int)(blockIdx.x & (SVNET_RED_SLICES - 1));
    for (int i = tid; i < 2 * Os; i += blockDim.x) atomicAdd(&red[slice * 2 * Os + i], lred[i]);
    for (int i = tid; i < 2 * Ov; i += blockDim.x) atomicAdd(&redv[slice * 2 * Ov + i], lred[2 * Os + i]);
    for (int i = tid; i < Ov; i += blockDim.x) atomicAdd(&dgate[b * Ov + i], lred[2 * Os + 2 * Ov + i]);
}

// rows per workgroup: the largest power of two <= 64 that divides N (a workgroup never spans two clouds)
static inline int64_t svnet_prelude_rows(int64_t N) {
    int64_t r = 64;
    while (r > 1 && N % r != 0) r >>= 1;
    return r;
}
