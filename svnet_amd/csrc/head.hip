// Classifier heads: dense layers over M = batch rows (M <= 64).
//
// Replaces  models/sv_dgcnn_cls.py:76-80 and models/sv_pointnet_cls.py:59-61
//     x = act(bn(linear(x)))  with linear = sv_layers.Linear(bw, ba) (sv_layers.py:35-51), bn = nn.BatchNorm1d, twice, then nn.Linear
// and their autograd.  With 32 rows these layers are a chain of ~25 launch- and latency-bound micro-kernels per step at the very
// end of the forward and the very start of the backward, where nothing else runs beside them (0.3 ms of a 5.4 ms step): here a
// binarized layer + BatchNorm + activation is ONE pass forward (after a packing pass over its input) and TWO passes backward:
//   pack   (wave per 64 input columns)   x + beta -> ternary / STE bit planes, row-major [M][KW] and column words [K] (bit m = row m)
//   fwd    (wave per output channel)     popcount dots of all rows -> y = n * scale -> batch statistics over the wave's lanes
//                                        (lane = row; fp64 sums) -> running statistics -> BatchNorm + activation
//   bwd_w  (workgroup per output channel) BatchNorm/activation backward of the channel (lane = row) -> dL/dy; the channel's
//                                        weight-gradient row GX[o,:] = sum_m dy[m] x_b[m,:] from the column words, STE chain rule to
//                                        (W, scale) - sv_layers.py:44-45 -, dn = dy * scale kept transposed for bwd_x
//   bwd_x  (workgroup per 64 input columns) dx[m,k] = STE[m,k] * sum_o dn[m,o] sign(W[o,k]): the output channels split over the
//                                        workgroup's waves (dn rows through scalar loads, one FMA per row and channel), combined in
//                                        LDS in a fixed order; dL/dbeta[k] = sum_m dx[m,k].  No atomics anywhere: reproducible.
// The fp32 output layer's backward (dx, dW, db of nn.Linear over the same few rows) is one launch (fplinear_small_bwd).
#include "common.h"

namespace {

constexpr int MROWS = 64;          // most rows these kernels take (lane = row)

// ---------------------------------------------------------------------------------------------- pack
// One wave per 64-column word: lane = column.  Row-major words by ballots (lane 0 stores), column words by shifting the lane's
// own bit of every row into place.
__global__ __launch_bounds__(64) void binhead_pack_kernel(const float* __restrict__ x, const float* __restrict__ beta, int M, int K, int KW,
                                                          uint64_t* __restrict__ xs, uint64_t* __restrict__ xz, uint64_t* __restrict__ xt,
                                                          uint64_t* __restrict__ xcs, uint64_t* __restrict__ xcz, uint64_t* __restrict__ xct) {
    const int lane = threadIdx.x, kw = blockIdx.x;
    const int k = kw * 64 + lane;
    const bool in = k < K;
    const int kc = in ? k : K - 1;
    const float b = beta[kc];
    uint32_t cs[2] = {0u, 0u}, cz[2] = {0u, 0u}, ct[2] = {0u, 0u};
    for (int m0 = 0; m0 < M; m0 += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = x[(int64_t)min(m0 + u, M - 1) * K + kc];     // (clamped: every load goes out)
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int m = m0 + u;
            if (m >= M) break;                                                             // (uniform)
            const float tv = in ? v[u] + b : 0.f;
            const bool pos = tv > 0.f, nz = tv != 0.f;
            const bool ste = in && fabsf(tv) <= 1.2f;
            const uint64_t sg = __ballot(pos), zz = __ballot(nz), st = __ballot(ste);
            if (lane == 0) {
                xs[m * KW + kw] = sg;
                xz[m * KW + kw] = zz;
                if (xt) xt[m * KW + kw] = st;
            }
            cs[m >> 5] |= (uint32_t)pos << (m & 31);
            cz[m >> 5] |= (uint32_t)nz << (m & 31);
            ct[m >> 5] |= (uint32_t)ste << (m & 31);
        }
    }
    if (xcs && in) {
        xcs[k] = (uint64_t)cs[0] | ((uint64_t)cs[1] << 32);
        xcz[k] = (uint64_t)cz[0] | ((uint64_t)cz[1] << 32);
        if (xct) xct[k] = (uint64_t)ct[0] | ((uint64_t)ct[1] << 32);
    }
}

// ---------------------------------------------------------------------------------------------- forward
struct HeadFwdArgs {
    const uint64_t* xs; const uint64_t* xz;           // [M][KW]
    const uint64_t* w_sign; const uint64_t* w_nz;     // [O][wld]
    const float* scale; const float* gamma; const float* bn_beta;
    float* rmean; float* rvar; long long* nbt;
    float* y; float* mean; float* invstd; float* out;
    int M, K, KW, O, wld, training, act;
    float eps, momentum, slope;
};

constexpr int FWD_OC = 4;          // output channels per workgroup (one per wave)

__global__ __launch_bounds__(256) void binhead_fwd_kernel(HeadFwdArgs a) {
    extern __shared__ uint64_t lds[];
    const int KW = a.KW, KWP = KW | 1;               // odd row stride (64-bit words): lanes = rows read conflict-free
    uint64_t* lxs = lds;                              // [MROWS][KWP]
    uint64_t* lxz = lds + MROWS * KWP;
    uint64_t* lws = lds + 2 * MROWS * KWP;            // [FWD_OC][KW]
    uint64_t* lwz = lws + FWD_OC * KW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * FWD_OC;
    for (int i = tid; i < MROWS * KW; i += 256) {
        const int m = i / KW, w = i - m * KW;
        const bool ok = m < a.M;
        lxs[m * KWP + w] = ok ? a.xs[i] : 0ull;
        lxz[m * KWP + w] = ok ? a.xz[i] : 0ull;
    }
    for (int i = tid; i < FWD_OC * KW; i += 256) {
        const int ol = i / KW, w = i - ol * KW;
        const int o = min(o0 + ol, a.O - 1);
        lws[i] = a.w_sign[(int64_t)o * a.wld + w];
        lwz[i] = a.w_nz[(int64_t)o * a.wld + w];
    }
    __syncthreads();
    const int o = o0 + wave;
    if (o >= a.O) return;                             // (whole wave)
    const int m = lane;
    const bool row = m < a.M;
    int pm = 0, pd = 0;
    for (int w = 0; w < KW; ++w) {
        const uint64_t mz = lxz[m * KWP + w] & lwz[wave * KW + w];
        pm += __popcll(mz);
        pd += __popcll(mz & (lxs[m * KWP + w] ^ lws[wave * KW + w]));
    }
    const int cnt = pm - 2 * pd;
    const float yv = (float)cnt * a.scale[o] + 0.f;   // (svnet_binlinear_fwd_f32's emit: count * scale + bias, bias = 0)
    float mu, is;
    if (a.training) {
        const double d = row ? (double)yv : 0.0;
        const double s1 = wave_sum(d), s2 = wave_sum(d * d);
        const double mean = s1 / (double)a.M;
        double var = s2 / (double)a.M - mean * mean;
        if (var < 0.0) var = 0.0;
        mu = (float)mean;
        is = (float)(1.0 / sqrt(var + (double)a.eps));
        if (lane == 0) {
            if (a.rmean) a.rmean[o] = (1.f - a.momentum) * a.rmean[o] + a.momentum * mu;
            if (a.rvar) {
                const double unb = (a.M > 1) ? var * ((double)a.M / (double)(a.M - 1)) : var;
                a.rvar[o] = (1.f - a.momentum) * a.rvar[o] + a.momentum * (float)unb;
            }
            if (o == 0 && a.nbt) *a.nbt += 1;
        }
    } else {
        mu = a.rmean[o];
        is = 1.f / sqrtf(a.rvar[o] + a.eps);
    }
    if (lane == 0) { a.mean[o] = mu; a.invstd[o] = is; }
    const float z = act_apply((yv - mu) * is * a.gamma[o] + a.bn_beta[o], a.act, a.slope);
    if (row) {
        a.y[(int64_t)m * a.O + o] = yv;
        a.out[(int64_t)m * a.O + o] = z;
    }
}

// ---------------------------------------------------------------------------------------------- backward, weights side
struct HeadBwdArgs {
    const float* g; const float* y; const float* mean; const float* invstd; const float* gamma; const float* bn_beta;
    const float* scale; const float* W; const float* w_b;
    const uint64_t* xcs; const uint64_t* xcz; const uint64_t* xt;
    float* dnT; float* dW; float* dscale; float* dgamma; float* dbn_beta; float* dx; float* dbeta_in;
    int M, K, KW, O, training, act;
    float slope;
};

__global__ __launch_bounds__(256) void binhead_bwd_w_kernel(HeadBwdArgs a) {
    __shared__ float part_s[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int o = blockIdx.x, M = a.M, K = a.K;
    // ---- BatchNorm + activation backward of channel o (every wave repeats it: lane = row)
    const bool row = lane < M;
    const int mc = row ? lane : M - 1;
    const float yv = a.y[(int64_t)mc * a.O + o], gv = row ? a.g[(int64_t)mc * a.O + o] : 0.f;
    const float mu = a.mean[o], is = a.invstd[o], ga = a.gamma[o], be = a.bn_beta[o], sc = a.scale[o];
    const float xh = (yv - mu) * is;
    const float gp = row ? gv * act_grad(xh * ga + be, a.act, a.slope) : 0.f;
    const float r0 = (float)wave_sum((double)gp), r1 = (float)wave_sum((double)gp * (double)xh);
    float dy = gp;
    if (a.training) dy -= (r0 + xh * r1) * (1.f / (float)M);
    dy = row ? dy * ga * is : 0.f;
    if (wave == 0) {
        a.dnT[o * MROWS + lane] = dy * sc;
        if (lane == 0) { a.dgamma[o] = r1; a.dbn_beta[o] = r0; }
    }
    // ---- GX[o, k] = sum_m dy[m] x_b[m, k]: lane = column, the rows' dy through v_readlane, x_b from the column words
    float part = 0.f;
    for (int kw = wave; kw < a.KW; kw += 4) {
        const int k = kw * 64 + lane;
        const bool in = k < K;
        const int kc = in ? k : K - 1;
        const uint64_t cs = a.xcs[kc], cz = a.xcz[kc];
        const float w = a.W[(int64_t)o * K + kc];
        const uint64_t posw = cz & cs, negw = cz & ~cs;
        const int p0 = (int)(uint32_t)posw, p1 = (int)(uint32_t)(posw >> 32), n0 = (int)(uint32_t)negw, n1 = (int)(uint32_t)(negw >> 32);
        float gx = 0.f;
        const int M0 = min(M, 32);
        for (int m = 0; m < M0; ++m) {
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dy), m));
            const int t = __builtin_amdgcn_sbfe(n0, m, 1) - __builtin_amdgcn_sbfe(p0, m, 1);      // +1 / 0 / -1
            gx = fmaf((float)t, d, gx);
        }
        for (int m = 32; m < M; ++m) {
            const float d = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dy), m));
            const int t = __builtin_amdgcn_sbfe(n1, m - 32, 1) - __builtin_amdgcn_sbfe(p1, m - 32, 1);
            gx = fmaf((float)t, d, gx);
        }
        if (in) {
            const float s = (w > 0.f) ? 1.f : ((w < 0.f) ? -1.f : 0.f);
            part += s * gx;
            if (a.dW) a.dW[(int64_t)o * K + k] = (fabsf(w) <= 1.2f) ? sc * gx : 0.f;
        }
    }
    part = wave_sum(part);
    if (lane == 0) part_s[wave] = part;
    __syncthreads();
    if (tid == 0) a.dscale[o] = (part_s[0] + part_s[1]) + (part_s[2] + part_s[3]);
}

// ---------------------------------------------------------------------------------------------- backward, input side
// MP: rows padded to 8 / 16 / 32 / 64 (accumulators per lane); NWV waves split the output channels.
template <int MP, int NWV>
__global__ __launch_bounds__(NWV * 64) void binhead_bwd_x_kernel(HeadBwdArgs a) {
    extern __shared__ float red[];                    // [NWV][MP][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kw = blockIdx.x, K = a.K, O = a.O, M = a.M;
    const int k = kw * 64 + lane;
    const bool in = k < K;
    const int kc = in ? k : K - 1;
    const int och = (O + NWV - 1) / NWV;
    const int o0 = wave * och, o1 = min(O, o0 + och);
    float acc[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) acc[m] = 0.f;
    constexpr int UO = 8;
    for (int o = o0; o < o1; o += UO) {
        float w[UO];
#pragma unroll
        for (int u = 0; u < UO; ++u) {
            const int oc = min(o + u, O - 1);
            w[u] = a.w_b[(int64_t)oc * K + kc];
        }
#pragma unroll
        for (int u = 0; u < UO; ++u) {
            const int oc = min(o + u, o1 - 1);       // (clamped inside the wave's range; masked through the weight)
            const float wv = (o + u < o1) ? w[u] : 0.f;
            const float* dr = a.dnT + oc * MROWS;     // wave-uniform row: scalar loads
#pragma unroll
            for (int m = 0; m < MP; ++m) acc[m] = fmaf(dr[m], wv, acc[m]);
        }
    }
#pragma unroll
    for (int m = 0; m < MP; ++m) red[(wave * MP + m) * 64 + lane] = acc[m];
    __syncthreads();
    float colsum = 0.f;
    for (int m = wave; m < M; m += NWV) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NWV; ++w2) s += red[(w2 * MP + m) * 64 + lane];
        const uint64_t st = a.xt[m * a.KW + kw];
        const float dxv = ((st >> lane) & 1ull) ? s : 0.f;
        if (in) a.dx[(int64_t)m * K + k] = dxv;
        colsum += dxv;
    }
    __syncthreads();
    red[wave * 64 + lane] = colsum;
    __syncthreads();
    if (wave == 0 && in) {
        float s = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < NWV; ++w2) s += red[w2 * 64 + lane];
        a.dbeta_in[k] = s;
    }
}

// ---------------------------------------------------------------------------------------------- fp32 output layer, backward
// y = x W^T + b over M <= 64 rows: dW[o,k] = sum_m g[m,o] x[m,k], dx[m,k] = sum_o g[m,o] W[o,k], db[o] = sum_m g[m,o]; one thread
// per output element of the three results.
__global__ __launch_bounds__(256) void fplinear_small_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                                 const float* __restrict__ W, int M, int K, int O, float* __restrict__ dx,
                                                                 float* __restrict__ dW, float* __restrict__ db) {
    const int64_t nW = (int64_t)O * K, nX = dx ? (int64_t)M * K : 0, nB = db ? O : 0;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nW) {
        if (!dW) return;
        const int o = (int)(e / K), k = (int)(e - (int64_t)o * K);
        float s = 0.f;
        for (int m = 0; m < M; ++m) s = fmaf(g[m * O + o], x[(int64_t)m * K + k], s);
        dW[e] = s;
    } else if (e < nW + nX) {
        const int64_t r = e - nW;
        const int m = (int)(r / K), k = (int)(r - (int64_t)m * K);
        float s = 0.f;
        for (int o = 0; o < O; ++o) s = fmaf(g[m * O + o], W[(int64_t)o * K + k], s);
        dx[r] = s;
    } else if (e < nW + nX + nB) {
        const int o = (int)(e - nW - nX);
        float s = 0.f;
        for (int m = 0; m < M; ++m) s += g[m * O + o];
        db[o] = s;
    }
}

}  // namespace

extern "C" int svnet_binhead_pack_f32(const float* x, const float* beta, int64_t M, int64_t K, uint64_t* x_sign, uint64_t* x_nz,
                                      uint64_t* x_ste, uint64_t* xc_sign, uint64_t* xc_nz, uint64_t* xc_ste, void* stream) {
    SVNET_REQUIRE(x && beta && x_sign && x_nz && ((xc_sign == nullptr) == (xc_nz == nullptr)), SVNET_E_ARG, "svnet_binhead_pack_f32: null pointer");
    SVNET_REQUIRE(M >= 1 && M <= MROWS && K >= 1 && K <= (1 << 20), SVNET_E_UNSUPPORTED, "svnet_binhead_pack_f32: 1 <= M <= 64 rows");
    const int KW = (int)((K + 63) / 64);
    hipLaunchKernelGGL(binhead_pack_kernel, dim3((unsigned)KW), dim3(64), 0, (hipStream_t)stream, x, beta, (int)M, (int)K, KW, x_sign, x_nz,
                       x_ste, xc_sign, xc_nz, xc_sign ? xc_ste : nullptr);
    SVNET_CHECK_LAUNCH("binhead_pack_kernel");
    return SVNET_OK;
}

static int binhead_check(const svnet_binhead_desc& d, const char* who) {
    SVNET_REQUIRE(d.M >= 1 && d.M <= MROWS, SVNET_E_UNSUPPORTED, "%s: 1 <= M <= 64 rows", who);
    SVNET_REQUIRE(d.K >= 1 && d.K <= 8192 && d.O >= 1 && d.O <= (1 << 20) && d.wld >= (d.K + 63) / 64, SVNET_E_UNSUPPORTED,
                  "%s: K <= 8192, O <= 2^20, wld >= ceil(K/64)", who);
    SVNET_REQUIRE(d.act >= 0 && d.act <= 2, SVNET_E_ARG, "%s: act in {0 none, 1 leaky, 2 relu}", who);
    return SVNET_OK;
}

extern "C" int svnet_binhead_fwd_f32(const svnet_binhead_desc* desc, void* stream) {
    SVNET_REQUIRE(desc, SVNET_E_ARG, "svnet_binhead_fwd_f32: null descriptor");
    const svnet_binhead_desc& d = *desc;
    if (int rc = binhead_check(d, "svnet_binhead_fwd_f32")) return rc;
    SVNET_REQUIRE(d.x_sign && d.x_nz && d.w_sign && d.w_nz && d.scale && d.gamma && d.bn_beta && d.y && d.mean && d.invstd && d.out,
                  SVNET_E_ARG, "svnet_binhead_fwd_f32: null pointer");
    SVNET_REQUIRE(d.training || (d.running_mean && d.running_var), SVNET_E_ARG, "svnet_binhead_fwd_f32: eval mode needs the running statistics");
    HeadFwdArgs a;
    a.xs = d.x_sign; a.xz = d.x_nz; a.w_sign = d.w_sign; a.w_nz = d.w_nz; a.scale = d.scale; a.gamma = d.gamma; a.bn_beta = d.bn_beta;
    a.rmean = d.running_mean; a.rvar = d.running_var; a.nbt = d.training ? d.nbt : nullptr;
    a.y = d.y; a.mean = d.mean; a.invstd = d.invstd; a.out = d.out;
    a.M = (int)d.M; a.K = (int)d.K; a.KW = (int)((d.K + 63) / 64); a.O = (int)d.O; a.wld = (int)d.wld; a.training = d.training; a.act = d.act;
    a.eps = d.eps; a.momentum = d.momentum; a.slope = d.slope;
    const size_t lds = ((size_t)2 * MROWS * (a.KW | 1) + (size_t)2 * FWD_OC * a.KW) * sizeof(uint64_t);
    SVNET_REQUIRE(lds <= 65536, SVNET_E_UNSUPPORTED, "svnet_binhead_fwd_f32: K <= 3776 (the packed rows of the batch live in LDS)");
    hipLaunchKernelGGL(binhead_fwd_kernel, dim3((unsigned)svnet_cdiv(d.O, FWD_OC)), dim3(256), lds, (hipStream_t)stream, a);
    SVNET_CHECK_LAUNCH("binhead_fwd_kernel");
    return SVNET_OK;
}

extern "C" int svnet_binhead_bwd_f32(const svnet_binhead_desc* desc, void* stream) {
    SVNET_REQUIRE(desc, SVNET_E_ARG, "svnet_binhead_bwd_f32: null descriptor");
    const svnet_binhead_desc& d = *desc;
    if (int rc = binhead_check(d, "svnet_binhead_bwd_f32")) return rc;
    SVNET_REQUIRE(d.g && d.y && d.mean && d.invstd && d.gamma && d.bn_beta && d.scale && d.W && d.w_b && d.xc_sign && d.xc_nz && d.x_ste &&
                      d.dnT && d.dscale && d.dgamma && d.dbn_beta, SVNET_E_ARG, "svnet_binhead_bwd_f32: null pointer");
    SVNET_REQUIRE((d.dx == nullptr) == (d.dbeta_in == nullptr), SVNET_E_ARG, "svnet_binhead_bwd_f32: dx and dbeta_in come together");
    HeadBwdArgs a;
    a.g = d.g; a.y = d.y; a.mean = d.mean; a.invstd = d.invstd; a.gamma = d.gamma; a.bn_beta = d.bn_beta; a.scale = d.scale; a.W = d.W;
    a.w_b = d.w_b; a.xcs = d.xc_sign; a.xcz = d.xc_nz; a.xt = d.x_ste;
    a.dnT = d.dnT; a.dW = d.dW; a.dscale = d.dscale; a.dgamma = d.dgamma; a.dbn_beta = d.dbn_beta; a.dx = d.dx; a.dbeta_in = d.dbeta_in;
    a.M = (int)d.M; a.K = (int)d.K; a.KW = (int)((d.K + 63) / 64); a.O = (int)d.O; a.training = d.training; a.act = d.act; a.slope = d.slope;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(binhead_bwd_w_kernel, dim3((unsigned)d.O), dim3(256), 0, st, a);
    SVNET_CHECK_LAUNCH("binhead_bwd_w_kernel");
    if (!d.dx) return SVNET_OK;
    const unsigned grid = (unsigned)a.KW;
#define SVNET_HEAD_BWD_X(MP, NWV) \
    hipLaunchKernelGGL((binhead_bwd_x_kernel<MP, NWV>), dim3(grid), dim3(NWV * 64), (size_t)NWV * MP * 64 * sizeof(float), st, a)
    if (d.M <= 8) SVNET_HEAD_BWD_X(8, 8);
    else if (d.M <= 16) SVNET_HEAD_BWD_X(16, 8);
    else if (d.M <= 32) SVNET_HEAD_BWD_X(32, 8);
    else SVNET_HEAD_BWD_X(64, 4);
#undef SVNET_HEAD_BWD_X
    SVNET_CHECK_LAUNCH("binhead_bwd_x_kernel");
    return SVNET_OK;
}

extern "C" int svnet_fplinear_small_bwd_f32(const float* g, const float* x, const float* W, int64_t M, int64_t K, int64_t O, float* dx,
                                            float* dW, float* db, void* stream) {
    SVNET_REQUIRE(g && x && W && M >= 1 && K >= 1 && O >= 1, SVNET_E_ARG, "svnet_fplinear_small_bwd_f32: bad arguments");
    SVNET_REQUIRE(M <= MROWS && O * K <= (1 << 22) && O <= 4096, SVNET_E_UNSUPPORTED, "svnet_fplinear_small_bwd_f32: M <= 64, O*K <= 4 M");
    const int64_t total = O * K + (dx ? M * K : 0) + (db ? O : 0);
    hipLaunchKernelGGL(fplinear_small_bwd_kernel, dim3((unsigned)svnet_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, g, x, W, (int)M,
                       (int)K, (int)O, dx, dW, db);
    SVNET_CHECK_LAUNCH("fplinear_small_bwd_kernel");
    return SVNET_OK;
}
