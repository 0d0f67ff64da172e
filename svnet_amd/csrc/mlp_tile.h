// The layer engine of the fused inference levels (sa_fused.hip, fp_fused.hip, sa_global.hip), stated once: a stack of folded 1x1 convolution +
// BatchNorm + ReLU layers over a tile of rows that lie in LDS, on v_mfma_f32_16x16x4_f32.  Per layer and output o the value is
//   acc = bf[o];  for c ascending acc = fmaf(h[c], Wf[o,c], acc);  h'[o] = acc > 0 ? acc : +0
// bit for bit: the bias is the accumulator's start, a wave owns 16-column tiles over the full K, and K is never split, so no value
// depends on how rows or columns are tiled.  Activations ping-pong between two LDS buffers, weights come from global
// memory (L2-resident) into registers, MLP_U k-steps ahead.  What happens to the LAST layer's ReLU outputs is the caller's: an epilogue
// policy (below).  Around the engine, stated once too: the host's plan pieces (mlp_strides, mlp_opad, mlp_rows), its launch pieces
// (mlp_level, mlp_window, mlp_optional, mlp_lds_optin) and the kernels' loop over the layers (mlp_stack); the gather into buffer 0, the
// policy and sa_fused.hip's plan in centres are each level's own.  Internal: not part of the C interface.  Built with -ffp-contract=off.
#pragma once
#include "pointset.h"

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int MLP_THREADS = 256, MLP_WAVES = MLP_THREADS / SVNET_WAVE;
constexpr int MLP_MAX_WIDTH = 256;                               // of a layer: 16 column tiles, four per wave
constexpr int MLP_LDS_MAX = 160 * 1024;
constexpr int MLP_U = 8;                                         // k-steps whose weights a lane holds at a time: 32 channels

inline int pad_to(int64_t v, int m) { return (int)((v + m - 1) / m * m); }

// The folded layers and widths of a call handed to the kernel by value: no device copy.  C[0] = input columns, C[l] = width of layer l.
struct MlpLevel {
    const float* w[SVNET_SA_MAX_LAYERS];
    const float* b[SVNET_SA_MAX_LAYERS];
    int C[SVNET_SA_MAX_LAYERS + 1];
    int L;
};

// The row strides of the two activation buffers (layer l reads buffer l & 1 and writes the other one) for C0 input columns: the
// widest row a buffer holds, padded to whole k-steps, then to 4 times an odd number: the 16 rows x 4 channels of an A fragment, and
// the 16 columns x 4 row quads of a result, then fall into 64 different banks.  (The last layer's outputs never go to a buffer.)
inline void mlp_strides(int64_t C0, int64_t L, const int64_t* widths, int (&stride)[2]) {
    stride[0] = stride[1] = 0;
    for (int64_t l = 0; l < L; ++l) {
        const int c = pad_to(l ? widths[l - 1] : C0, 4), s = c % 8 ? c : c + 4;
        if (s > stride[l & 1]) stride[l & 1] = s;
    }
}

// The last width padded to whole column tiles: a row of a kernel's table of column maxima.
inline int mlp_opad(int64_t L, const int64_t* widths) { return pad_to(widths[L - 1], 16); }

// The row plan of a kernel whose workgroup takes `rows` consecutive rows: the first of `cands` (descending) whose two activation
// buffers and `extra` more bytes fit in LDS, lds = 4 rows (stride[0] + stride[1]) + extra <= MLP_LDS_MAX; false when none does.
template <int NC>
inline bool mlp_rows(const int (&cands)[NC], const int (&stride)[2], int64_t extra, int& rows, int& lds) {
    for (const int r : cands) {
        const int64_t need = (int64_t)4 * r * (stride[0] + stride[1]) + extra;
        if (need <= MLP_LDS_MAX) { rows = r; lds = (int)need; return true; }
    }
    return false;
}

// (max_width: the column-tile loop of mlp_layer takes any width; a kernel's envelope may be wider than MLP_MAX_WIDTH - sa_global.hip)
inline bool mlp_widths_ok(int64_t L, const int64_t* widths, int64_t max_width = MLP_MAX_WIDTH) {
    if (!widths || L < 1 || L > SVNET_SA_MAX_LAYERS) return false;
    for (int64_t l = 0; l < L; ++l)
        if (widths[l] < 1 || widths[l] > max_width) return false;
    return true;
}

// ---- the launch pieces of an entry point `name` (svnet_*_f32): each returns SVNET_OK or, with svnet_last_error set, the error.
// The level of a call from its arguments: C0 input columns, and per layer the width and the folded weights and bias.
inline int mlp_level(const char* name, int64_t C0, int64_t L, const int64_t* widths, const void* wf, const void* bf, MlpLevel& lv) {
    lv = MlpLevel{};
    lv.L = (int)L;
    lv.C[0] = (int)C0;
    const auto w = static_cast<const float* const*>(wf), bb = static_cast<const float* const*>(bf);
    for (int l = 0; l < lv.L; ++l) {
        SVNET_REQUIRE(w[l] && bb[l], SVNET_E_ARG, "%s: null wf[%d] / bf[%d]", name, l, l);
        lv.w[l] = w[l];
        lv.b[l] = bb[l];
        lv.C[l + 1] = (int)widths[l];
    }
    return SVNET_OK;
}

// The window of the result: the level's CL channels from c_off on lie inside the C_total of out.
inline int mlp_window(const char* name, int64_t c_off, int64_t CL, int64_t C_total) {
    SVNET_REQUIRE(c_off >= 0 && c_off + CL <= C_total, SVNET_E_ARG, "%s: channels %lld .. %lld outside C_total %lld", name, (long long)c_off,
                  (long long)(c_off + CL), (long long)C_total);
    return SVNET_OK;
}

// A feature matrix of zero columns may be null.  It is never read, but the kernels form addresses from it: any valid pointer serves.
inline const float* mlp_optional(const float* p, const float* other) { return p ? p : other; }

// The opt-in of KERNEL (one record of the devices done per kernel: common.h) to MLP_LDS_MAX bytes of dynamic LDS where the plan needs it.
template <auto KERNEL>
inline int mlp_lds_optin(const char* name, int lds) {
    bool ok = true;
    if (lds > 64 * 1024) SVNET_LDS_OPTIN(ok, MLP_LDS_MAX, name, reinterpret_cast<const void*>(KERNEL));
    return ok ? SVNET_OK : SVNET_E_LAUNCH;
}

// The epilogue of a layer that is not the last: its outputs go to the other activation buffer (mlp_layer does that itself).
struct MlpToLds {
    static constexpr bool LAST = false;
    __device__ __forceinline__ void operator()(int, int, const float (&)[4]) const {}
};

// The B operands of one lane for MLP_U k-steps from channel c on, step u at channel c + 4 u: Wf[o][c + 4 u] of the lane's column o.  A
// channel past the row is an exact zero; its load reads the row's last weight instead, so that no load needs a branch.
// (W is wave-uniform and row = o Cin a 32-bit lane offset: the loads take the SGPR-base form and keep no 64-bit address per load.)
__device__ __forceinline__ void mlp_weights(const float* __restrict__ W, int row, int Cin, int c, float (&w)[MLP_U]) {
#pragma unroll
    for (int u = 0; u < MLP_U; ++u) {
        const int cu = c + 4 * u;
        const float x = ld_f32_sbase_fresh(W, (uint32_t)(row + (cu < Cin ? cu : Cin - 1)) * 4u);
        w[u] = cu < Cin ? x : 0.f;
    }
}

// One layer over the NRT 16-row tiles of the workgroup's rows.  A wave takes the column tiles wave, wave + 4, ...  A lane holds the B
// operands of its column o = 16 ct + lane % 16 for MLP_U k-steps (channels k0 + lane / 16 + 4 u) in registers, straight from global
// memory, and the next MLP_U - of this tile or, at its end, of the wave's next tile - are under way while these multiply.  More steps
// in flight, or the activations read ahead of their products, cost registers, and a fourth wave per SIMD was worth more than either
// (DESIGN.md 4.20).  The A operands (row 16 rt + lane % 16, channel k0 + lane / 16) come from the activation buffer and feed NRT
// independent accumulators that started at the bias.  A lane of a result holds column lane % 16 of rows 4 (lane / 16) + 0..3.
// Epi::LAST: the ReLU outputs of a real column o go to epi(first row, o, the four values) instead of LDS.
template <int NRT, class Epi>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ bias, int Cin, int O, const float* in, int sin,
                                          float* outb, int sout, Epi epi, int wave, int lane) {
    const int r16 = lane & 15, q = lane >> 4;
    const int Kp = (Cin + 3) & ~3, Op = (O + 3) & ~3, nct = (O + 15) >> 4;
    const float* arow = in + r16 * sin + q;
    float wc[MLP_U], wn[MLP_U];
    if (wave < nct) {
        const int o = wave * 16 + r16;
        mlp_weights(W, (o < O ? o : O - 1) * Cin, Cin, q, wc);
    }
    for (int ct = wave; ct < nct; ct += MLP_WAVES) {
        const int o = ct * 16 + r16, on = o + 16 * MLP_WAVES;
        const bool ov = o < O;
        const int wrow = (ov ? o : O - 1) * Cin, wnext = (on < O ? on : O - 1) * Cin;      // (past the last tile: loaded, never used)
        const float b0 = ov ? bias[o] : 0.f;
        f32x4 acc[NRT];
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) acc[rt] = f32x4{b0, b0, b0, b0};
        for (int k0 = 0; k0 < Kp; k0 += 4 * MLP_U) {
            if (k0 + 4 * MLP_U < Kp) mlp_weights(W, wrow, Cin, k0 + 4 * MLP_U + q, wn);
            else mlp_weights(W, wnext, Cin, q, wn);
#pragma unroll
            for (int u = 0; u < MLP_U; ++u) {
                if (k0 + 4 * u >= Kp) break;                     // (wave-uniform)
#pragma unroll
                for (int rt = 0; rt < NRT; ++rt)
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(arow[rt * 16 * sin + k0 + 4 * u], wc[u], acc[rt], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < MLP_U; ++u) wc[u] = wn[u];
        }
#pragma unroll
        for (int rt = 0; rt < NRT; ++rt) {
            const int row = rt * 16 + q * 4;
            float v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = ov && acc[rt][i] > 0.f ? acc[rt][i] : 0.f;      // a column past the layer's: zero
            if (!Epi::LAST) {
                if (o < Op) {                                    // up to the next layer's padded K: zeros
#pragma unroll
                    for (int i = 0; i < 4; ++i) outb[(row + i) * sout + o] = v[i];
                }
            } else if (ov) {
                epi(row, o, v);
            }
        }
    }
}

template <class Epi>
__device__ __forceinline__ void mlp_layer_rt(int nrt, const float* W, const float* bias, int Cin, int O, const float* in, int sin, float* outb,
                                             int sout, Epi epi, int wave, int lane) {
    switch (nrt) {
        case 1: mlp_layer<1>(W, bias, Cin, O, in, sin, outb, sout, epi, wave, lane); break;
        case 2: mlp_layer<2>(W, bias, Cin, O, in, sin, outb, sout, epi, wave, lane); break;
        case 3: mlp_layer<3>(W, bias, Cin, O, in, sin, outb, sout, epi, wave, lane); break;
        default: mlp_layer<4>(W, bias, Cin, O, in, sin, outb, sout, epi, wave, lane); break;
    }
}

// The layer stack over the NRT = nrt 16-row tiles in buffer 0: layer l reads buffer l & 1 and writes the other one, with a barrier
// behind it; the last layer's ReLU outputs go to `last` instead - handed over by value, so a policy may keep state during the layer.
// BARRIER_LAST: a barrier behind the last layer too, for a policy whose results the workgroup reads back from LDS.
template <bool BARRIER_LAST, class Epi>
__device__ __forceinline__ void mlp_stack(int nrt, const MlpLevel& lv, const int (&stride)[2], float* buf0, float* buf1, Epi last, int wave,
                                          int lane) {
    for (int l = 0; l < lv.L; ++l) {
        const float* in = l & 1 ? buf1 : buf0;
        float* outb = l & 1 ? buf0 : buf1;
        const int sin = stride[l & 1], sout = stride[(l & 1) ^ 1];
        if (l + 1 < lv.L) mlp_layer_rt(nrt, lv.w[l], lv.b[l], lv.C[l], lv.C[l + 1], in, sin, outb, sout, MlpToLds{}, wave, lane);
        else mlp_layer_rt(nrt, lv.w[l], lv.b[l], lv.C[l], lv.C[l + 1], in, sin, outb, sout, last, wave, lane);
        if (BARRIER_LAST || l + 1 < lv.L) __syncthreads();
    }
}

}  // namespace
