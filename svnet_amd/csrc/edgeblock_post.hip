// Small point-level / parameter-level stages around the fused edge pass of a binarized edge layer (edgeblock.hip,
// edgeblock_bwd.hip).  Each replaces a handful of launch-bound framework ops by ONE launch:
//   svnet_edgeblock_prepare_vec_f32 : sign(W2), sign(Wz) rearranged for the per-point products U|T and Zp|Zq
//   svnet_knn_reverse_i32           : reverse neighbour lists of a kNN graph (scatter -> gather)
//   svnet_edgeblock_bwd_gather_f32  : neighbour sums of the per-edge message rows -> A = [dU | dT | dZp | dZq] rows, ds, dv, dbeta
//   svnet_edgeblock_bwd_params_f32  : STE chain rule to (W1, scale1), (W2, scale2), (Wz, scalez) from the three Gram products
// Reference: models/sv_layers.py:35-51 (Linear bw/ba), :172-196 (SVBlock), models/utils/sv_util.py:90-116 (edge features).
#include "common.h"

namespace {

__device__ __forceinline__ float sgn(float w) { return (w > 0.f) ? 1.f : ((w < 0.f) ? -1.f : 0.f); }

// wv [2Ov+6, Cv]: rows 0..Ov-1 = sign(W2[:, :Cv]) (acts on v_j - v_i -> U), Ov..2Ov-1 = sign(W2[:, Cv:]) (acts on v_i -> T),
// then 3 rows sign(Wz[:, :Cv]) (Zp) and 3 rows sign(Wz[:, Cv:]) (Zq).  scv [2Ov+6] = [sc2, sc2, scz, scz].
__global__ void prepare_vec_kernel(const float* __restrict__ W2, const float* __restrict__ sc2, const float* __restrict__ Wz,
                                   const float* __restrict__ scz, int Ov, int Cv, float* __restrict__ wv, float* __restrict__ scv) {
    const int R = 2 * Ov + 6;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < R * Cv + R; e += gridDim.x * blockDim.x) {
        if (e < R * Cv) {
            const int r = e / Cv, c = e - r * Cv;
            float w;
            if (r < 2 * Ov) w = W2[(r % Ov) * 2 * Cv + (r / Ov) * Cv + c];
            else { const int q = r - 2 * Ov; w = Wz[(q % 3) * 2 * Cv + (q / 3) * Cv + c]; }
            wv[e] = sgn(w);
        } else {
            const int r = e - R * Cv;
            scv[r] = r < 2 * Ov ? sc2[r % Ov] : scz[(r - 2 * Ov) % 3];
        }
    }
}

// One wave per weight row.  Rows [0,Os): linear1 from GXp [Os,320] (fused column order); [Os,Os+Ov): linear2 from
// GXc[0:2Ov] ([o] = U part, [Ov+o] = T part); last 3: v2s frame from GXc[2Ov:2Ov+6].  Gradients are ASSIGNED.
__global__ __launch_bounds__(256) void bwd_params_kernel(const float* __restrict__ GXp, const float* __restrict__ GXc,
                                                         const float* __restrict__ W1, const float* __restrict__ sc1,
                                                         const float* __restrict__ W2, const float* __restrict__ sc2,
                                                         const float* __restrict__ Wz, const float* __restrict__ scz, int Os, int Ov,
                                                         int Cs, int Cv, float* __restrict__ dW1, float* __restrict__ dsc1,
                                                         float* __restrict__ dW2, float* __restrict__ dsc2, float* __restrict__ dWz,
                                                         float* __restrict__ dscz) {
    const int lane = threadIdx.x & 63;
    const int row = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (row >= Os + Ov + 3) return;
    float part = 0.f;
    if (row < Os) {
        const int K1 = 2 * Cs + 6 * Cv;
        const float sc = sc1[row];
        for (int f = lane; f < K1; f += 64) {
            const int g = f - 2 * Cs;
            const int col = f < Cs ? f : (f < 2 * Cs ? 64 + f - Cs : 128 + 64 * (g % 3) + g / 3);
            const float w = W1[row * K1 + f], gx = GXp[row * 320 + col];
            part += sgn(w) * gx;
            dW1[row * K1 + f] = (fabsf(w) <= 1.2f) ? sc * gx : 0.f;
        }
        part = wave_sum(part);
        if (lane == 0) dsc1[row] = part;
        return;
    }
    const bool is2 = row < Os + Ov;
    const int o = is2 ? row - Os : row - Os - Ov;
    const int O = is2 ? Ov : 3;
    const float* W = is2 ? W2 : Wz;
    const float* G = is2 ? GXc : GXc + (int64_t)2 * Ov * Cv;
    float* dW = is2 ? dW2 : dWz;
    const float sc = is2 ? sc2[o] : scz[o];
    for (int f = lane; f < 2 * Cv; f += 64) {
        const int half = f >= Cv, c = f - half * Cv;
        const float w = W[o * 2 * Cv + f], gx = G[(o + half * O) * Cv + c];
        part += sgn(w) * gx;
        dW[o * 2 * Cv + f] = (fabsf(w) <= 1.2f) ? sc * gx : 0.f;
    }
    part = wave_sum(part);
    if (lane == 0) (is2 ? dsc2 : dscz)[o] = part;
}

// ---- reverse neighbour lists of one kNN graph: for every point j the edges e = i*k + t with idx[e] == j, grouped by j
// (rev_range[2j], rev_range[2j+1]) = [begin, end) into rev_edge.  One workgroup per cloud; counters and the scan live in
// LDS (N <= 8192).  The order inside a list follows the LDS atomics and is not fixed from run to run.
constexpr int REV_MAX_N = 8192;
// Lists longer than `chunk` entries (feature-space graphs have hubs: 206 incoming edges against a mean of 20 on the bench model's
// last layer) are cut up: every further chunk of such a list becomes an item (point, chunk number) of ovf_items, counted in
// ovf_count[0], which the gather kernel's second launch sums with atomics - a wave per whole list made the kernel as slow as its
// longest list.
__global__ __launch_bounds__(1024) void knn_reverse_kernel(const int64_t* __restrict__ idx, int N, int k, int32_t* __restrict__ rev_range,
                                                          int32_t* __restrict__ rev_edge, int32_t* __restrict__ rev_src, int chunk,
                                                          int32_t* __restrict__ ovf_items, int32_t* __restrict__ ovf_count) {
    extern __shared__ int cnt[];          // [N] counts -> cursors; [N .. N+1024) scan scratch
    int* part = cnt + N;
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int64_t e0 = (int64_t)b * N * k;
    const int EN = N * k;
    for (int j = tid; j < N; j += nt) cnt[j] = 0;
    __syncthreads();
    for (int e = tid; e < EN; e += nt) {
        const int64_t j = idx[e0 + e];
        if ((uint64_t)j < (uint64_t)N) atomicAdd(&cnt[(int)j], 1);     // out-of-range ids are skipped everywhere
    }
    __syncthreads();
    // exclusive scan of cnt[0..N): each thread owns a contiguous run
    const int per = (N + nt - 1) / nt;
    const int j0 = min(tid * per, N), j1 = min(j0 + per, N);
    int run = 0;
    for (int j = j0; j < j1; ++j) run += cnt[j];
    part[tid] = run;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {
        const int v = tid >= off ? part[tid - off] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int base = part[tid] - run;          // exclusive prefix of this thread's run
    for (int j = j0; j < j1; ++j) {
        const int c = cnt[j];
        rev_range[2 * ((int64_t)b * N + j)] = (int32_t)(e0 + base);
        rev_range[2 * ((int64_t)b * N + j) + 1] = (int32_t)(e0 + base + c);
        cnt[j] = base;                   // becomes the fill cursor
        base += c;
        if (ovf_count && c > chunk) {
            const int extra = (c - 1) / chunk;                            // chunks 1 .. extra
            const int pos = atomicAdd(ovf_count, extra);
            for (int q = 0; q < extra; ++q) { ovf_items[2 * (pos + q)] = b * N + j; ovf_items[2 * (pos + q) + 1] = q + 1; }
        }
    }
    __syncthreads();
    for (int e = tid; e < EN; e += nt) {
        const int64_t j = idx[e0 + e];
        if ((uint64_t)j < (uint64_t)N) {
            const int pos = atomicAdd(&cnt[(int)j], 1);
            rev_edge[e0 + pos] = (int32_t)(e0 + e);
            rev_src[e0 + pos] = b * N + e / k;                 // global id of the edge's source point
        }
    }
}


// ---- neighbour sums over the reverse lists: one wave per destination point j, lanes = columns.
//   message rows msg[e] = [ds (Cs) | dve (3 Cv) | dz (9)] are summed (NCH chunks of 64 columns);
//   the neighbour's share of dL/dv' (v' = U_j - U_i + T_i) of every incoming edge is RECOMPUTED from U_j (own row) and the
//   source point's tables ub = T_i - U_i, ge = gv_i*gate/k (lanes = Ov channels, three axes per lane): it costs ~40 VALU per
//   edge on a kernel that waits on HBM, and saves writing and re-reading 3*Ov floats per edge.
// Next row / next tables are requested two entries ahead.  Writes the gradient rows of the collapsed products directly:
//   acat[(j,a), :] = [U_a - dvc | dvc | Z_a - dzc | dzc],   ds_acc[j] += S,   dv_acc[j] += V.
// OVF = false: wave j sums the first `chunk` entries of list j and WRITES the point's rows; OVF = true (second launch, behind
// the first on the stream): the waves walk the items (point, chunk number) of the longer lists and ADD their sums with atomics.
// PACK (Ov <= 32): the recomputation of the neighbour's share of dL/dv' runs on G = 64 / Ov incoming edges per wave-instruction
// (lane = (edge slot, channel), like edgeblock_bwd_vec_kernel) in a loop of its own, instead of on one edge with 64 - Ov lanes idle:
// the kernel is bound by its per-edge instructions, not by memory, and that part was 40 of its ~50 per edge.
template <int NCH, bool OVF, bool PACK>
__global__ __launch_bounds__(256) void edgeblock_bwd_gather_kernel(const float* __restrict__ msg, const int32_t* __restrict__ rev_range,
                                                                   const int32_t* __restrict__ rev_edge, const int32_t* __restrict__ rev_src,
                                                                   const float* __restrict__ ut, const float* __restrict__ ub_tab,
                                                                   const float* __restrict__ ge_tab, const float* __restrict__ coef,
                                                                   const float* __restrict__ bcoef, int Os, const float* __restrict__ dvc,
                                                                   const float* __restrict__ dzc, int64_t P, int bpc, int Cs, int Cv, int Ov, int R,
                                                                   float* __restrict__ acat, int RW, float* __restrict__ ds_acc,
                                                                   float* __restrict__ dv_acc, const float* __restrict__ dbeta_perm,
                                                                   float* __restrict__ dbeta1, int chunk, const int32_t* __restrict__ ovf_items,
                                                                   const int32_t* __restrict__ ovf_count) {
    const int lane = threadIdx.x & 63;
    // XCD-aware order (bpc = workgroups per cloud, 0 = off): workgroups b and b+8 share an XCD, so XCD x walks the clouds
    // x, x+8, ... one after the other and the cloud's ub/ge tables (1 MB at Ov = 42) are served from that XCD's L2
    int64_t blk = blockIdx.x;
    if (bpc > 0) {
        const int64_t xcd = blk & 7, slot = blk >> 3;
        blk = ((slot / bpc) * 8 + xcd) * bpc + (slot % bpc);
    }
    const int64_t wave_g = blk * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (!OVF && blockIdx.x == 0) {       // dL/dbeta from the fused column order back to the reference's feature order
        const int K1 = 2 * Cs + 6 * Cv;
        for (int f = threadIdx.x; f < K1; f += blockDim.x) {
            const int g = f - 2 * Cs;
            const int col = f < Cs ? f : (f < 2 * Cs ? 64 + f - Cs : 128 + 64 * (g % 3) + g / 3);
            float s = 0.f;                       // (the tile kernel spreads its column sums over SVNET_DBETA_SLICES copies: every tile adding
            for (int q = 0; q < SVNET_DBETA_SLICES; ++q) s += dbeta_perm[q * 320 + col];   //  to the same ten cache lines serialised at the memory side)
            dbeta1[f] = s;
        }
    }
    if (!OVF && wave_g >= P) return;
    const int n_items = OVF ? __builtin_amdgcn_readfirstlane(ovf_count[0]) : 1;
    uint32_t col[NCH];               // unsigned 32-bit lane offsets + wave-uniform row bases: SGPR-base loads, no 64-bit VALU adds
#pragma unroll
    for (int q = 0; q < NCH; ++q) col[q] = 4u * (uint32_t)min(64 * q + lane, R - 1);   // BYTE offsets; clamped: lanes past the row re-read its last column
    // vector path operands of this lane's channel
    const int pG = PACK ? 64 / Ov : 1, pg = PACK ? lane / Ov : 0;      // PACK: edge slot of the lane, its channel lane - pg * Ov
    const bool pact = pg < pG;
    const int o = PACK ? (pact ? lane - pg * Ov : 0) : min(lane, Ov - 1);
    const uint32_t o0 = 4u * (uint32_t)o, o1 = 4u * (uint32_t)(o + Ov), o2 = 4u * (uint32_t)(o + 2 * Ov);   // byte offsets
#define SVNET_AT(BASE, BYTES) ld_f32_sbase(BASE, BYTES)
    const float* Av = coef + 4 * Os; const float* C0 = bcoef + 3 * Os;
    const float avc = Av[o], bvc = Av[Ov + o], c0 = C0[o], c1 = C0[Ov + o];
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t it = OVF ? wave_g : 0; it < n_items; it += n_waves) {      // (one trip when !OVF)
    int64_t j = wave_g;
    int beg, end;
    if (OVF) {
        j = __builtin_amdgcn_readfirstlane(ovf_items[2 * it]);
        const int cn = __builtin_amdgcn_readfirstlane(ovf_items[2 * it + 1]);
        beg = rev_range[2 * j] + cn * chunk;
        end = min(rev_range[2 * j + 1], beg + chunk);
    } else {
        beg = rev_range[2 * j];
        end = min(rev_range[2 * j + 1], chunk > 0 ? beg + chunk : 0x7FFFFFFF);
    }
    float acc[NCH];
#pragma unroll
    for (int q = 0; q < NCH; ++q) acc[q] = 0.f;
    const float uj0 = ut[(j * 3 + 0) * 2 * Ov + o], uj1 = ut[(j * 3 + 1) * 2 * Ov + o], uj2 = ut[(j * 3 + 2) * 2 * Ov + o];
    float ua0 = 0.f, ua1 = 0.f, ua2 = 0.f;
    // A ring of four (row, tables) slots with compile-time indices, requested three entries ahead: rotating the prefetched
    // registers instead (x = next; next = load) makes every copy wait for the load it reads, i.e. one full latency per entry.
    float rw[4][NCH], tb[4][6];
#define SVNET_GATHER_LOAD(N_, SLOT)                                                                     \
    do {                                                                                                \
        const float* row_ = msg + (int64_t)__builtin_amdgcn_readlane(ev, (N_)) * R;                     \
        _Pragma("unroll") for (int q = 0; q < NCH; ++q) rw[SLOT][q] = SVNET_AT(row_, col[q]);           \
        const int64_t si_ = (int64_t)__builtin_amdgcn_readlane(sv, (N_)) * 3 * Ov;                      \
        const float* ub_ = ub_tab + si_; const float* ge_ = ge_tab + si_;                               \
        tb[SLOT][0] = SVNET_AT(ub_, o0); tb[SLOT][1] = SVNET_AT(ub_, o1); tb[SLOT][2] = SVNET_AT(ub_, o2); \
        tb[SLOT][3] = SVNET_AT(ge_, o0); tb[SLOT][4] = SVNET_AT(ge_, o1); tb[SLOT][5] = SVNET_AT(ge_, o2); \
    } while (0)
    // the list's edge ids / source points come in with one coalesced load each per 64 entries (lane n holds entry n, handed to
    // the scalar unit by v_readlane), so a row's loads never wait on a load of their own index
    for (int base = beg; base < end; base += 64) {
        const int cnt = min(64, end - base);
        const int ev = rev_edge[base + min(lane, cnt - 1)];
        const int sv = rev_src[base + min(lane, cnt - 1)];
        // The loop body has no branches (the waitcnt pass gives up on the ring when it has to merge paths): entries past the
        // end re-request the list's last entry (cache hits) and are weighted 0.
        const int last = cnt - 1;
        if (PACK) {
            // (A) message rows, one entry per iteration, three entries ahead
#define SVNET_GATHER_ROW(N_, SLOT)                                                                      \
    do {                                                                                                \
        const float* row_ = msg + (int64_t)__builtin_amdgcn_readlane(ev, (N_)) * R;                     \
        _Pragma("unroll") for (int q = 0; q < NCH; ++q) rw[SLOT][q] = SVNET_AT(row_, col[q]);           \
    } while (0)
            SVNET_GATHER_ROW(0, 0);
            SVNET_GATHER_ROW(min(1, last), 1);
            SVNET_GATHER_ROW(min(2, last), 2);
            for (int n4 = 0; n4 < cnt; n4 += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int n = n4 + u;
                    SVNET_GATHER_ROW(min(n + 3, last), (u + 3) & 3);
                    __builtin_amdgcn_sched_barrier(0);
                    const float w = n < cnt ? 1.f : 0.f;
#pragma unroll
                    for (int q = 0; q < NCH; ++q) acc[q] += w * rw[u][q];
                }
            }
#undef SVNET_GATHER_ROW
            // (B) dv' of pG entries at a time: lane (pg, o) takes entry n0 + pg; its source point's tables through 32-bit lane offsets
            const uint32_t ov3 = 12u * (uint32_t)Ov;
#define SVNET_GATHER_TAB(N0, T)                                                                         \
    do {                                                                                                \
        const int n_ = (N0) + pg;                                                                       \
        const uint32_t src_ = (uint32_t)__shfl(sv, min(n_, last), 64);     /* (every lane takes part) */ \
        const uint32_t off_ = src_ * ov3 + 4u * (uint32_t)o;                                            \
        T[0] = SVNET_AT(ub_tab, off_); T[1] = SVNET_AT(ub_tab, off_ + 4u * (uint32_t)Ov); T[2] = SVNET_AT(ub_tab, off_ + 8u * (uint32_t)Ov); \
        T[3] = SVNET_AT(ge_tab, off_); T[4] = SVNET_AT(ge_tab, off_ + 4u * (uint32_t)Ov); T[5] = SVNET_AT(ge_tab, off_ + 8u * (uint32_t)Ov); \
    } while (0)
            float ta[6], tn[6];
            SVNET_GATHER_TAB(0, ta);
            for (int n0 = 0; n0 < cnt; n0 += 2 * pG) {
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float* tc = u ? tn : ta;
                    float* tx = u ? ta : tn;
                    const int nb = n0 + u * pG;
                    SVNET_GATHER_TAB(min(nb + pG, last), tx);             // the next group (clamped: a group past the end is weighted 0)
                    __builtin_amdgcn_sched_barrier(0);
                    const float w = (pact && nb + pg < cnt) ? 1.f : 0.f;
                    const float vp0 = uj0 + tc[0], vp1 = uj1 + tc[1], vp2 = uj2 + tc[2];
                    const float nv = fast_sqrt(vp0 * vp0 + vp1 * vp1 + vp2 * vp2);
                    const float nn = nv + 1e-6f;
                    const float rn = fast_rcp(nn);
                    const float qq = (avc + bvc * rn) * w;
                    const float gdot = tc[3] * vp0 + tc[4] * vp1 + tc[5] * vp2;
                    const float dnn = -gdot * bvc * rn * rn + c0 + c1 * nn;
                    const float kk = dnn * fast_rcp(fmaxf(nv, 1e-30f)) * (nv > 0.f ? w : 0.f);
                    ua0 += tc[3] * qq + kk * vp0; ua1 += tc[4] * qq + kk * vp1; ua2 += tc[5] * qq + kk * vp2;
                }
            }
#undef SVNET_GATHER_TAB
            continue;
        }
        SVNET_GATHER_LOAD(0, 0);
        SVNET_GATHER_LOAD(min(1, last), 1);
        SVNET_GATHER_LOAD(min(2, last), 2);
        for (int n4 = 0; n4 < cnt; n4 += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = n4 + u;
                SVNET_GATHER_LOAD(min(n + 3, last), (u + 3) & 3);
                __builtin_amdgcn_sched_barrier(0);                     // the requests go out HERE, not next to their first use
                const float w = n < cnt ? 1.f : 0.f;                   // wave-uniform
#pragma unroll
                for (int q = 0; q < NCH; ++q) acc[q] += w * rw[u][q];
                const float* tc = tb[u];
                // dv' of the edge (source i -> this point): same arithmetic as edgeblock_bwd_vec_kernel
                const float vp0 = uj0 + tc[0], vp1 = uj1 + tc[1], vp2 = uj2 + tc[2];
                const float nv = fast_sqrt(vp0 * vp0 + vp1 * vp1 + vp2 * vp2);
                const float nn = nv + 1e-6f;
                const float rn = fast_rcp(nn);
                const float qq = (avc + bvc * rn) * w;
                const float gdot = tc[3] * vp0 + tc[4] * vp1 + tc[5] * vp2;
                const float dnn = -gdot * bvc * rn * rn + c0 + c1 * nn;
                const float kk = dnn * fast_rcp(fmaxf(nv, 1e-30f)) * (nv > 0.f ? w : 0.f);   // (a select, not a branch)
                ua0 += tc[3] * qq + kk * vp0; ua1 += tc[4] * qq + kk * vp1; ua2 += tc[5] * qq + kk * vp2;
            }
        }
    }
#undef SVNET_GATHER_LOAD
#undef SVNET_AT
    if (PACK) {   // fold the edge slots: lanes pg * Ov + o -> lane o
        for (int gg = 1; gg < pG; ++gg) {
            const int src = (lane + gg * Ov) & 63;
            const float t0 = __shfl(ua0, src, 64), t1 = __shfl(ua1, src, 64), t2 = __shfl(ua2, src, 64);   // all lanes take part
            if (lane < Ov) { ua0 += t0; ua1 += t1; ua2 += t2; }
        }
    }
    const int oV = Cs, oZ = oV + 3 * Cv;                               // msg row = [ds (Cs) | dve (3 Cv) | dz (9) | pad]
#pragma unroll
    for (int q = 0; q < NCH; ++q) {
        const int c = 64 * q + lane;
        if (c >= oZ + 9) continue;
        const float v = acc[q];
        if (c < oV) {
            if (OVF) atomicAdd(&ds_acc[j * Cs + c], v); else ds_acc[j * Cs + c] += v;
        } else if (c < oZ) {
            if (OVF) atomicAdd(&dv_acc[j * 3 * Cv + (c - oV)], v); else dv_acc[j * 3 * Cv + (c - oV)] += v;
        } else {
            const int z = c - oZ, a = z / 3, jz = z - a * 3;
            if (OVF) {
                atomicAdd(&acat[(j * 3 + a) * RW + 2 * Ov + jz], v);
            } else {
                const float cen = dzc[j * 9 + z];
                acat[(j * 3 + a) * RW + 2 * Ov + jz] = v - cen;
                acat[(j * 3 + a) * RW + 2 * Ov + 3 + jz] = cen;
            }
        }
    }
    if (lane < Ov) {
        const float ua[3] = {ua0, ua1, ua2};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (OVF) {
                atomicAdd(&acat[(j * 3 + a) * RW + lane], ua[a]);
            } else {
                const float cen = dvc[(j * 3 + a) * Ov + lane];
                acat[(j * 3 + a) * RW + lane] = ua[a] - cen;
                acat[(j * 3 + a) * RW + Ov + lane] = cen;
            }
        }
    }
    }   // items
}

}  // namespace

extern "C" int svnet_edgeblock_prepare_vec_f32(const float* W2, const float* scale2, const float* Wz, const float* scalez, int64_t Ov,
                                               int64_t Cv, float* wv, float* scv, void* stream) {
    SVNET_REQUIRE(W2 && scale2 && Wz && scalez && wv && scv && Ov > 0 && Cv > 0, SVNET_E_ARG, "svnet_edgeblock_prepare_vec_f32: bad arguments");
    const int64_t n = (2 * Ov + 6) * (Cv + 1);
    hipLaunchKernelGGL(prepare_vec_kernel, dim3(svnet_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, W2, scale2, Wz, scalez, (int)Ov,
                       (int)Cv, wv, scv);
    SVNET_CHECK_LAUNCH("prepare_vec_kernel");
    return SVNET_OK;
}

extern "C" int svnet_edgeblock_bwd_params_f32(const float* GXp, const float* GXc, const float* W1, const float* scale1, const float* W2,
                                              const float* scale2, const float* Wz, const float* scalez, int64_t Os, int64_t Ov,
                                              int64_t Cs, int64_t Cv, float* dW1, float* dscale1, float* dW2, float* dscale2, float* dWz,
                                              float* dscalez, void* stream) {
    SVNET_REQUIRE(GXp && GXc && W1 && scale1 && W2 && scale2 && Wz && scalez && dW1 && dscale1 && dW2 && dscale2 && dWz && dscalez,
                  SVNET_E_ARG, "svnet_edgeblock_bwd_params_f32: null pointer");
    SVNET_REQUIRE(Cs > 0 && Cs <= 64 && Cv > 0 && 2 * Cv <= 64 && Os > 0 && Ov > 0, SVNET_E_UNSUPPORTED,
                  "svnet_edgeblock_bwd_params_f32: needs Cs <= 64, 2*Cv <= 64");
    hipLaunchKernelGGL(bwd_params_kernel, dim3((unsigned)svnet_cdiv((Os + Ov + 3) * 64, 256)), dim3(256), 0, (hipStream_t)stream, GXp, GXc,
                       W1, scale1, W2, scale2, Wz, scalez, (int)Os, (int)Ov, (int)Cs, (int)Cv, dW1, dscale1, dW2, dscale2, dWz, dscalez);
    SVNET_CHECK_LAUNCH("bwd_params_kernel");
    return SVNET_OK;
}

extern "C" int svnet_knn_reverse_i32(const int64_t* idx, int64_t B, int64_t N, int64_t k, int32_t* rev_range, int32_t* rev_edge,
                                     int32_t* rev_src, int64_t chunk, int32_t* ovf_items, int32_t* ovf_count, void* stream) {
    SVNET_REQUIRE(idx && rev_range && rev_edge && rev_src && B >= 0 && N > 0 && k > 0, SVNET_E_ARG, "svnet_knn_reverse_i32: bad arguments");
    SVNET_REQUIRE(N <= REV_MAX_N, SVNET_E_UNSUPPORTED, "svnet_knn_reverse_i32: N=%lld > %d", (long long)N, REV_MAX_N);
    SVNET_REQUIRE(B * N * k < (int64_t)1 << 31, SVNET_E_UNSUPPORTED, "svnet_knn_reverse_i32: more than 2^31 edges");
    if (B == 0) return SVNET_OK;
    SVNET_REQUIRE((ovf_items == nullptr) == (ovf_count == nullptr) && (!ovf_items || chunk > 0), SVNET_E_ARG,
                  "svnet_knn_reverse_i32: ovf_items, ovf_count and chunk > 0 go together");
    hipLaunchKernelGGL(knn_reverse_kernel, dim3((unsigned)B), dim3(1024), (size_t)(N + 1024) * sizeof(int), (hipStream_t)stream, idx, (int)N,
                       (int)k, rev_range, rev_edge, rev_src, (int)chunk, ovf_items, ovf_count);
    SVNET_CHECK_LAUNCH("knn_reverse_kernel");
    return SVNET_OK;
}

extern "C" int svnet_edgeblock_bwd_gather_f32(const float* msg, const int32_t* rev_range, const int32_t* rev_edge, const int32_t* rev_src,
                                              const float* ut, const float* ub_tab, const float* ge_tab, const float* coef,
                                              const float* bcoef, int64_t Os, const float* dvc, const float* dzc, int64_t P, int64_t N,
                                              int64_t Cs, int64_t Cv, int64_t Ov, float* acat, int64_t acat_ld, float* ds_acc, float* dv_acc,
                                              const float* dbeta_perm, float* dbeta1, int64_t chunk, const int32_t* ovf_items,
                                              const int32_t* ovf_count, void* stream) {
    SVNET_REQUIRE(msg && rev_range && rev_edge && rev_src && ut && ub_tab && ge_tab && coef && bcoef && dvc && dzc && acat && ds_acc &&
                      dv_acc && dbeta_perm && dbeta1 && P > 0 && N > 0 && P % N == 0 && Os > 0, SVNET_E_ARG, "svnet_edgeblock_bwd_gather_f32: bad arguments");
    SVNET_REQUIRE(acat_ld >= 2 * Ov + 6, SVNET_E_ARG, "svnet_edgeblock_bwd_gather_f32: acat_ld < 2*Ov + 6");
    SVNET_REQUIRE(Cs > 0 && Cs <= 64 && Cv > 0 && 2 * Cv <= 64 && Ov > 0 && Ov <= 64, SVNET_E_UNSUPPORTED,
                  "svnet_edgeblock_bwd_gather_f32: needs Cs <= 64, 2*Cv <= 64, Ov <= 64");
    const int R = msg_stride(Cs, Cv, Ov);
    const int nch = (R + 63) / 64;
    const unsigned grid = (unsigned)svnet_cdiv(P, 4);
    const int bpc = ((P / N) % 8 == 0 && N % 4 == 0) ? (int)(N / 4) : 0;   // clouds in groups of 8, whole workgroups per cloud
    hipStream_t st = (hipStream_t)stream;
    SVNET_REQUIRE((ovf_items == nullptr) == (ovf_count == nullptr) && (!ovf_items || chunk > 0), SVNET_E_ARG,
                  "svnet_edgeblock_bwd_gather_f32: ovf_items, ovf_count and chunk > 0 go together (as given to svnet_knn_reverse_i32)");
    const int ch = ovf_items ? (int)chunk : 0;
    const unsigned ogrid = (unsigned)(grid < 1024 ? grid : 1024);        // the items are walked with a grid stride (their count is only known on the device)
#define SVNET_GATHER(NCH) do { if (Ov <= 32 && P * 3 * Ov < ((int64_t)1 << 30)) SVNET_GATHER_P(NCH, true); else SVNET_GATHER_P(NCH, false); } while (0)
#define SVNET_GATHER_P(NCH, PK)                                                                                                      \
    do {                                                                                                                             \
        hipLaunchKernelGGL((edgeblock_bwd_gather_kernel<NCH, false, PK>), dim3(grid), dim3(256), 0, st, msg, rev_range, rev_edge, rev_src, ut, \
                           ub_tab, ge_tab, coef, bcoef, (int)Os, dvc, dzc, P, bpc, (int)Cs, (int)Cv, (int)Ov, R, acat, (int)acat_ld, ds_acc, \
                           dv_acc, dbeta_perm, dbeta1, ch, ovf_items, ovf_count);                                                    \
        if (ovf_items)                                                                                                               \
            hipLaunchKernelGGL((edgeblock_bwd_gather_kernel<NCH, true, PK>), dim3(ogrid), dim3(256), 0, st, msg, rev_range, rev_edge, rev_src, ut, \
                               ub_tab, ge_tab, coef, bcoef, (int)Os, dvc, dzc, P, 0, (int)Cs, (int)Cv, (int)Ov, R, acat, (int)acat_ld, ds_acc, \
                               dv_acc, dbeta_perm, dbeta1, ch, ovf_items, ovf_count);                                                \
    } while (0)
    switch (nch) {
        case 1: SVNET_GATHER(1); break;
        case 2: SVNET_GATHER(2); break;
        default: SVNET_GATHER(3); break;
    }
#undef SVNET_GATHER
#undef SVNET_GATHER_P
    SVNET_CHECK_LAUNCH("edgeblock_bwd_gather_kernel");
    return SVNET_OK;
}

extern "C" int64_t svnet_edgeblock_msg_stride(int64_t Cs, int64_t Cv, int64_t Ov) { return msg_stride(Cs, Cv, Ov); }
