// The dispatch of svnet_gemm_f32, stated once: which kernel family a descriptor runs on and which template variant inside it.
// gemm_plan() is pure - it launches nothing and reads only the descriptor (sizes, strides, options, pointer alignments and which
// pointers are null); svnet_gemm_f32 executes what it returns, svnet_gemm_tier / svnet_gemm_variant report it.  The conditions exist
// nowhere else: a launch helper that re-derived one of them could drift from what the queries say.
#pragma once
#include <stdlib.h>

#include "common.h"

extern "C" size_t svnet_gemm_workspace_bytes(int64_t N, int64_t K);

constexpr int GEMM_BM = 64, GEMM_BN = 64, GEMM_BK = 16;     // the vector-ALU tile kernel's tile (gemm.hip)

// variant of the ternary TN kernel (also taken by svnet_edgeblock_wgrad_f32's affine form)
struct TernPlan {
    int nq;                 // 32-column q tiles per workgroup: 1, 2, 4, 5
    int ptiles_per_block;   // 1, 2, 4
    int lds_reduce;
    uint32_t qlist;         // != 0: compacted launch, one z group over exactly the live tiles (4 bits each, tile id + 1)
};

struct GemmPlan {
    int tier;               // SVNET_GEMM_*
    int variant;            // packed as include/svnet_hip.h documents
    bool empty;             // M == 0 || N == 0: nothing is launched
    // ROWS / ROWS_LDS / ROWS_SPLIT
    int cpb;                // columns per workgroup of the rows kernels: 32 NT
    bool a_vec;             // A rows 16-byte aligned and lda % 4 == 0
    bool packed;            // ROWS: B packed into the workspace first
    bool avec, deep;        // ROWS: mfma_rows_kernel<NT, AVEC, DEEP>
    bool lds_aligned;       // ROWS_LDS: mfma_rows2_kernel<1, aligned>
    int nj, w;              // ROWS_SPLIT: mfma_rows3_kernel<NJ, W>
    // TN_FP32
    int ip, jq;
    // TN_TERN
    TernPlan tern;
    // TILE
    int split;
    int64_t k_chunk;
};

// columns per workgroup (NT * 32) of the rows kernels.  Few row blocks (the classifier head: M = batch): narrow column tiles so that the
// grid still has tens of workgroups
inline int rows_cpb(int64_t M, int64_t N) { return (N <= 32 || M <= 512) ? 32 : (N <= 64 ? 64 : (N <= 128 ? 128 : 256)); }

// A partial tile mask names tiles 0..31 (the caller refuses one for Q > 1024).  Few tiles in use: one z group over exactly those (the A
// split is then shared) - when every live tile fits the 4-bit list, i.e. has an index of at most 14; a live tile above that keeps the
// launch uncompacted (the kernel skips cleared tiles either way).
inline TernPlan tern_plan(int64_t P, int64_t Q, uint32_t qmask) {
    TernPlan t;
    t.nq = Q <= 32 ? 1 : (Q <= 64 ? 2 : (Q <= 128 ? 4 : 5));
    const int ptiles = (int)svnet_cdiv(P, 32);
    t.ptiles_per_block = ptiles >= 3 ? 4 : ptiles;
    t.qlist = 0;
    if (qmask != 0xFFFFFFFFu) {
        int used = 0, top = -1;
        uint32_t list = 0;
        for (int i = 0; i < 32 && (int64_t)i * 32 < Q; ++i)
            if ((qmask >> i) & 1u) {
                if (used < 5 && i <= 14) list |= (uint32_t)(i + 1) << (4 * used);
                ++used;
                top = i;
            }
        if (used > 0 && used <= t.nq && top <= 14) t.qlist = list;
    }
    const int nsub = 4 / t.ptiles_per_block;
    const size_t lds = (size_t)(nsub - 1) * t.ptiles_per_block * t.nq * 1024 * sizeof(float);
    t.lds_reduce = (nsub > 1 && ptiles == t.ptiles_per_block && lds <= 64 * 1024) ? 1 : 0;
    return t;
}
inline int tern_variant(const TernPlan& t) { return t.nq | t.ptiles_per_block << 4 | t.lds_reduce << 8 | (t.qlist ? 1 : 0) << 9; }

inline int gemm_plan(const svnet_gemm_desc* desc, GemmPlan& p) {
    SVNET_REQUIRE(desc, SVNET_E_ARG, "svnet_gemm_f32: null descriptor");
    const svnet_gemm_desc& d = *desc;
    SVNET_REQUIRE(d.M >= 0 && d.N >= 0 && d.K >= 0, SVNET_E_ARG, "svnet_gemm_f32: negative size");
    SVNET_REQUIRE(d.C && d.B && (d.A || d.a_sign), SVNET_E_ARG, "svnet_gemm_f32: null operand");
    SVNET_REQUIRE(!d.a_sign || d.a_nz, SVNET_E_ARG, "svnet_gemm_f32: ternary A needs both planes");
    SVNET_REQUIRE(d.c_cs != 0 && d.ldc != 0, SVNET_E_ARG, "svnet_gemm_f32: zero C stride");
    p = GemmPlan();
    p.tier = SVNET_GEMM_TILE;
    p.variant = p.split = 1;
    p.k_chunk = GEMM_BK;
    p.empty = d.M == 0 || d.N == 0;
    if (p.empty) return SVNET_OK;
    const bool plain_epi = !d.col_scale && !d.bias && !d.mask && !d.col_sum && !d.a_scale;
    const uintptr_t ap = reinterpret_cast<uintptr_t>(d.A), wp = reinterpret_cast<uintptr_t>(d.workspace);

    // ---- ternary A (row-sliced planes over the reduction index): C(i,j) = sum_k tern(i,k) * B[k*b_rs + j]
    if (d.a_sign) {
        SVNET_REQUIRE(d.b_cs == 1 && plain_epi, SVNET_E_UNSUPPORTED, "svnet_gemm_f32: ternary A needs row-major B and a plain epilogue");
        SVNET_REQUIRE(d.tern_tile_mask == 0 || d.tern_tile_mask == 0xFFFFFFFFu || d.M <= 1024, SVNET_E_UNSUPPORTED,
                      "svnet_mfma_tn: a partial column-tile mask needs Q <= 1024 (got %lld)", (long long)d.M);
        p.tier = SVNET_GEMM_TN_TERN;
        p.tern = tern_plan(/*P=*/d.N, /*Q=*/d.M, d.tern_tile_mask ? d.tern_tile_mask : 0xFFFFFFFFu);
        p.variant = tern_variant(p.tern);
        return SVNET_OK;
    }
    // ---- reduction over rows with both operands fp32 rows: A(i,k) = A[k*a_cs + i], B(k,j) = B[k*b_rs + j]
    if (d.a_rs == 1 && d.b_cs == 1 && d.K >= 1024 && plain_epi && d.M <= 4096 && d.N <= 4096) {
        // the largest tile that still leaves >= 32 tiles: every row split adds one float atomic per output element, and with few tiles
        // the grid is filled by row splits ([512 x 127] as four 128 x 128 tiles: 128 splits, 50 of its 82 us in the atomics)
        const int64_t P = d.M, Q = d.N;
        auto tiles = [&](int ip, int jq) { return svnet_cdiv(P, 64 * ip) * svnet_cdiv(Q, 64 * jq); };
        if (P > 64 && Q > 64 && tiles(2, 2) >= 32) { p.ip = 2; p.jq = 2; }
        else if (P > 64 && (Q <= 64 || P >= Q) && tiles(2, 1) >= 32) { p.ip = 2; p.jq = 1; }
        else if (Q > 64 && tiles(1, 2) >= 32) { p.ip = 1; p.jq = 2; }
        else if (P > 64 && tiles(2, 1) >= 32) { p.ip = 2; p.jq = 1; }
        else { p.ip = 1; p.jq = 1; }
        p.tier = SVNET_GEMM_TN_FP32;
        p.variant = p.ip | p.jq << 4;
        return SVNET_OK;
    }
    p.cpb = rows_cpb(d.M, d.N);
    p.a_vec = (d.a_rs % 4 == 0) && (ap % 16 == 0);
    // ---- rows x exact-bf16 weights
    if (d.b_exact && d.a_cs == 1 && d.c_cs == 1 && d.M >= 16 && d.K >= 8) {
        SVNET_REQUIRE(d.a_rs < ((int64_t)1 << 24), SVNET_E_UNSUPPORTED, "svnet_mfma_rows: A row stride %lld >= 2^24 (32-bit tile offsets)", (long long)d.a_rs);
        p.packed = d.workspace && d.workspace_bytes >= svnet_gemm_workspace_bytes(d.N, d.K) && wp % 16 == 0;
        const int nt = p.cpb / 32;
        // the LDS-tiled kernel: many rows, pre-packed B whose padded column count covers whole 256-column groups
        static const bool rows2_off = getenv("SVNET_ROWS2_OFF") != nullptr;       // (diagnostic switch)
        if (nt == 8 && !rows2_off && p.packed && d.K >= 64 && d.M >= 4096 && d.N > 128) {
            p.tier = SVNET_GEMM_ROWS_LDS;
            p.lds_aligned = p.a_vec && (d.K & 3) == 0 && !(d.a_scale && (reinterpret_cast<uintptr_t>(d.a_scale) & 15) != 0);
            p.variant = p.lds_aligned ? 1 : 0;
            return SVNET_OK;
        }
        p.tier = SVNET_GEMM_ROWS;
        p.avec = p.a_vec && (d.K & 7) == 0;
        p.deep = d.K > 64;
        p.variant = nt | (p.avec ? 1 : 0) << 4 | (p.deep ? 1 : 0) << 5 | (p.packed ? 1 : 0) << 6;
        return SVNET_OK;
    }
    // ---- many rows x general fp32 weights: A and B split into three bf16 pieces each, the six leading products on the matrix cores (mfma_rows3_kernel)
    if (!d.b_exact && d.a_cs == 1 && d.c_cs == 1 && d.M >= 1024 && d.K >= 8 && d.N >= 8 && !d.col_scale && !d.mask && !d.col_sum && !d.a_scale &&
        d.workspace && d.workspace_bytes >= 3 * svnet_gemm_workspace_bytes(d.N, d.K)) {
        SVNET_REQUIRE(wp % 16 == 0 && svnet_gemm_workspace_bytes(d.N, d.K) % 16 == 0, SVNET_E_WORKSPACE,
                      "svnet_mfma_rows_split: needs 3 x svnet_gemm_workspace_bytes of 16-byte aligned workspace");
        SVNET_REQUIRE(d.a_rs < ((int64_t)1 << 24), SVNET_E_UNSUPPORTED, "svnet_mfma_rows_split: A row stride %lld >= 2^24", (long long)d.a_rs);
        p.tier = SVNET_GEMM_ROWS_SPLIT;
        p.nj = d.N <= 64 ? 1 : (d.N <= 128 ? 2 : 4);
        p.w = ((ap & 15) == 0 && (d.a_rs & 3) == 0 && (d.K & 3) == 0) ? 4 : (((ap & 7) == 0 && (d.a_rs & 1) == 0 && (d.K & 1) == 0) ? 2 : 1);
        p.variant = p.nj | p.w << 4;
        return SVNET_OK;
    }
    // ---- few outputs, long reduction: one wave per output
    if (d.M * d.N <= 8192 && d.K >= 128 && !d.mask && !d.col_sum && d.split_k <= 1) {
        p.tier = SVNET_GEMM_DOT;
        p.variant = 0;
        return SVNET_OK;
    }
    // ---- everything else: the vector-ALU tile kernel, K split over blockIdx.z (float atomics into a zero-filled C)
    const int64_t tiles = svnet_cdiv(d.M, GEMM_BM) * svnet_cdiv(d.N, GEMM_BN);
    int split = d.split_k;
    if (split <= 0) {
        split = 1;
        // few output tiles and a long reduction (the fp classifier head: [32 x 1022] . [1022 x 512] is 8 tiles - as 8 workgroups walking
        // K in 16-wide steps it took 210 us): K is cut into chunks of >= 64 until ~2048 / tiles workgroups exist
        if (tiles < 512 && d.K >= 256) {
            int64_t want = svnet_cdiv(2048, tiles);
            int64_t maxs = svnet_cdiv(d.K, 64);
            split = (int)(want < maxs ? want : maxs);
            if (split < 1) split = 1;
        }
    }
    p.k_chunk = svnet_cdiv(svnet_cdiv(d.K > 0 ? d.K : 1, split), GEMM_BK) * GEMM_BK;
    p.split = (int)svnet_cdiv(d.K > 0 ? d.K : 1, p.k_chunk);
    SVNET_REQUIRE(svnet_cdiv(d.M, GEMM_BM) <= 2147483647ll && svnet_cdiv(d.N, GEMM_BN) <= 65535 && p.split <= 65535, SVNET_E_UNSUPPORTED,
                  "svnet_gemm_f32: grid too large");
    p.variant = p.split;
    return SVNET_OK;
}
