// The dispatch of the binarized dense layer's two forward kernels, stated once: which template, launch form and grid a shape runs on.
// binlinear_plan() / binlinear_i8_plan() are pure - they launch nothing and read only the sizes; svnet_binlinear_fwd_f32 and
// svnet_binlinear_i8_fwd_f32 execute what they return, svnet_binlinear_tier / svnet_binlinear_i8_tier report it.  The conditions exist
// nowhere else: a launch helper that re-derived one of them could drift from what the queries say.
#pragma once
#include "common.h"

constexpr int BL_ROWS = 64;          // rows per workgroup tile of binlinear_fwd_kernel
constexpr int BL_MAX_WORDS = 34;     // 64-bit words per row that the tile's three planes may take in LDS (K <= 2176 per chunk)

constexpr int BL8_BM = 128;          // rows per workgroup of binlinear_i8_fwd_kernel
constexpr int BL8_KC = 128;          // columns per chunk
constexpr int BL8_LDA = BL8_KC + 16; // bytes per LDS row (36 dwords: 16-byte reads of 16 consecutive rows hit 64 distinct banks)

// The popcount kernel.  K > 2176 is processed in chunks of whole words; the integer count of the earlier chunks travels in y (int32),
// the last chunk applies scale and bias.  O > 256 (512 with two channels per thread) takes several launches over the output channels,
// each of which repeats the (cheap) packing pass.
inline int binlinear_plan(int64_t M, int64_t K, int64_t O, int64_t chunk, svnet_binlinear_plan& p) {
    SVNET_REQUIRE(M >= 0 && K > 0 && O > 0, SVNET_E_ARG, "svnet_binlinear_fwd_f32: bad sizes");
    SVNET_REQUIRE(K <= (1 << 20) && O <= (1 << 20), SVNET_E_UNSUPPORTED, "svnet_binlinear_fwd_f32: K=%lld, O=%lld too large", (long long)K,
                  (long long)O);
    const int64_t KWF = svnet_cdiv(K, 64);                    // words per full row (= weight plane row stride)
    const int64_t nchunk = svnet_cdiv(KWF, BL_MAX_WORDS);
    const int64_t wpc = svnet_cdiv(KWF, nchunk);              // words per chunk (<= 34)
    SVNET_REQUIRE(chunk >= 0 && chunk < nchunk, SVNET_E_ARG, "svnet_binlinear_tier: chunk %lld of %lld", (long long)chunk, (long long)nchunk);
    p = svnet_binlinear_plan();
    p.nchunk = (int)nchunk;
    p.wpc = (int)wpc;
    p.chunk = (int)chunk;
    p.col0 = chunk * wpc * 64;
    p.kc = (int)((chunk + 1 == nchunk) ? K - p.col0 : wpc * 64);
    p.kw = (int)svnet_cdiv(p.kc, 64);
    p.ymode = (chunk > 0 ? 1 : 0) | (chunk + 1 < nchunk ? 2 : 0);
    p.lds_bytes = (size_t)3 * BL_ROWS * p.kw * sizeof(uint64_t);
    const int64_t tiles = svnet_cdiv(M, BL_ROWS);
    const int64_t groups = svnet_cdiv(O, 256);               // 256-channel groups
    // two output channels per thread only when there are row tiles in plenty (and the weight words of both fit the registers: KW <= 8);
    // fewer tiles take a one-launch split over the output channels (PPM = 1) so that the grid still fills the chip
    const bool two = p.kw <= 8 && O > 256 && tiles * groups > 256 * 16;
    p.kwm = p.kw <= 2 ? 2 : (p.kw <= 4 ? 4 : (p.kw <= 8 ? 8 : (p.kw <= 16 ? 16 : BL_MAX_WORDS)));
    p.ppm = two ? 2 : 1;
    if (!two && tiles <= 8 && O > 32) {
        // small M: one launch, ceil(O/32) workgroups per row tile (each repeats the cheap packing pass of its tile)
        p.form = SVNET_BINLINEAR_TILE_SPLIT;
        p.og_shift = 5;
        p.o_blocks = (int)svnet_cdiv(O, 32);
        p.launches = 1;
        p.grid_tiles = tiles;
    } else if (!two && O > 256 && tiles * groups <= 256 * 16) {
        // a few hundred row tiles (conv5: 512 tiles x 512 channels): one workgroup per (tile, 256 channels) in ONE launch, so that the
        // grid has >= 4 workgroups per CU (2 per CU - 2 waves per SIMD - left every load latency of the packing pass exposed)
        p.form = SVNET_BINLINEAR_GROUPS;
        p.og_shift = 8;
        p.o_blocks = (int)groups;
        p.launches = 1;
        p.grid_tiles = tiles;
    } else {
        // one launch per 256 PPM output channels, the grid capped at 2048 row tiles (the kernel's tile loop takes the rest)
        p.form = SVNET_BINLINEAR_LOOP;
        p.og_shift = 5;
        while ((1 << p.og_shift) < O && p.og_shift < 8) ++p.og_shift;
        p.o_blocks = 1;
        p.launches = (int)svnet_cdiv(O, 256 * p.ppm);
        p.grid_tiles = tiles < 256 * 8 ? tiles : 256 * 8;
    }
    if (M == 0) p.launches = 0;
    return SVNET_OK;
}

// The int8 matrix-core kernel: 128, 256 or 512 output channels per workgroup (16 waves: one, two or four 32-column tiles per wave),
// further column groups over grid.y.
inline int binlinear_i8_plan(int64_t M, int64_t K, int64_t O, int col_sums, svnet_binlinear_i8_plan& p) {
    SVNET_REQUIRE(M >= 0 && K > 0 && O > 0, SVNET_E_ARG, "svnet_binlinear_i8_fwd_f32: bad sizes");
    SVNET_REQUIRE(K < (1 << 24) && O < (1 << 24), SVNET_E_UNSUPPORTED, "svnet_binlinear_i8_fwd_f32: K=%lld, O=%lld too large", (long long)K, (long long)O);
    SVNET_REQUIRE(!col_sums || K <= 46340, SVNET_E_UNSUPPORTED, "svnet_binlinear_i8_fwd_f32: column sums need K <= 46340 (got %lld)", (long long)K);
    p = svnet_binlinear_i8_plan();
    p.kp = (int)(svnet_cdiv(K, BL8_KC) * BL8_KC);
    p.nchunks = p.kp / BL8_KC;
    p.ntw = O <= 128 ? 1 : (O <= 256 ? 2 : 4);
    p.grid_x = svnet_cdiv(M, BL8_BM);
    p.grid_y = (int)svnet_cdiv(O, 128 * p.ntw);
    p.lds_bytes = (size_t)BL8_BM * BL8_LDA + (size_t)128 * p.ntw * BL8_LDA + 3 * BL8_BM * 2 * sizeof(uint64_t);
    return SVNET_OK;
}
