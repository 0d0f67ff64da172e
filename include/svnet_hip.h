/*
 * svnet_hip.h — C ABI of libsvnet_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * SVNet hot path.  The reference (hellozhuo/svnet) is pure Python/PyTorch and has no FFI of its
 * own; each entry point below names the reference op chain it replaces (file:line relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless stated otherwise; tensors are dense row-major fp32,
 *     indices int64; "rows" M is the product of all leading dimensions
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never allocates or
 *     frees device memory and keeps no device state between calls
 *   - `stream` is a hipStream_t (passed as void*); calls are asynchronous and ordered on it
 *   - return value: 0 = ok, <0 = error (SVNET_E_*); svnet_last_error() gives a message for the
 *     calling thread.  Nothing throws across the ABI.
 */
#ifndef SVNET_HIP_H
#define SVNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVNET_OK 0
#define SVNET_E_ARG (-1)       /* null pointer / negative size / inconsistent arguments */
#define SVNET_E_UNSUPPORTED (-2) /* shape outside what the kernels were built for */
#define SVNET_E_WORKSPACE (-3) /* workspace too small */
#define SVNET_E_LAUNCH (-4)    /* HIP reported an error at launch */

/* Grid-wide sums are spread over slices (workgroup w adds to slice w % SVNET_RED_SLICES): a thousand float / double atomics onto one
 * address are served one after the other at the memory side and set the pace of the reduction kernels.                            */
#define SVNET_RED_SLICES 16
/* Length (elements) of a SLICED accumulator of L sums (svnet_colstats_f64, svnet_bn_act_bwd_reduce_f32, svnet_vbn_bwd_reduce_f32,
 * svnet_bn_pool_bwd_f32, the col_sums of svnet_binlinear_i8_fwd_f32): [L totals | SVNET_RED_SLICES x L slices | 2 spare], zero-filled by
 * the caller.  The REDUCING entry point only fills the slices; the totals (first L elements) are written by the entry point that
 * CONSUMES the accumulator (svnet_bn_finalize_f32, svnet_bn_act_bwd_apply_f32, svnet_vbn_bwd_apply_f32, the apply pass of
 * svnet_bn_pool_bwd_f32; svnet_vbn_fwd_stats_f32 reads the slices and writes no totals) or by svnet_slices_sum_f32 / _f64 - i.e. the
 * slices are handed from their adders to their reader across a kernel boundary of the stream, never inside a launch.               */
#define SVNET_SLICED_LEN(L) ((SVNET_RED_SLICES + 1) * (L) + 2)
/* buf[0:L] = sum over the slices of a sliced accumulator (for a caller that reads the totals itself). */
int svnet_slices_sum_f32(float* buf, int64_t L, void* stream);
int svnet_slices_sum_f64(double* buf, int64_t L, void* stream);

/* ABI version = 100 * round-of-change + serial.  It changes whenever an entry point gains / loses an argument or a caller-owned buffer
 * changes its required length (200: sliced accumulators, SVNET_SLICED_LEN; 400: this header; 401: the totals of a sliced accumulator are
 * written by its consumer, svnet_slices_sum_*; 402: GX of svnet_v2s_bwd_*, gw of svnet_xyzblock_bwd_f32 and col_sum of svnet_gemm_f32 are sliced accumulators; 403: svnet_binweight_grad_f32 takes sliced inputs; 421: svnet_three_nn_f32, svnet_three_interpolate_f32; 422: svnet_ball_query_f32, svnet_group_points_f32; 423: svnet_vlinear_stats_f32 is gone; 424: svnet_edgeblock_fwd_tier, svnet_edgeblock_bwd_tier, svnet_edgeblock_wgrad_tier, svnet_xyzblock_tier; 425: svnet_pointset_reverse_i32, svnet_three_interpolate_bwd_f32, svnet_group_points_bwd_f32; 426: wbt of svnet_edgeblock_wbt_bf16 is 512 values longer, the all-zero fragment; 427: svnet_ball_query_msg_f32, svnet_group_points_msg_f32, svnet_group_points_msg_bwd_f32; 428: svnet_sa_fold_f32, svnet_sa_fused_f32; 429: svnet_fp_fused_f32, svnet_fp_fused_supported, svnet_fp_fused_rows_tile; 430: svnet_sa_global_f32, svnet_sa_global_supported, svnet_sa_global_rows_tile; 431: svnet_pool_gather_attr_f32, the attribute fields attr, A, attr_vectors, attr_out at the end of svnet_batch_desc; 432: svnet_vn_fold_f32, svnet_vn_tables_f32, svnet_vn_edge_mean_f32, svnet_vn_supported, svnet_vn_workspace_bytes; 433: svnet_vn_point_supported, svnet_vn_point_workspace_bytes, svnet_vn_point_fold_f32, svnet_vn_point_f32, svnet_vn_cloud_mean_f32, svnet_vn_std_pool_supported, svnet_vn_std_pool_workspace_bytes, svnet_vn_std_pool_f32; 434: svnet_vn_edge2_supported, svnet_vn_edge2_mean_f32, svnet_vn_std_coords_supported, svnet_vn_std_coords_f32; 435: svnet_vn_cross_supported, svnet_vn_cross_fold_f32, svnet_vn_edge_cross_mean_f32, svnet_vn_point_norm_supported, svnet_vn_point_norm_fold_f32, svnet_vn_point_norm_f32; 436: svnet_gemm_tier, svnet_gemm_variant; 437: svnet_vn_point_wide_supported, svnet_vn_point_wide_workspace_bytes, svnet_vn_point_wide_fold_f32, svnet_vn_point_wide_f32, svnet_vn_point_norm_wide_supported, svnet_vn_point_norm_wide_fold_f32, svnet_vn_point_norm_wide_f32, svnet_vn_cloud_mean_wide_f32, svnet_vn_std_pool_wide_supported, svnet_vn_std_pool_wide_workspace_bytes, svnet_vn_std_pool_wide_f32, svnet_vn_std_coords_wide_supported, svnet_vn_std_coords_wide_f32; 438: svnet_bi_packed_bytes, svnet_bi_fold_f32, svnet_bi_chain_supported, svnet_bi_chain_rows_tile, svnet_bi_chain_workspace_bytes, svnet_bi_chain_f32; 439: svnet_binlinear_tier, svnet_binlinear_i8_tier).  svnet_version() returns the value the
 * library was BUILT with: a caller compiled against another header must refuse to run (svnet_amd/_lib.py does).                   */
#define SVNET_ABI_VERSION 439
int svnet_version(void);
const char* svnet_last_error(void);

/* A gate MLP run by extra workgroups of a coefficient launch (svnet_edgeblock_coeffs_f32, svnet_xyzblock_coeffs_f32,
 * svnet_edgeblock_bwd_coeffs_f32: their last argument, NULL = none): the arguments of svnet_gate_mlp_fwd_f32 / svnet_gate_mlp_bwd_f32
 * below.  The gate and the coefficients only share their inputs; as two launches they were two latency-bound links of every fused
 * layer's critical path. */
typedef struct svnet_gate_fwd_job {
    const float* gin; const double* gin_f64; float* gin_out; float in_scale; const float* W0; const float* W2;
    int64_t B, Cin, H, Ov; float* h; float* gate;
    const float* rows; int64_t R;   /* optional third source of the MLP's input (gin and gin_f64 NULL): gin_out[b,:] = mean over the R
                                       rows of cloud b of rows [B*R, Cin] (sv_layers.py:179: s.mean over the points), kept for the backward */
} svnet_gate_fwd_job;
typedef struct svnet_gate_bwd_job {
    const float* dgate; const float* gate; const float* h; const float* gin; float in_scale; const float* W0; const float* W2;
    int64_t B, Cin, H, Ov; float out_scale; float* dgin; float* dW0; float* dW2;
} svnet_gate_bwd_job;

/* ------------------------------------------------------------------ k-NN  (models/utils/sv_util.py:19-25, knn)
 * x is addressed as x[b*sb + n*sn + c*sc] (the [B,C,N] tensor the reference passes, any strides).
 * xx_mode: 0 = ||x||^2 summed the way ATen reduces an OUTER dim (contiguous [B,C,N]),
 *          1 = the way ATen reduces the CONTIGUOUS dim (transposed view of [B,N,C])   
 * idx_out: [B,N,k] int64, cloud-local neighbour ids, nearest first (self first), ties -> lowest id.
 * Bit-exact against the reference's torch-CPU result for C <= 384, N <= 32768, k <= 128 (k <= N); anything
 * past those limits returns SVNET_E_UNSUPPORTED.                                                        */
size_t svnet_knn_workspace_bytes(int64_t B, int64_t N, int64_t C);
int svnet_knn_f32(const float* x, int64_t B, int64_t N, int64_t C, int64_t sb, int64_t sn, int64_t sc,
                  int xx_mode, int k, int64_t* idx_out, void* workspace, size_t workspace_bytes, void* stream);
/* The feature-space graph of get_graph_feature_sv (sv_util.py:100-101): k-NN on the rows cat[s, v.view(B,N,3Cv)] read from
 * s [B,N,Cs] and v [B,N,Cv3] where they lie (no concatenated copy); same arithmetic as svnet_knn_f32 with xx_mode 1.
 * Workspace: svnet_knn_workspace_bytes(B, N, Cs + Cv3).                                               */
int svnet_knn_sv_f32(const float* s, int64_t Cs, const float* v, int64_t Cv3, int64_t B, int64_t N, int k, int64_t* idx_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The candidate table of a k-NN call prepared by the PRODUCER of the features (the apply pass of the previous fused level): the k-NN is
 * on the forward's critical path and its first kernel only re-reads, squares and transposes what that pass has just written
 * (sv_dgcnn_cls.py:55-65: svpool(conv_l(..)) -> get_graph_feature_sv -> knn).  svnet_knn_table_fusable: 1 when the table of (B, N, C)
 * is the channel-major one the producers write and N % 32 == 0.  svnet_edgeblock_apply_knn_f32 / svnet_xyzblock_apply_knn_f32: the apply
 * pass of svnet_edgeblock_apply_f32 / svnet_xyzblock_apply_f32 (same arguments, bit-identical s_out / v_out / slices) that also fills
 * knn_workspace (svnet_knn_workspace_bytes(P / N, N, Os + 3 Ov)) with the table and the ||x||^2 of the rows cat[s, v.view(3 Ov)]
 * (sv_util.py:100; ATen's contiguous-row recipe, bit for bit what svnet_knn_sv_f32 computes).  svnet_knn_from_table_f32: the k-NN
 * proper on such a workspace - idx_out as svnet_knn_f32.                                                                            */
int svnet_knn_table_fusable(int64_t B, int64_t N, int64_t C);
int svnet_knn_from_table_f32(const void* workspace, size_t workspace_bytes, int64_t B, int64_t N, int64_t C, int k, int64_t* idx_out,
                             void* stream);
int svnet_edgeblock_apply_knn_f32(const int32_t* n_max, const int32_t* n_min, const float* mv, const float* mvn, const float* coef,
                                  const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope, float* s_out, float* v_out,
                                  float* s_cat, int64_t s_ld, float* v_cat, int64_t v_ld, void* knn_workspace, size_t knn_workspace_bytes,
                                  void* stream);
int svnet_xyzblock_apply_knn_f32(const float* y_max, const float* y_min, const float* mv, const float* mvn, const float* coef,
                                 const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope, float* s_out, float* v_out,
                                 float* s_cat, int64_t s_ld, float* v_cat, int64_t v_ld, void* knn_workspace, size_t knn_workspace_bytes,
                                 void* stream);

/* ------------------------------------------------------------------ edge features from xyz
 * (sv_util.py:28-62 get_graph_feature, :64-88 get_graph_feature_cross)
 * x: contiguous [B,3m,N] (channel = m*3+d).  idx: [B,N,k] cloud-local.
 * mode 0: out[b,n,j,d,:] = [x_j-x_i (m), x_i (m)]            -> [B,N,k,3,2m]
 * mode 1: (first=True)    [x_j-x_i, mean_j(x_j-x_i)]          -> [B,N,k,3,2m]
 * mode 2: (cross)         [x_j-x_i, x_i, x_j x x_i]           -> [B,N,k,3,3m]                   */
int svnet_edge_xyz_f32(const float* x, const int64_t* idx, int64_t B, int64_t N, int64_t k, int64_t m, int mode,
                       float* out, void* stream);

/* ------------------------------------------------------------------ edge features from (s,v) tables
 * (sv_util.py:90-116 get_graph_feature_sv; backward = autograd of :106-114, an index_put accumulate)
 * table: [B*N, G, F]; out: [B*N*k, G, 2F] with out[e,g,:F] = t[j,g,:]-t[i,g,:], out[e,g,F:] = t[i,g,:].
 * (G,F) = (1,Cs) for scalars, (3,Cv) for vectors.  idx_is_global: idx already holds b*N+j row ids. */
int svnet_edge_diffcat_fwd_f32(const float* table, const int64_t* idx, int idx_is_global, int64_t B, int64_t N,
                               int64_t k, int64_t G, int64_t F, float* out, void* stream);
/* d_table must be zero-filled by the caller; gradients are accumulated with float atomics.          */
int svnet_edge_diffcat_bwd_f32(const float* d_out, const int64_t* idx, int idx_is_global, int64_t B, int64_t N,
                               int64_t k, int64_t G, int64_t F, float* d_table, void* stream);

/* ------------------------------------------------------------------ generic fp32 GEMM  C[M,N] = epi(sum_k A(i,k) B(k,j))
 * Used for every dense contraction of the path: F.linear of sv_layers.py:31,49 and the autograd
 * products of its backward.  A(i,k) = A[i*a_rs + k*a_cs] * a_scale[k], B(k,j) = B[k*b_rs + j*b_cs],
 * C(i,j) = C[i*ldc + j*c_cs].
 * Bit-planes are "row-sliced": word [(r >> 6) * W + c] holds bit (r & 63) of column c for rows 64*(r>>6)..+63
 * (W = number of columns; rows beyond the tensor are 0).  They appear in two places:
 *   - a_sign/a_nz != NULL: the A operand is ternary, A(i,k) = nz ? (sign ? +1 : -1) : 0, sliced over the
 *     REDUCTION index k with W = M columns i (this is x_b^T of a binarized layer: weight-gradient products);
 *   - mask: STE mask of the output, sliced over the output rows i with W = N columns.
 * b_exact != 0 promises that every B value is exactly representable in bf16 (sign weights: -1, 0, +1), which
 * lets the tall-and-skinny product run on bf16 MFMA with an exact 3-way split of A.
 * Epilogue, in this order: *alpha, *col_scale[j], +bias[j], *mask(i,j), then col_sum[j] += sum_i C(i,j) (float atomics into
 * the slices of a SLICED accumulator of N floats, SVNET_SLICED_LEN(N): caller zero-fills, totals by svnet_slices_sum_f32), then
 * store (or accumulate when accumulate != 0).                                                                 */
typedef struct svnet_gemm_desc {
    int64_t M, N, K;
    const float* A; int64_t a_rs, a_cs;
    const float* a_scale;
    const uint64_t* a_sign; const uint64_t* a_nz;
    const float* B; int64_t b_rs, b_cs;
    int b_exact;
    float* C; int64_t ldc, c_cs;
    float alpha;
    const float* col_scale;
    const float* bias;
    const uint64_t* mask;
    float* col_sum;
    int split_k;       /* 0 = choose automatically (vector-ALU kernel only) */
    int accumulate;    /* C += result */
    uint32_t tern_tile_mask; /* ternary A only: bit t set = rows [32t, 32t+32) of A^T (output rows i) may be non-zero; 0 = all.
                                Cleared tiles are skipped: their outputs are left untouched (use with accumulate on zeros).
                                A partial mask (neither 0 nor all ones) needs M <= 1024.  When it has at most as many live tiles as one
                                workgroup takes (NQ below) and every live tile has an index of at most 14, the launch is compacted
                                to one column group over exactly the live tiles; a live tile 15 .. 31 keeps it uncompacted.       */
    void* workspace;   /* optional scratch; with b_exact, >= svnet_gemm_workspace_bytes(N, K) lets the MFMA path pack B once as */
    size_t workspace_bytes; /* bf16 [N][K] (k contiguous) so that its LDS staging is plain 16-byte copies                       */
} svnet_gemm_desc;
size_t svnet_gemm_workspace_bytes(int64_t N, int64_t K);
int svnet_gemm_f32(const svnet_gemm_desc* desc, void* stream);
/* Which kernel a descriptor runs on.  Both are pure host functions of the descriptor (sizes, strides, options, which pointers are null
 * and how the non-null ones are aligned; nothing is dereferenced or launched), and svnet_gemm_f32 executes exactly what they report.
 * A descriptor that svnet_gemm_f32 refuses gives its negative SVNET_E_* code (and the same svnet_last_error) from both.  An empty
 * product (M == 0 or N == 0) launches nothing and reports SVNET_GEMM_TILE, variant 1.
 * svnet_gemm_tier: the family.
 *   SVNET_GEMM_TN_TERN    ternary A planes (weight gradients of the binarized layers): mfma_tn_tern_kernel
 *   SVNET_GEMM_TN_FP32    a_rs == 1, b_cs == 1, K >= 1024, M, N <= 4096, plain epilogue: mfma_tn2_kernel
 *   SVNET_GEMM_ROWS       b_exact, a_cs == 1, c_cs == 1, M >= 16, K >= 8: mfma_rows_kernel
 *   SVNET_GEMM_ROWS_LDS   as ROWS with B packed into the workspace, M >= 4096, N > 128, K >= 64: mfma_rows2_kernel
 *   SVNET_GEMM_ROWS_SPLIT general B, a_cs == 1, c_cs == 1, M >= 1024, K >= 8, N >= 8, alpha / bias / accumulate only, a workspace of
 *                         3 x svnet_gemm_workspace_bytes: mfma_rows3_kernel
 *   SVNET_GEMM_DOT        M * N <= 8192, K >= 128, no mask, no col_sum, split_k <= 1: gemm_dot_kernel
 *   SVNET_GEMM_TILE       everything else: gemm_kernel on the vector ALUs
 * svnet_gemm_variant: the template choice inside the family, packed as
 *   TN_TERN     NQ (1, 2, 4, 5) | ptiles_per_block (1, 2, 4) << 4 | lds_reduce << 8 | compacted tile list << 9
 *   TN_FP32     IP | JQ << 4                                        (mfma_tn2_kernel<IP, JQ>)
 *   ROWS        NT (1, 2, 4, 8) | AVEC << 4 | DEEP << 5 | B packed << 6
 *   ROWS_LDS    1 = aligned float4 A loads, 0 = per-element A loads
 *   ROWS_SPLIT  NJ (1, 2, 4) | A load width (4, 2, 1) << 4
 *   DOT         0
 *   TILE        the number of K splits (1 = no split: plain stores, no zero-fill launch)                                          */
#define SVNET_GEMM_TN_TERN 1
#define SVNET_GEMM_TN_FP32 2
#define SVNET_GEMM_ROWS 3
#define SVNET_GEMM_ROWS_LDS 4
#define SVNET_GEMM_ROWS_SPLIT 5
#define SVNET_GEMM_DOT 6
#define SVNET_GEMM_TILE 7
int svnet_gemm_tier(const svnet_gemm_desc* desc);
int svnet_gemm_variant(const svnet_gemm_desc* desc);

/* ------------------------------------------------------------------ binarized layers (sv_layers.py:20-53 Linear, :55-78 Conv1d)
 * Weight preparation (sign(W) with sign(0)=0, clamp/STE mask |W|<=1.2):
 *   w_sign/w_nz: [O, Kw] uint64 bit-planes (Kw = ceil(K/64)), w_b: [O,K] fp32 in {-1,0,1},
 *   w_eff: [O,K] = scale[o]*w_b (NULL allowed), any output pointer may be NULL.                    */
int svnet_binweight_prepare_f32(const float* W, const float* scale, int64_t O, int64_t K, uint64_t* w_sign,
                                uint64_t* w_nz, float* w_b, float* w_eff, void* stream);
/* y[m,o] = scale[o] * sum_k sgn(x[m,k]+beta[k]) * sgn(W[o,k])  (+bias[o]) by XNOR/popcount on ternary
 * bit-planes.  x row stride ldx.  Optional outputs (NULL to skip), each a row-sliced plane [ceil(M/64), K]
 * uint64 (layout: see svnet_gemm_desc):  x_sign, x_nz (sign / non-zero planes of the binarized input),
 * x_ste (|x+beta| <= 1.2).  3 bits per input element replace the saved fp32 input in training.        */
int svnet_binlinear_fwd_f32(const float* x, int64_t ldx, const float* beta, const uint64_t* w_sign,
                            const uint64_t* w_nz, const float* scale, const float* bias, int64_t M, int64_t K,
                            int64_t O, float* y, uint64_t* x_sign, uint64_t* x_nz, uint64_t* x_ste, void* stream);
/* Which kernel svnet_binlinear_fwd_f32 runs a shape on.  A pure host function of the sizes: nothing is dereferenced or launched, `plan` is
 * a HOST pointer, and svnet_binlinear_fwd_f32 executes exactly what it reports.  Sizes that svnet_binlinear_fwd_f32 refuses give its
 * negative SVNET_E_* code (and the same svnet_last_error).  K > 2176 (34 words of 64 columns: what a row tile's planes may take in LDS)
 * is processed in `nchunk` column chunks of `wpc` words, the last one possibly shorter; the integer count of the earlier chunks
 * travels in y as int32.  `chunk` (0 .. nchunk - 1) selects the chunk that the fields from `chunk` on describe.                      */
#define SVNET_BINLINEAR_TILE_SPLIT 1 /* at most 8 row tiles, O > 32: one launch, ceil(O / 32) workgroups of 32 channels per row tile        */
#define SVNET_BINLINEAR_GROUPS 2     /* O > 256, tiles * ceil(O / 256) <= 4096: one launch, one workgroup per (tile, 256 channels)            */
#define SVNET_BINLINEAR_LOOP 3       /* everything else: one launch per 256 * ppm channels (o_base), the grid capped at 2048 row tiles      */
typedef struct svnet_binlinear_plan {
    int nchunk;            /* column chunks: ceil(ceil(K / 64) / 34)                                            */
    int wpc;               /* 64-bit words per chunk: ceil(ceil(K / 64) / nchunk)                               */
    int chunk;             /* the chunk described from here on                                                  */
    int64_t col0;          /* its first column: chunk * wpc * 64                                                */
    int kc;                /* its columns                                                                       */
    int kw;                /* its words: ceil(kc / 64)                                                          */
    int kwm;               /* the kernel template's word bound: 2, 4, 8, 16 or 34 (34: the WIDE form, kw > 16)  */
    int ppm;               /* output channels per thread: 2 when kw <= 8, O > 256 and tiles * ceil(O / 256) > 4096, else 1 */
    int form;              /* SVNET_BINLINEAR_TILE_SPLIT / _GROUPS / _LOOP                                      */
    int og_shift;          /* log2 of the threads that share one row: 5 (TILE_SPLIT), 8 (GROUPS), 5 .. 8 by O (LOOP) */
    int o_blocks;          /* workgroups per row tile                                                           */
    int launches;          /* kernel launches of this chunk (0 when M == 0)                                     */
    int64_t grid_tiles;    /* row tiles the grid takes at once (grid = grid_tiles * o_blocks workgroups)        */
    int ymode;             /* bit 0: add the int32 count kept in y, bit 1: keep the count instead of scaling it */
    size_t lds_bytes;      /* dynamic LDS per workgroup: 3 planes x 64 rows x kw words                          */
} svnet_binlinear_plan;
int svnet_binlinear_tier(int64_t M, int64_t K, int64_t O, int64_t chunk, svnet_binlinear_plan* plan);
/* The same layer on the matrix cores, for many rows (v_mfma_i32_32x32x32_i8 on int8 ternary operands, exact int32 counts: outputs
 * and saved planes identical to svnet_binlinear_fwd_f32).  w_i8 = svnet_binweight_pack_i8(W): sign(W) as int8 [O][128*ceil(K/128)],
 * every 128-column chunk in the kernel's reduction order, zero padded (svnet_binweight_i8_bytes bytes).                           */
size_t svnet_binweight_i8_bytes(int64_t O, int64_t K);
int svnet_binweight_pack_i8(const float* W, int64_t O, int64_t K, int8_t* w_i8, void* stream);
/* col_sums (NULL to skip): a sliced accumulator of 2*O doubles (SVNET_SLICED_LEN(2*O), zero-filled): sum_m y[m,o] and sum_m y[m,o]^2 - the batch statistics of the BatchNorm that follows
 * (sv_layers.py:189), from the exact integer counts, so that the output is not read again for them (feed svnet_bn_finalize_f32).      */
int svnet_binlinear_i8_fwd_f32(const float* x, int64_t ldx, const float* beta, const int8_t* w_i8, const float* scale,
                               const float* bias, int64_t M, int64_t K, int64_t O, float* y, uint64_t* x_sign, uint64_t* x_nz,
                               uint64_t* x_ste, double* col_sums, void* stream);
/* Which template and grid svnet_binlinear_i8_fwd_f32 / svnet_binlinear_i8_cloud_fwd_f32 run a shape on (col_sums != 0: with column
 * sums): a pure host function like svnet_binlinear_tier, `plan` a HOST pointer; refused sizes give their SVNET_E_* code.            */
typedef struct svnet_binlinear_i8_plan {
    int ntw;               /* 32-column tiles per wave: 1 (O <= 128), 2 (O <= 256), 4; a workgroup takes 128 * ntw channels */
    int64_t grid_x;        /* row blocks of 128                                                                 */
    int grid_y;            /* column groups of 128 * ntw channels                                               */
    int nchunks;           /* 128-column chunks of K                                                            */
    int kp;                /* 128 * nchunks: the row length of w_i8                                             */
    size_t lds_bytes;      /* dynamic LDS per workgroup                                                         */
} svnet_binlinear_i8_plan;
int svnet_binlinear_i8_tier(int64_t M, int64_t K, int64_t O, int col_sums, svnet_binlinear_i8_plan* plan);
/* The same layer when part of its input is CONSTANT over the rows of a cloud (the broadcast half of a concatenation:
 * sv_dgcnn_partseg.py:115-118 `repeat` + `cat`, sv_pointnet_cls.py:43-52 `expand_as` + `svcat`): x [M, K] holds only the per-point
 * columns, cloud_n [M / rows_per_cloud, O] the integer counts (as floats) of the per-cloud columns - svnet_binlinear_fwd_f32 over the
 * B per-cloud rows with scale = 1 -, and y[m,o] = scale[o] * (count(x[m]) + cloud_n[m / rows_per_cloud, o]) (+ bias).  The sum of the two
 * counts is the count over the full row: outputs and col_sums identical to the product over the materialised concatenation.      */
int svnet_binlinear_i8_cloud_fwd_f32(const float* x, int64_t ldx, const float* beta, const int8_t* w_i8, const float* scale,
                                     const float* bias, int64_t M, int64_t K, int64_t O, float* y, uint64_t* x_sign, uint64_t* x_nz,
                                     uint64_t* x_ste, double* col_sums, const float* cloud_n, int64_t rows_per_cloud, void* stream);
/* Chain rule from GX[o,k] = sum_m g[m,o] x_eff[m,k] to the parameters of a bw layer (App. C2):
 *   dW[o,k] = scale[o]*GX[o,k]*[|W[o,k]|<=1.2],  dscale[o] = sum_k w_b[o,k]*GX[o,k];  accumulate != 0 adds to dW/dscale. */
/* gx_sliced != 0: GX is a sliced accumulator of O*K floats (SVNET_SLICED_LEN) whose slices are added up on the way in.
 * sum_buf / sum_len (NULL / 0 to skip): another sliced accumulator whose totals this launch leaves in its first sum_len elements
 * (the dL/dbeta column sums of the same layer's input-gradient product: saves a svnet_slices_sum_f32 launch).                       */
int svnet_binweight_grad_f32(const float* GX, const float* W, const float* scale, int64_t O, int64_t K,
                             float* dW, float* dscale, int accumulate, int gx_sliced, float* sum_buf, int64_t sum_len, void* stream);

/* ------------------------------------------------------------------ fused edge block (tier 2)
 * One pass over the edges of a BINARIZED edge layer, never materialising an edge tensor:
 *   get_graph_feature_sv (sv_util.py:90-116) -> SVBlock (sv_layers.py:172-196) -> svpool (sv_util.py:118-132).
 * Inputs are point tables: s [P,Cs], v [P,3,Cv], idx [P,k] (cloud-local), and two small per-point products that
 * the linear maps on v_e = [v_j - v_i, v_i] collapse to:
 *   zz [P,3,6]    = [Zp | Zq],  Zp = v . (scale_z*sign(Wz[:, :Cv]))^T,  Zq = v . (scale_z*sign(Wz[:, Cv:]))^T   (v2s frame)
 *   ut [P,3,2Ov]  = [U  | T ],  U  = v . (scale2*sign(W2[:, :Cv]))^T,   T  = v . (scale2*sign(W2[:, Cv:]))^T    (linear2)
 * linear1's sign planes / beta are permuted once into the kernel's bit order (5 words: s_j-s_i | s_i | s_v[:,0] |
 * s_v[:,1] | s_v[:,2]) by svnet_edgeblock_prepare_f32.  Limits: Cs <= 64, 2*Cv <= 64, Os <= 128, Ov <= 64, k <= 64 (backward: 2 <= k).
 * Per-point outputs: n_max/n_min [P,Os] (extreme integer popcount sums over the k neighbours) with their slots,
 * mv/mvn [P,3,Ov] (mean_k v', mean_k v'/|v'|); batch statistics as exact integer sums stat_n [SVNET_RED_SLICES][2*Os] (sum n,
 * sum n^2; in slices that svnet_edgeblock_coeffs_f32 adds up) and fp64 sums stat_v [SVNET_RED_SLICES][2*Ov]; gate_sum [B,2Cs] = sum over the cloud's edges of [s_j-s_i, s_i] (caller zero-fills
 * stat_*, gate_sum; stat_* may both be NULL in eval mode).                                                      */
typedef struct svnet_edgeblock_desc {
    int64_t B, N, k;
    int Cs, Cv, Os, Ov;
    const float* s; const float* v; const int64_t* idx;
    const float* zz; const float* ut;
    const uint64_t* w_sign; const uint64_t* w_nz; const float* beta_perm;
    int32_t* n_max; int32_t* n_min; uint8_t* slot_max; uint8_t* slot_min;
    float* mv; float* mvn;
    int64_t* stat_n; double* stat_v; double* gate_sum;
    /* kept for the backward (both or none): n16 [E,Os] = the integer popcount sum of every edge row, planes [E,3,5] = the
     * sign | non-zero | STE (|x+beta| <= 1.2) bit planes of the binarized edge feature in the fused bit order            */
    int16_t* n16; uint64_t* planes;
    /* (may be NULL) the flag svnet_edgeblock_wbt_bf16 leaves: 1 = no weight of the layer is exactly 0, i.e. sign(W1) is +-1 everywhere and the
     * forward kernels may skip the weights' non-zero plane (same integer counts, 40 % fewer popcount instructions)                     */
    const uint32_t* w_dense;
} svnet_edgeblock_desc;
int svnet_edgeblock_prepare_f32(const float* W, const float* beta, int64_t Os, int64_t Cs, int64_t Cv, uint64_t* w_sign,
                                uint64_t* w_nz, float* beta_perm /*[5*64]*/, void* stream);
/* The binarized weights of the two per-point products in one table: wv [2Ov+6, Cv] = [sign(W2[:, :Cv]) ; sign(W2[:, Cv:]) ;
 * sign(Wz[:, :Cv]) ; sign(Wz[:, Cv:])], scv [2Ov+6] = [scale2, scale2, scalez, scalez]  (ut = v.wv[:2Ov]^T*scv, zz = v.wv[2Ov:]^T*scv). */
int svnet_edgeblock_prepare_vec_f32(const float* W2, const float* scale2, const float* Wz, const float* scalez, int64_t Ov,
                                    int64_t Cv, float* wv, float* scv, void* stream);
int svnet_edgeblock_fwd_f32(const svnet_edgeblock_desc* desc, void* stream);
/* Which kernel instantiation svnet_edgeblock_fwd_f32 launches for these sizes (pure host function; the launch switches on it):
 * SVNET_EDGE_FWD_TWO = the two-edges-per-iteration kernel (Cs <= 32, 2 Cv <= 32, Os <= 32, Ov <= 32 and 32-bit offsets into ut);
 * else 100 + 10 * OP + NARROW = edgeblock_fwd_kernel<OP, NARROW> (OP = output channels per lane: 1 for Os <= 64, else 2; NARROW = Cs <= 32
 * and 2 Cv <= 32).  -1 = outside the limits above (Cs <= 64, 2 Cv <= 64, Os <= 128, Ov <= 64).                                    */
#define SVNET_EDGE_FWD_TWO 1
int svnet_edgeblock_fwd_tier(int64_t Cs, int64_t Cv, int64_t Os, int64_t Ov, int64_t B, int64_t N);
/* coef [4*Os + 4*Ov] = [A1 | B1 | mean_y | invstd_y | Av | Bv | mean_n' | invstd_n']: BatchNorm folded into
 * y = A1*n + B1 and q = Av + Bv/n'; training != 0 uses the batch sums (E = B*N*k edges) and updates running_*.   */
int svnet_edgeblock_coeffs_f32(const int64_t* stat_n, const double* stat_v, int64_t E, int64_t Os, int64_t Ov,
                               const float* scale1, const float* gamma1, const float* beta1, float* running_mean1,
                               float* running_var1, const float* gamma2, const float* beta2, float* running_mean2,
                               float* running_var2, int training, float eps, float momentum, float* coef,
                               int64_t* num_batches_tracked1, int64_t* num_batches_tracked2 /* += 1 when training; may be NULL */,
                               const svnet_gate_fwd_job* gate_job /* may be NULL */, void* stream);
/* s_out[P,Os] = leaky_relu(A1*(A1>=0 ? n_max : n_min) + B1);  v_out[P,3,Ov] = gate[b]*(Av*mv + Bv*mvn).
 * s_cat / v_cat (each may be NULL): the same values written a second time as a column slice of wider rows - s_cat[p*s_ld + o],
 * v_cat[(p*3 + d)*v_ld + c] - i.e. straight into svcat([x1, x2, x3, x4]) of sv_dgcnn_cls.py:68 (no concatenation pass).        */
int svnet_edgeblock_apply_f32(const int32_t* n_max, const int32_t* n_min, const float* mv, const float* mvn,
                              const float* coef, const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov,
                              float slope, float* s_out, float* v_out, float* s_cat, int64_t s_ld, float* v_cat, int64_t v_ld,
                              void* stream);

/* Everything between a fused level's edge pass and the next level's k-NN in ONE launch: the coefficients (svnet_*_coeffs_f32, gate MLP
 * included), the apply pass (svnet_*_apply_f32) and, with knn_workspace, the next k-NN's table (svnet_*_apply_knn_f32).  Three dependent
 * launches of latency-bound work per level sat on the forward's critical path; here every workgroup (32 points of one cloud) derives
 * the ~2 (Os + Ov) coefficients from the statistic slices and its cloud's gate itself - the same expressions as the separate kernels,
 * bit-identical outputs - and workgroup 0 alone writes coef, the running statistics and the counters.  Needs N % 32 == 0, Os <= 256,
 * Ov <= 256 and a dynamic LDS of at most 64 KiB - the coefficients, plus 32 staged rows of Os + 3 Ov floats only with a table
 * (svnet_block_tail_supported); stat1 = the scalar path's sums: int64 slices of (sum n, sum n^2) for the edge block
 * (scale1 required), fp64 slices of (sum y, sum y^2) for the first level (scale1 NULL); hi / lo = n_max / n_min (int32) or y_max / y_min. */
typedef struct svnet_block_tail_desc {
    const void* stat1; const double* stat_v; int64_t E, Os, Ov;
    const float* scale1;
    const float* gamma1; const float* beta1; float* running_mean1; float* running_var1;
    const float* gamma2; const float* beta2; float* running_mean2; float* running_var2;
    int training; float eps, momentum;
    float* coef; int64_t* num_batches_tracked1; int64_t* num_batches_tracked2;
    svnet_gate_fwd_job gate;
    const void* hi; const void* lo; const float* mv; const float* mvn;
    int64_t P, N; float slope;
    float* s_out; float* v_out; float* s_cat; int64_t s_ld; float* v_cat; int64_t v_ld;
    void* knn_workspace; size_t knn_workspace_bytes;          /* NULL / 0: no table */
} svnet_block_tail_desc;
int svnet_block_tail_supported(int64_t P, int64_t N, int64_t Os, int64_t Ov, int with_knn_table);
int svnet_edgeblock_tail_f32(const svnet_block_tail_desc* desc, void* stream);
int svnet_xyzblock_tail_f32(const svnet_block_tail_desc* desc, void* stream);

/* Backward of the fused edge block: a point-level prelude reduces the batch-statistic terms of both BatchNorms,
 * then the edge pass produces all gradients from the point tables and the n16 / planes the forward kept
 * (csrc/edgeblock_bwd.hip).  Outputs of svnet_edgeblock_bwd_f32 (caller zero-fills every *_acc, dzc, dbeta_perm):
 *   dn_out [E,Os]            dL/d(scale*n) per edge          -> GX = dn_out^T . x_b via svnet_gemm_f32 (ternary A)
 *   x_sign32/x_nz32          row-sliced planes of x_b in fused column order, [ceil(E/64), 320] uint64 viewed as uint32
 *   msg [E,R]                per-edge contributions to the NEIGHBOUR j of each edge (summed by svnet_edgeblock_bwd_gather_f32)
 *   ub_tab, ge_tab [P,3,Ov]  per-point operands from which that kernel recomputes the neighbour's share of dL/dv'
 *   ds_acc [P,Cs], dv_acc [P,3,Cv]   centre parts of the gradients of the point tables
 *   dvc [P,3,Ov], dzc [P,3,3]  centre sums of dL/dv' and dL/dz   (dU = sum_j - dvc, dT = dvc; dZp = sum_j - dzc, dZq = dzc)
 *   dbeta_perm [SVNET_DBETA_SLICES][320]   dL/dbeta in fused column order, spread over slices that
 *                            svnet_edgeblock_bwd_gather_f32 sums (one set of 320 addresses was an atomic hot spot)        */
#define SVNET_DBETA_SLICES 64
typedef struct svnet_edgeblock_bwd_desc {
    int64_t B, N, k;
    int Cs, Cv, Os, Ov;
    const float* v; const int64_t* idx; const float* zz; const float* ut;
    const int16_t* n16; const uint64_t* planes;   /* kept by svnet_edgeblock_fwd_f32 */
    const uint16_t* w1bt;        /* svnet_edgeblock_wbt_bf16: sign(W1) as bf16 MFMA fragments, 320 * 16*ceil(Os/16) + 512 values */
    const float* scale1;
    const uint8_t* slot_max; const uint8_t* slot_min;
    const float* coef;           /* from svnet_edgeblock_coeffs_f32 */
    const float* gate;           /* [B,Ov] */
    const float* gy;             /* [P,Os] from the prelude */
    const float* bcoef;          /* [8*Os + 2*Ov + 4] from svnet_edgeblock_bwd_coeffs_f32 (with scale1) */
    const float* gv;             /* upstream gradient of v_out [P,3,Ov] */
    const float* gconst;         /* [B,2Cs]: dL/d(gate input) / (N*k) */
    float* dn_out; uint32_t* x_sign32; uint32_t* x_nz32;
    float* msg;                  /* [E, svnet_edgeblock_msg_stride]: per-edge neighbour contributions (written, not accumulated) */
    float* ub_tab; float* ge_tab; /* [P,3,Ov] each: T_i - U_i and gv_i*gate/k, written by the vector path for the gather kernel */
    float* ds_acc; float* dv_acc; float* dvc; float* dzc; float* dbeta_perm;   /* centre sums (atomics) / dvc written */
    int64_t* debug;              /* optional [4]: {count, first bad edge, its idx value, N}; edges with idx outside [0,N) are skipped */
    int parts;                   /* 0 or 3: both kernels; 1: vector path only (dvc, ub_tab, ge_tab); 2: scalar/tile path only.  The two
                                    are independent, so a caller may issue them on two streams                                   */
} svnet_edgeblock_bwd_desc;
/* wbt: 320 * 16*ceil(Os/16) + 512 bf16 values, [column tile (10)][k-step][lane (64)][8] (the tile kernel's B-fragment order), then ONE
 * all-zero fragment [lane (64)][8]: what a wave without a column tile, and the second k-step of Os = 8 / 16, read                          */
/* w_dense (may be NULL; then Cs / Cv are unused): one uint32, set to 1 when the planes show no zero weight among the columns in use
 * (Cs bits of words 0 - 1, 2 Cv bits of words 2 - 4), else 0 - see svnet_edgeblock_desc                                                   */
int svnet_edgeblock_wbt_bf16(const uint64_t* w_sign, const uint64_t* w_nz, int64_t Os, int64_t Cs, int64_t Cv, uint16_t* wbt,
                             uint32_t* w_dense, void* stream);
/* gy = Gs*lrelu'(y) at the pooled edge; red [SVNET_RED_SLICES][2*Os], redv [SVNET_RED_SLICES][2*Ov], dgate [B,Ov] accumulate (caller
 * zero-fills).  The batch sums are spread over slices (workgroup w adds to slice w % SVNET_RED_SLICES) that
 * svnet_edgeblock_bwd_coeffs_f32 adds up: 512 workgroups adding to ONE set of 2*Os + 2*Ov addresses spent more time in the memory
 * side's atomic queue (11 - 24 us of the kernel's 23 - 35, measured) than reading their rows.                                  */
int svnet_edgeblock_bwd_prelude_f32(const float* gs, const float* gv, const int32_t* n_max, const int32_t* n_min,
                                    const float* mv, const float* mvn, const float* coef, const float* scale1,
                                    const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope,
                                    float* gy, float* red, float* redv, float* dgate,
                                    /* optional SECOND gradient source, added to the first: gs2[p*gs2_ld + o], gv2[(p*3+d)*gv2_ld + c] - column
                                       slices of the gradient of svcat([x1, .., xn]) read where they lie (gs / gv may then be NULL: the
                                       concatenation is the only consumer); with gv2 the summed vector gradient is written to gv_sum [P,3,Ov] */
                                    const float* gs2, int64_t gs2_ld, const float* gv2, int64_t gv2_ld, float* gv_sum, void* stream);
/* bcoef = [m1 | m2 | cs (Os each) | c0 | c1 (Ov each)], and when scale1 != NULL (binarized layer), from the next multiple of
 * 4 floats on, the tile kernel's per-channel table [cs | alpha | beta | scale | pooled-is-max] (5*Os): allocate
 * 8*Os + 2*Ov + 4 floats.  BatchNorm parameter gradients are written to dgamma*, dbeta*.                              */
/* red / redv: the SVNET_RED_SLICES slices a prelude kernel filled (svnet_edgeblock_bwd_prelude_f32, svnet_xyzblock_bwd_prelude_f32). */
int svnet_edgeblock_bwd_coeffs_f32(const float* red, const float* redv, const float* coef, const float* gamma1,
                                   const float* gamma2, int64_t E, int64_t Os, int64_t Ov, int training, const float* scale1,
                                   float* bcoef, float* dgamma1, float* dbeta1, float* dgamma2, float* dbeta2,
                                   const svnet_gate_bwd_job* gate_job /* may be NULL */, void* stream);
int svnet_edgeblock_bwd_f32(const svnet_edgeblock_bwd_desc* desc, void* stream);
/* Which instantiation of the 32-edge tile kernel svnet_edgeblock_bwd_f32 launches (pure host function; the launch switches on it):
 * 100 * NKS + NC2 = edgeblock_bwd_kernel<0, NKS, NC2>.  NKS = 2 / 4 / 8 for Os <= 32 / 64 / 128 (16-row k-steps of phase B); NC2 = 20 / 24 /
 * 44 / 48 = the eight-edges-per-wave form of phase C for Cv <= 10 / 12 / 21 / 24, taken when 3 <= Cv <= 24 and 3 Cv <= 2 Cs, else 0 = the
 * one-edge form.  -1 = outside the backward's limits: Cs <= 64, 2 Cv <= 64, Os a power of two in 8 .. 128.                         */
int svnet_edgeblock_bwd_tier(int64_t Cs, int64_t Cv, int64_t Os);
/* Reverse neighbour lists of a kNN graph (idx [B*N,k], cloud-local ids): the edges e = i*k + t that point at j are
 * rev_edge[rev_range[2j] .. rev_range[2j+1]), their source points i (global ids) rev_src[..].  rev_range [2*B*N], rev_edge and
 * rev_src [B*N*k]; N <= 8192; ids outside [0,N) are skipped.  Optional (all three or none): lists longer than `chunk` entries
 * are cut up for svnet_edgeblock_bwd_gather_f32 - every chunk after the first becomes an item (point, chunk number) of ovf_items
 * [2 * (2*B*N*k/chunk + 1)] int32, their number is ADDED to ovf_count[0] (caller zero-fills).                                   */
int svnet_knn_reverse_i32(const int64_t* idx, int64_t B, int64_t N, int64_t k, int32_t* rev_range, int32_t* rev_edge,
                          int32_t* rev_src, int64_t chunk, int32_t* ovf_items, int32_t* ovf_count, void* stream);
/* Row stride (floats) of the per-edge message rows msg[e] = [dL/ds_j (Cs) | dL/dv_j (3*Cv) | dL/dz (9) | pad]
 * that svnet_edgeblock_bwd_f32 writes instead of scattering with float atomics.                                       */
int64_t svnet_edgeblock_msg_stride(int64_t Cs, int64_t Cv, int64_t Ov);
/* Sums the message rows over the reverse lists (one wave per destination point, no atomics), recomputes the neighbour's share
 * of dL/dv' of every incoming edge from ut (U_j), ub_tab / ge_tab (source point) and the coefficients, and finishes the
 * point-level gradients: acat [3P, acat_ld] = [dU | dT | dZp | dZq | pad] (dU = sum - dvc, dT = dvc, ...), ds_acc [P,Cs] +=,
 * dv_acc [P,3,Cv] +=, dbeta1 [2Cs+6Cv] = the slices of dbeta_perm summed, in the reference's feature order.                                  */
int svnet_edgeblock_bwd_gather_f32(const float* msg, const int32_t* rev_range, const int32_t* rev_edge, const int32_t* rev_src,
                                   const float* ut, const float* ub_tab, const float* ge_tab, const float* coef, const float* bcoef,
                                   int64_t Os, const float* dvc, const float* dzc, int64_t P /* = B*N points */,
                                   int64_t N /* points per cloud (sets the XCD-aware point order) */, int64_t Cs, int64_t Cv,
                                   int64_t Ov, float* acat,
                                   int64_t acat_ld /* row stride of acat, >= 2Ov+6 (a multiple of 4 keeps the GEMM's loads 16-byte) */,
                                   float* ds_acc, float* dv_acc, const float* dbeta_perm, float* dbeta1,
                                   int64_t chunk, const int32_t* ovf_items, const int32_t* ovf_count /* as given to svnet_knn_reverse_i32, or 0 / NULL:
                                   a wave then walks a whole list, however long */, void* stream);
/* STE chain rule (svnet_binweight_grad_f32's formula, ASSIGNED) for linear1 from GXp [Os,320] (fused column order), for
 * linear2 from GXc[0:2Ov] and for the v2s frame from GXc[2Ov:2Ov+6]  (GXc [2Ov+6, Cv]).                              */
int svnet_edgeblock_bwd_params_f32(const float* GXp, const float* GXc, const float* W1, const float* scale1, const float* W2,
                                   const float* scale2, const float* Wz, const float* scalez, int64_t Os, int64_t Ov,
                                   int64_t Cs, int64_t Cv, float* dW1, float* dscale1, float* dW2, float* dscale2, float* dWz,
                                   float* dscalez, void* stream);

/* ------------------------------------------------------------------ fused FIRST edge layer (full precision)
 * get_graph_feature (sv_util.py:28-62) -> Vector2Scalar(2,3) (init_scalar, sv_layers.py:111-129)
 * -> SVBlock((6,2),(Os,Ov)) fp (sv_layers.py:172-196) -> svpool (sv_util.py:118-132) in one pass over the edges
 * (csrc/xyzblock.hip).  x: contiguous [B,3,N]; idx [B*N,k] cloud-local; w0/wz: [3,2] (init_scalar / block v2s),
 * w1: [Os,12], w2: [Ov,2].  Per-point outputs as for the binarized block, with fp32 y_max / y_min instead of
 * integer sums; stat_y [SVNET_RED_SLICES][2*Os], stat_v [SVNET_RED_SLICES][2*Ov] fp64 sums (slices, added up by
 * svnet_xyzblock_coeffs_f32) and gate_sum [B,6] accumulate (caller zero-fills).                                   */
typedef struct svnet_xyzblock_desc {
    int64_t B, N, k;
    int Os, Ov;
    const float* x; const int64_t* idx;
    const float* w0; const float* wz; const float* w1; const float* w2;
    float* y_max; float* y_min; uint8_t* slot_max; uint8_t* slot_min;
    float* mv; float* mvn;
    double* stat_y; double* stat_v; double* gate_sum;
    int64_t nc;        /* vector channels of the edge feature: 0 / 2 = [x_j - x_i | x_i] (get_graph_feature), 3 = + x_j x x_i          */
                       /* (get_graph_feature_cross); w0 / wz [3,nc], w1 [Os,6nc], w2 [Ov,nc], gate_sum [B,3nc]                    */
} svnet_xyzblock_desc;
int svnet_xyzblock_fwd_f32(const svnet_xyzblock_desc* desc, void* stream);
/* coef: same layout as svnet_edgeblock_coeffs_f32 (A1 = gamma*invstd, B1 = beta - gamma*mean*invstd, ...).        */
int svnet_xyzblock_coeffs_f32(const double* stat_y, const double* stat_v, int64_t E, int64_t Os, int64_t Ov,
                              const float* gamma1, const float* beta1, float* running_mean1, float* running_var1,
                              const float* gamma2, const float* beta2, float* running_mean2, float* running_var2,
                              int training, float eps, float momentum, float* coef, int64_t* num_batches_tracked1,
                              int64_t* num_batches_tracked2, const svnet_gate_fwd_job* gate_job /* may be NULL */, void* stream);
int svnet_xyzblock_apply_f32(const float* y_max, const float* y_min, const float* mv, const float* mvn, const float* coef,
                             const float* gate, int64_t P, int64_t N, int64_t Os, int64_t Ov, float slope, float* s_out,
                             float* v_out, float* s_cat, int64_t s_ld, float* v_cat, int64_t v_ld /* as svnet_edgeblock_apply_f32 */,
                             void* stream);
/* Backward: the coordinates need no gradient, so the edge pass only accumulates parameter gradients
 * gw = [dW1 (Os*12) | dW2 (Ov*2) | dW0 (6) | dWz (6)]: a SLICED accumulator of GW = Os*6nc + Ov*nc + 6nc floats (SVNET_SLICED_LEN(GW),
 * caller zero-fills, totals by svnet_slices_sum_f32).  bcoef comes from
 * svnet_edgeblock_bwd_coeffs_f32 (same coefficient layout); gconst [B,6] = dL/d(gate input) / (N*k).             */
int svnet_xyzblock_bwd_prelude_f32(const float* gs, const float* gv, const float* y_max, const float* y_min, const float* mv,
                                   const float* mvn, const float* coef, const float* gate, int64_t P, int64_t N, int64_t Os,
                                   int64_t Ov, float slope, float* gy, float* red, float* redv, float* dgate, const float* gs2,
                                   int64_t gs2_ld, const float* gv2, int64_t gv2_ld, float* gv_sum /* as svnet_edgeblock_bwd_prelude_f32 */,
                                   void* stream);
typedef struct svnet_xyzblock_bwd_desc {
    int64_t B, N, k;
    int Os, Ov;
    const float* x; const int64_t* idx;
    const float* w0; const float* wz; const float* w1; const float* w2;
    const uint8_t* slot_max; const uint8_t* slot_min;
    const float* coef; const float* bcoef; const float* gate; const float* gy; const float* gv; const float* gconst;
    float* gw;
    int64_t nc;        /* as in svnet_xyzblock_desc; gw = [dW1 (Os*6nc) | dW2 (Ov*nc) | dW0 (3nc) | dWz (3nc)], gconst [B,3nc]   */
} svnet_xyzblock_bwd_desc;
int svnet_xyzblock_bwd_f32(const svnet_xyzblock_bwd_desc* desc, void* stream);
/* Which instantiation svnet_xyzblock_fwd_f32 and svnet_xyzblock_bwd_f32 launch (pure host function; both launches switch on it):
 * 10 * NC + EPI = xyzblock_fwd_kernel<NC, EPI> / xyzblock_bwd_kernel<NC, EPI>; NC = 2 (nc 0 or 2) or 3; EPI = edges per wave iteration: 2 for
 * Os <= 32 and Ov <= 32, else 1.  -1 = outside Os <= 64, Ov <= 64, nc in {0, 2, 3}.                                                 */
int svnet_xyzblock_tier(int64_t Os, int64_t Ov, int64_t nc);

/* Weight-gradient product of a fused edge layer: GX[o*320 + c] += sum_e dy[e,o] * x_b[e,c] over the E = B*N*k edge rows, with
 * dy[e,o] = dL/dy_pre RECOMPUTED from the forward's int16 sums: chc[o]*g - (chc[Os+o] + chc[2Os+o]*n16[e,o]), g = gy[p,o] when the
 * pooled slot of (p,o) (slot_max or slot_min by chc[4Os+o]) is e - p*k, else 0; chc = the per-channel table svnet_edgeblock_bwd_coeffs_f32
 * leaves at bcoef + ((3*Os + 2*Ov + 3) & ~3).  x_sign / x_nz: the row-sliced planes the tile kernel writes.  8 <= k <= 64.
 * GX accumulates (caller zero-fills); q_tile_mask as tern_tile_mask of svnet_gemm_desc.                                          */
int svnet_edgeblock_wgrad_f32(const int16_t* n16, const uint8_t* slot_max, const uint8_t* slot_min, const float* gy,
                              const float* chc, const uint64_t* x_sign, const uint64_t* x_nz, int64_t E, int64_t k, int64_t Os,
                              float* GX, uint32_t q_tile_mask, void* stream);
/* Which kernel svnet_edgeblock_wgrad_f32 launches (pure host function; the launch and the caller's choice of path switch on it):
 * SVNET_WGRAD_AFF2 = one 128 x 320 output tile per workgroup (Os = 128, all ten 32-column tiles of q_tile_mask in use, E % 32 == 0);
 * SVNET_WGRAD_TERN5 = the ternary TN kernel with five column tiles per wave, affine A operand.  -1 = not served (k < 8: a 16-row k-step
 * would span more than two points; k > 64; E % k != 0; Os > 128; (E / k) * Os >= 2^29): the caller has the tile kernel write dn_out and
 * runs svnet_gemm_f32 on the planes instead.                                                                                      */
#define SVNET_WGRAD_TERN5 1
#define SVNET_WGRAD_AFF2 2
int svnet_edgeblock_wgrad_tier(int64_t E, int64_t k, int64_t Os, uint32_t q_tile_mask);

/* ------------------------------------------------------------------ Vector2Scalar (sv_layers.py:104-129)
 * v: [M,3,C]; w_eff: [J,C] effective weights (scale*sign(W) or W); z[m,i,j] = sum_c v[m,i,c] w_eff[j,c];
 * s[m, d*J+j] = sum_i v[m,i,d] z[m,i,j].  z_out optional ([M,3,J]).  J == 3, C <= 768.              */
int svnet_v2s_fwd_f32(const float* v, const float* w_eff, int64_t M, int64_t C, int64_t J, float* s, float* z_out,
                      void* stream);
/* ds: [M,C*J]; dz_in: optional gradient arriving at z ([M,3,J]); dv: [M,3,C] (written);
 * GX: a SLICED accumulator of J*C floats (SVNET_SLICED_LEN(J*C), caller zero-fills; totals by svnet_slices_sum_f32):
 * GX[j,c] = sum_m sum_i dz[m,i,j] v[m,i,c].  */
int svnet_v2s_bwd_f32(const float* v, const float* w_eff, const float* ds, const float* dz_in, int64_t M, int64_t C,
                      int64_t J, float* dv, float* GX, void* stream);
/* cat[pre, Vector2Scalar(v)] written in place (sv_layers.py:187-188: the input of an SVBlock's linear1): out [M, out_ld] rows =
 * [pre (pre_cols floats) | s (C*J floats)], out_ld >= pre_cols + C*J; and the backward with the gradient of s given as a column slice
 * of a wider gradient (rows of stride ds_ld).                                                                                       */
int svnet_v2s_cat_fwd_f32(const float* v, const float* w_eff, const float* pre, int64_t pre_cols, int64_t M, int64_t C, int64_t J,
                          float* out, int64_t out_ld, void* stream);
/* ... and, from the copy of `pre` it makes anyway, the per-cloud column sums of pre: pre_sum [M / rows_per_cloud, pre_cols] fp64 (caller
 * zero-fills) - the input of the SVBlock's gate MLP (sv_layers.py:179: s.mean over the points; svnet_gate_mlp_fwd_f32 with gin_f64 =
 * pre_sum, in_scale = 1 / rows_per_cloud), so that no pooling pass reads s a second time.  svnet_v2s_cat_sum_supported: 24 < C <= 192,
 * pre_cols <= 256 (C <= 96) / 512, whole clouds, rows_per_cloud a multiple of 32 (C <= 96) / 16.                                      */
int svnet_v2s_cat_sum_supported(int64_t M, int64_t C, int64_t pre_cols, int64_t rows_per_cloud);
int svnet_v2s_cat_sum_fwd_f32(const float* v, const float* w_eff, const float* pre, int64_t pre_cols, int64_t M, int64_t C, int64_t multi,
                              float* out, int64_t out_ld, double* pre_sum, int64_t rows_per_cloud, void* stream);
int svnet_v2s_bwd_ld_f32(const float* v, const float* w_eff, const float* ds, int64_t ds_ld, const float* dz_in, int64_t M, int64_t C,
                         int64_t J, float* dv, float* GX, void* stream);
/* Frame projection with a GIVEN per-row frame z [M,3,J] (the back-projection einsum 'bimj,bijk->bimk' of
 * sv_pointnet_partseg.py:89): s[m, c*J+j] = sum_i v[m,i,c] z[m,i,j].  Backward: dv [M,3,C] and dz [M,3,J], both written.  */
int svnet_vproject_fwd_f32(const float* v, const float* z, int64_t M, int64_t C, int64_t J, float* s, void* stream);
int svnet_vproject_bwd_f32(const float* v, const float* z, const float* ds, int64_t M, int64_t C, int64_t J, float* dv,
                           float* dz, void* stream);

/* ------------------------------------------------------------------ BatchNorm1d over rows (+ activation)
 * (sv_layers.py:166-167,189-190; nn.BatchNorm1d defaults eps=1e-5, momentum=0.1)
 * stats: sums[0:C] = sum_m x, sums[C:2C] = sum_m x^2 in fp64; `sums` is a sliced accumulator of 2*C doubles (SVNET_SLICED_LEN(2*C),
 * zero-filled by the caller).
 * kind 0: x is [M,C];  kind 1: x is [M,3,C] and the statistic is n = ||x[m,:,c]||_2 + 1e-6 (VectorBN, :94). */
int svnet_colstats_f64(const float* x, int64_t M, int64_t C, int kind, double* sums, void* stream);
/* mean/invstd from the sums (training: `sums` = the sliced accumulator svnet_colstats_f64 / svnet_binlinear_i8_fwd_f32 filled; its totals
 * are left in sums[0:2C]), running-stat update and num_batches_tracked += 1 (each may be NULL). */
int svnet_bn_finalize_f32(double* sums, int64_t M, int64_t C, float eps, float momentum, float* mean,
                          float* invstd, float* running_mean, float* running_var, int64_t* num_batches_tracked,
                          void* stream);
/* eval mode: mean = running_mean, invstd = 1/sqrt(running_var+eps).                                 */
int svnet_bn_eval_stats_f32(const float* running_mean, const float* running_var, int64_t C, float eps, float* mean,
                            float* invstd, void* stream);
/* y = act((x-mean)*invstd*gamma+beta); act: 0 none, 1 leaky-relu(slope), 2 relu.                    */
int svnet_bn_act_fwd_f32(const float* x, const float* mean, const float* invstd, const float* gamma,
                         const float* beta, int64_t M, int64_t C, int act, float slope, float* y, void* stream);
/* backward, pass 1: red[0:C] = sum g', red[C:2C] = sum g'*xhat (`red`: a sliced accumulator of 2*C floats, SVNET_SLICED_LEN(2*C), zero-filled),
 * g' = g * act'(bn(x)).  pass 2: dx; train_stats=1 subtracts the batch-statistic terms; it adds the slices of `red` up and leaves
 * dgamma = red[C:2C], dbeta = red[0:C] (without pass 2: svnet_slices_sum_f32(red, 2C)).           */
int svnet_bn_act_bwd_reduce_f32(const float* g, const float* x, const float* mean, const float* invstd,
                                const float* gamma, const float* beta, int64_t M, int64_t C, int act, float slope,
                                float* red, void* stream);
int svnet_bn_act_bwd_apply_f32(const float* g, const float* x, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, float* red, int64_t M, int64_t C, int act,
                               float slope, int train_stats, float* dx, void* stream);

/* ------------------------------------------------------------------ VectorBN (+ gate)  (sv_layers.py:81-102, :194)
 * v: [M,3,C]; n = ||v||+1e-6; out = v * (bn(n)/n) * gate[b,c]  (gate NULL = 1; b = m / rows_per_batch). */
int svnet_vbn_fwd_f32(const float* v, const float* mean, const float* invstd, const float* gamma, const float* beta,
                      const float* gate, int64_t rows_per_batch, int64_t M, int64_t C, float* out, void* stream);
/* The same forward with the statistics finalised inside (training): sums = svnet_colstats_f64(v, kind 1); every thread derives its
 * channel's mean / invstd (svnet_bn_finalize_f32's arithmetic), workgroup 0 writes them to mean / invstd [C] (the backward needs them)
 * and updates running_mean / running_var / num_batches_tracked (each may be NULL) - no one-workgroup launch between the two passes. */
int svnet_vbn_fwd_stats_f32(const float* v, const double* sums, float eps, float momentum, float* mean, float* invstd,
                            float* running_mean, float* running_var, int64_t* num_batches_tracked, const float* gamma,
                            const float* beta, const float* gate, int64_t rows_per_batch, int64_t M, int64_t C, float* out,
                            void* stream);
/* pass 1: red[0:C] = sum dr, red[C:2C] = sum dr*nhat (`red`: a sliced accumulator of 2*C floats, SVNET_SLICED_LEN(2*C)),
 * dgate[b,c] += sum g*v*q  (caller zero-fills red, dgate) */
int svnet_vbn_bwd_reduce_f32(const float* g, const float* v, const float* mean, const float* invstd,
                             const float* gamma, const float* beta, const float* gate, int64_t rows_per_batch,
                             int64_t M, int64_t C, float* red, float* dgate, void* stream);
int svnet_vbn_bwd_apply_f32(const float* g, const float* v, const float* mean, const float* invstd,
                            const float* gamma, const float* beta, const float* gate, float* red,
                            int64_t rows_per_batch, int64_t M, int64_t C, int train_stats, float* dv, void* stream);

/* ------------------------------------------------------------------ pooling (sv_util.py:118-132 svpool; adaptive pools of sv_dgcnn_cls.py:72-73)
 * x: [outer, R, inner] -> out [outer, inner].  mode 0 = max (argmax int32 saved, first index on ties),
 * mode 1 = mean.  workspace (optional, svnet_pool_workspace_bytes): lets a long reduction with few outputs (pooling over
 * the N points) be split over workgroups; the partial results are combined in a fixed order (bit-reproducible, no float
 * atomics).  NaN inputs are not supported on the split max path.               */
size_t svnet_pool_workspace_bytes(int64_t outer, int64_t R, int64_t inner, int mode);
int svnet_pool_fwd_f32(const float* x, int64_t outer, int64_t R, int64_t inner, int mode, float* out, int64_t out_ld,
                       int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream);
/* [max | mean] over the reduced axis in ONE pass over x (sv_dgcnn_cls.py:72-74: adaptive max pool and adaptive avg pool of the same
 * feature): out_max / out_mean [outer, inner] rows of stride out_ld, argmax as svnet_pool_fwd_f32; R >= 256; workspace =
 * svnet_pool_workspace_bytes(outer, R, inner, 0) + svnet_pool_workspace_bytes(outer, R, inner, 1) bytes.  The mean's partial sums
 * are added in a fixed order (bit-reproducible), like mode 1 of svnet_pool_fwd_f32.                                              */
int svnet_pool_maxmean_fwd_f32(const float* x, int64_t outer, int64_t R, int64_t inner, float* out_max, float* out_mean,
                               int64_t out_ld, int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream);
/* conv5 of the classifier (sv_layers.py:189-190 bn1 + LeakyReLU, then sv_dgcnn_cls.py:72-74 max / avg pool over the points): BatchNorm
 * with the given per-channel statistics (+ activation: 0 none, 1 LeakyReLU(slope), 2 ReLU) of y [outer*R, inner], pooled
 * [max | mean] over R in the same pass - the activated tensor is never written.  Outputs / argmax / workspace as
 * svnet_pool_maxmean_fwd_f32 (R >= 256).  The values equal pooling svnet_bn_act_fwd_f32's output bit for bit.                     */
int svnet_bn_pool_fwd_f32(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta,
                          int64_t outer, int64_t R, int64_t inner, int act, float slope, float* out_max, float* out_mean,
                          int64_t out_ld, int32_t* argmax, void* workspace, size_t workspace_bytes,
                          int workspace_zeroed /* != 0: the first outer*inner*8 bytes of the workspace (the arg-max keys) are zero already */,
                          void* stream);
/* Its backward from the POOLED gradients (gmax, gmean: rows of stride g_ld): the gradient of the activated tensor,
 * (r == argmax ? gmax : 0) + gmean / R, is formed on the fly.  red [2*inner] (caller zero-fills) = [dbeta | dgamma];
 * dy [outer*R, inner] (may be NULL) the gradient of y, with the batch-statistic terms when train_stats.                           */
int svnet_bn_pool_bwd_f32(const float* gmax, const float* gmean, int64_t g_ld, const int32_t* argmax, const float* y,
                          const float* mean, const float* invstd, const float* gamma, const float* beta, int64_t outer, int64_t R,
                          int64_t inner, int act, float slope, int train_stats, float* red, float* dy, void* stream);   /* out[o*out_ld + i]; argmax [outer,inner] */
int svnet_pool_bwd_f32(const float* g, const int32_t* argmax, int64_t outer, int64_t R, int64_t inner, int mode,
                       float* dx, void* stream);
/* The tail of the classifier's vector path as one pass over linear2's product v [B*N, 3, C] (C <= 192): VectorBN + gate
 * (sv_layers.py:86-102,193-194) -> Vector2Scalar of svfuse (sv_layers.py:111-129,206-220; w_eff [3, C] = scale * sign(W)) -> [max | mean]
 * over each cloud's N points (sv_dgcnn_cls.py:70-74) - neither VectorBN's output nor the [B*N, 3C] scalars are written.
 * sums != NULL (training): the sliced fp64 accumulator svnet_colstats_f64(v, B*N, C, kind 1) filled; the batch statistics are
 * finalised inside (mean / invstd [C] written, running statistics and *nbt updated as svnet_vbn_fwd_stats_f32 does).  sums == NULL
 * (eval): mean / invstd are INPUTS (svnet_bn_eval_stats_f32).  gate [B, C] or NULL.  out_max / out_mean [B, 3C] rows of stride out_ld,
 * argmax [B, 3C] int32 (point index in the cloud, first index on ties); workspace = svnet_vtail_workspace_bytes(B, N, C) bytes.
 * The maxima equal pooling the layer-wise chain's output; the means add their partial sums in a fixed order (bit-reproducible).   */
size_t svnet_vtail_workspace_bytes(int64_t B, int64_t N, int64_t C);
int svnet_vtail_fwd_f32(const float* v, const double* sums, float eps, float momentum, float* mean, float* invstd,
                        float* running_mean, float* running_var, long long* nbt, const float* gamma, const float* beta,
                        const float* gate, const float* w_eff, int64_t B, int64_t N, int64_t C, float* out_max, float* out_mean,
                        int64_t out_ld, int32_t* argmax, void* workspace, size_t workspace_bytes,
                        int workspace_zeroed /* != 0: the first B*3C*8 bytes (the arg-max keys) are zero already */, void* stream);
/* Its backward up to VectorBN's batch sums, from the POOLED gradients (gmax / gmean: rows of stride g_ld): the gradient of the scalars,
 * (point == argmax ? gmax : 0) + gmean / N, is formed on the fly, Vector2Scalar's backward runs in registers.  Outputs: g5 [B*N, 3, C] =
 * dL/d(VectorBN's output) (may be NULL: see svnet_vtail_bwd_apply_f32), to be handed to svnet_vbn_bwd_apply_f32 as its `g` together with `red`; red = SLICED accumulator of 2C floats
 * (SVNET_SLICED_LEN(2C), zero-filled; the apply pass adds the slices up and leaves [dbeta | dgamma]); dgate [B, C] (zero-filled, += ; may
 * be NULL when gate is); GX = sliced accumulator of 3C floats: dL/d(w_eff) as [3][C] (svnet_binweight_grad_f32 with gx_sliced).        */
int svnet_vtail_bwd_f32(const float* v, const float* mean, const float* invstd, const float* gamma, const float* beta,
                        const float* gate, const float* w_eff, const float* gmax, const float* gmean, int64_t g_ld,
                        const int32_t* argmax, int64_t B, int64_t N, int64_t C, float* red, float* dgate, float* GX, float* g5,
                        void* stream);
/* The rest of that backward WITHOUT the stored g5 (pass NULL for it above): the same per-point recomputation of dL/d(VectorBN's output), then
 * VectorBN's apply pass on it (svnet_vbn_bwd_apply_f32's formulas) with the totals of `red`'s slices - dv [B*N, 3, C] = dL/dv, and
 * [dbeta | dgamma] left in the first 2C elements of red.  One read of v and one write instead of two reads, a write and a read.          */
int svnet_vtail_bwd_apply_f32(const float* v, const float* mean, const float* invstd, const float* gamma, const float* beta,
                              const float* gate, const float* w_eff, const float* gmax, const float* gmean, int64_t g_ld,
                              const int32_t* argmax, int64_t B, int64_t N, int64_t C, float* red, int train_stats, float* dv, void* stream);
/* dx[o,r,i] = add[(o*R + r)*add_ld + i] + gmean[o,i] / R: the backward of a mean over r (sv_layers.py:179: the gate's pooled input) added to
 * another gradient of the same tensor that arrives as rows of stride add_ld (the s columns of the gradient of cat[s, Vector2Scalar(v)],
 * sv_layers.py:187-188) - one pass instead of a broadcast pass and a strided elementwise add.                                       */
int svnet_pool_mean_bwd_add_f32(const float* gmean, const float* add, int64_t add_ld, int64_t outer, int64_t R, int64_t inner,
                                float* dx, void* stream);
/* Backward of cat(max, mean) over the same axis (the classifier's global pooling, sv_dgcnn_cls.py:72-74) in one pass:
 * gmax / gmean: dL/dmax and dL/dmean as rows of stride g_ld (column slices of the pooled feature's gradient),
 * dx[o,r,i] = (argmax[o,i] == r ? gmax[o,i] : 0) + gmean[o,i] / R.       */
int svnet_pool_maxmean_bwd_f32(const float* gmax, const float* gmean, int64_t g_ld, const int32_t* argmax, int64_t outer, int64_t R,
                               int64_t inner, float* dx, void* stream);

/* ------------------------------------------------------------------ element-wise activations of the gate (sv_layers.py:156-161)
 * kind 1 = relu, 2 = sigmoid, 3 = leaky-relu(0.2).  Backward uses the OUTPUT y.                      */
int svnet_act_fwd_f32(const float* x, int64_t n, int kind, float* y, void* stream);
int svnet_act_bwd_f32(const float* g, const float* y, int64_t n, int kind, float* dx, void* stream);

/* ------------------------------------------------------------------ gate MLP of an SVBlock (sv_layers.py:156-161,179-183)
 * gate[b,:] = sigmoid(W2 . relu(W0 . (in_scale*gin[b,:])));  W0 [H,Cin], W2 [Ov,H], no biases; h [B,H] is saved for the
 * backward.  The input is either gin (fp32) or gin_f64 (the fp64 gate_sum of a fused edge layer), which is rounded to
 * fp32 into gin_out [B,Cin] first (kept by the caller for the backward).
 * Backward: dgin = out_scale * dL/d(in_scale*gin) (may be NULL), dW0 / dW2 ACCUMULATE (float atomics).       */
int svnet_gate_mlp_fwd_f32(const float* gin, const double* gin_f64, float* gin_out, float in_scale, const float* W0,
                           const float* W2, int64_t B, int64_t Cin, int64_t H, int64_t Ov, float* h, float* gate,
                           const float* rows /* may be NULL */, int64_t R /* see svnet_gate_fwd_job */, void* stream);
int svnet_gate_mlp_bwd_f32(const float* dgate, const float* gate, const float* h, const float* gin, float in_scale,
                           const float* W0, const float* W2, int64_t B, int64_t Cin, int64_t H, int64_t Ov, float out_scale,
                           float* dgin, float* dW0, float* dW2, void* stream);

/* ------------------------------------------------------------------ classifier heads: dense layers over M = batch rows (M <= 64)
 * (models/sv_dgcnn_cls.py:76-80, models/sv_pointnet_cls.py:59-61:  act(bn(linear(x)))  with linear = sv_layers.Linear(bw, ba),
 *  sv_layers.py:35-51, bn = nn.BatchNorm1d, act = leaky_relu / relu; then nn.Linear)
 * One packing pass over the layer's input, ONE pass forward (binarized product + batch statistics + BatchNorm + activation) and
 * two passes backward (per output channel: BatchNorm backward, weight / scale gradients; per 64 input columns: dx, dbeta) instead
 * of ~12 launch-bound kernels per layer.  Integer counts, outputs and gradients follow svnet_binlinear_fwd_f32 +
 * svnet_colstats_f64 / svnet_bn_finalize_f32 / svnet_bn_act_* and their backward formulas; nothing is accumulated atomically.
 * pack: x [M,K] + beta [K] -> x_sign / x_nz / x_ste row-major [M][ceil(K/64)] (x_ste may be NULL) and the column words
 *       xc_sign / xc_nz [K] (bit m = row m; both NULL or both given - the backward needs them; xc_ste [K], optional, is the STE
 *       plane in the same form = the row-sliced layout of svnet_binlinear_fwd_f32's saved planes).                               */
typedef struct svnet_binhead_desc {
    int64_t M, K, O;                  /* rows (1..64), input columns, output channels */
    const float* W;                   /* [O,K] fp32 master weights (backward: STE mask |W| <= 1.2 and sign) */
    const uint64_t* w_sign;           /* [O][wld] plane words of sign(W) (svnet_binweight_prepare_f32) */
    const uint64_t* w_nz;
    int64_t wld;                      /* words per weight row (>= ceil(K/64)) */
    const float* w_b;                 /* [O,K] sign(W) as +-1 / 0 (backward) */
    const float* scale;               /* [O] */
    const float* gamma;               /* BatchNorm weight / bias [O] */
    const float* bn_beta;
    float* running_mean;              /* [O] or NULL; updated when training (eval: read) */
    float* running_var;
    long long* nbt;                   /* num_batches_tracked (+= 1 when training) or NULL */
    int training;                     /* 1 = batch statistics + STE backward; 0 = running statistics (forward only) */
    float eps, momentum;
    int act;                          /* 0 none, 1 LeakyReLU(slope), 2 ReLU */
    float slope;
    const uint64_t* x_sign;           /* packed input (svnet_binhead_pack_f32) */
    const uint64_t* x_nz;
    const uint64_t* x_ste;            /* backward */
    const uint64_t* xc_sign;          /* backward */
    const uint64_t* xc_nz;
    float* y;                         /* [M,O] pre-BatchNorm output n * scale (forward: written; backward: read) */
    float* mean;                      /* [O] statistics used (forward: written; backward: read) */
    float* invstd;
    float* out;                       /* [M,O] forward result */
    const float* g;                   /* backward: dL/dout [M,O] */
    float* dnT;                       /* backward scratch [O][64] */
    float* dW;                        /* [O,K] (may be NULL) */
    float* dscale;                    /* [O] */
    float* dgamma;                    /* [O] */
    float* dbn_beta;                  /* [O] */
    float* dx;                        /* [M,K] and dbeta_in [K]: both NULL or both given */
    float* dbeta_in;
} svnet_binhead_desc;
int svnet_binhead_pack_f32(const float* x, const float* beta, int64_t M, int64_t K, uint64_t* x_sign, uint64_t* x_nz,
                           uint64_t* x_ste, uint64_t* xc_sign, uint64_t* xc_nz, uint64_t* xc_ste, void* stream);
int svnet_binhead_fwd_f32(const svnet_binhead_desc* d, void* stream);
int svnet_binhead_bwd_f32(const svnet_binhead_desc* d, void* stream);
/* Backward of y = x W^T + b (nn.Linear, sv_dgcnn_cls.py:80) over M <= 64 rows in one launch: dx [M,K] (may be NULL), dW [O,K],
 * db [O] (may be NULL), all ASSIGNED.                                                                                             */
int svnet_fplinear_small_bwd_f32(const float* g, const float* x, const float* W, int64_t M, int64_t K, int64_t O, float* dx,
                                 float* dW, float* db, void* stream);

/* ------------------------------------------------------------------ label-smoothed cross entropy (utils.py:33-50 cal_loss; csrc/loss.hip)
 * logits [R,C], target [R] int64; loss = mean_r -(soft . log_softmax); dlogits = d loss / d logits.
 * workspace: >= 1024 floats (per-workgroup partial losses, added in a fixed order: bit-reproducible).   */
int svnet_smooth_ce_f32(const float* logits, const int64_t* target, int64_t R, int64_t C, float eps, float* loss,
                        float* dlogits, float* workspace, int64_t workspace_floats, void* stream);

/* ------------------------------------------------------------------ knowledge distillation fused with cal_loss (csrc/loss.hip)
 * The reference publishes distilled binary models (README, scripts.sh: *_binary_kd_*) without the loss's source; this is Hinton et al.'s:
 *     ce_r = -(soft_r . log_softmax(s_r))   (utils.py:33-50, soft = 1 - eps at the target, eps / (C - 1) elsewhere)
 *     kl_r = sum_c p_rc (logp_rc - logq_rc),  logp = log_softmax(t_r / T), logq = log_softmax(s_r / T), p = exp(logp)
 *     L = (1 - alpha) mean_r ce_r + alpha T^2 mean_r kl_r
 *     dlogits = dL/ds = [(1 - alpha)(softmax(s_r) - soft_r) + alpha T (exp(logq_r) - p_r)] / rows     (may be NULL; the teacher gets none)
 * student / teacher / dlogits share ONE layout:
 *     SVNET_KD_ROWS           [R,C] contiguous: pass B = R, N = 1; target [R]
 *     SVNET_KD_CHANNEL_MAJOR  [B,C,N] contiguous (the part-segmentation models' output: rows = points, classes at stride N); target
 *                             [B,N].  Read and written where it lies, consecutive lanes along N: no transposed copy of anything.
 * result: 3 floats {L, CE, KL}, CE and KL the unweighted means.  T > 0 and 0 <= alpha <= 1 (else SVNET_E_ARG).  Targets are compared
 * with the class index, never used as one.  logp / logq are formed as (x - max) / T - log(sum exp): an underflowed p contributes 0.
 * workspace: >= SVNET_KD_WORKSPACE_FLOATS floats (one (ce, kl) pair per workgroup, added in a fixed order by a finishing launch of the
 * same call: no float atomics, results and gradient are bit-reproducible).
 * svnet_kd_supported / svnet_kd_tier are pure host functions over the same (layout, B, C, N): supported = 2 <= C <= 65536, 1 <= rows
 * (R, or B * N) <= 2^31 - 1, N = 1 in the rows layout; anything else makes the call return SVNET_E_UNSUPPORTED.  tier: -1 = unsupported,
 * else bit 0 = the classes do not fit one pass (rows layout: C > 64, a lane walks several classes; channel-major: C > 64, the logits
 * are re-read from memory instead of kept in registers), bit 1 = more rows than one grid (rows layout: > 4096 rows, channel-major:
 * > 262144 points) - the workgroups stride.  At alpha = 0 the rows layout's dlogits are svnet_smooth_ce_f32's, bit for bit.          */
#define SVNET_KD_ROWS 0
#define SVNET_KD_CHANNEL_MAJOR 1
#define SVNET_KD_WORKSPACE_FLOATS 8192
int svnet_kd_supported(int layout, int64_t B, int64_t C, int64_t N);
int svnet_kd_tier(int layout, int64_t B, int64_t C, int64_t N);
int svnet_kd_loss_f32(int layout, const float* student, const float* teacher, const int64_t* target, int64_t B, int64_t C, int64_t N,
                      float eps, float alpha, float T, float* result, float* dlogits, float* workspace, int64_t workspace_floats,
                      void* stream);

/* ------------------------------------------------------------------ optimizer steps on flat buffers (main_cls_dgcnn.py:128-133)
 * p, g, m, v, buf: n floats each (all parameters / gradients of the model, flattened in model.parameters() order).
 * Adam = torch.optim.Adam(lr, betas, eps, weight_decay) at 1-based `step` (bias correction); SGD = torch.optim.SGD(lr,
 * momentum, weight_decay) with buf = g on the first step.                                                   */
int svnet_adam_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, void* stream);
int svnet_sgd_step_f32(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float weight_decay,
                       int first_step, void* stream);
/* The same steps with their step-dependent scalars read from DEVICE memory (a launch that can be part of a captured graph; the host
 * refreshes `hyper` before every replay): adam hyper = [lr, beta1, beta2, eps, weight_decay, 1 - beta1^t, 1 / sqrt(1 - beta2^t)],
 * sgd hyper = [lr, momentum, weight_decay, first_step (0 / 1)].                                                                    */
int svnet_adam_step_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper, void* stream);
int svnet_sgd_step_dev_f32(float* p, const float* g, float* buf, int64_t n, const float* hyper, void* stream);

/* ------------------------------------------------------------------ batch assembly from a device-resident pool
 * What the reference's loaders do per sample on the host (data.py:165-170 translate_pointcloud; :192-198 ModelNet40, :284-294
 * ShapeNetPart, :327-337 ScanObjectNN), the collate, the per-batch rotation (main_cls_dgcnn.py:168-178) and the permute to [B,3,N]
 * (:179) as ONE launch, one workgroup per cloud, into fixed caller-owned buffers.  Everything slot b receives is a pure function of
 * (seed, epoch, g = first + b) - counter-based splitmix64, the derivation is fixed in svnet_amd/data.py's docstring - so batch size,
 * rank count, graph replay and a resume cannot change a sample.  Slots count .. B-1 repeat slot 0 (a short final batch stays finite).
 * The sorted modes put 8 bytes per key into LDS (keys: N for FIRST_SHUFFLED, P for SUBSET; at most 8192 = 64 KiB, no opt-in).
 * Attributes: attr_out[b,:,n] is the attr row of the pool point x[b,:,n] came from (slots past count repeat slot 0, a poisoned order
 * entry gives NaN), filled by the same launch and with no further random numbers.  Scalar channels are the pool's bits.  A direction
 * group (q_0, q_1, q_2) transforms as a normal under x' = R (S x) + shift, i.e. with R S^-1 followed by a renormalisation - the
 * definition, operation by operation, stands in svnet_amd/data.py's docstring ("attributes"): with scale_shift q_c = fl(n_c / scale_c),
 * l = fl(sqrt(fl(fl(fl(q_0 q_0) + fl(q_1 q_1)) + fl(q_2 q_2)))), q_c = fl(q_c / l) if l > 0; with a rotation out = R q in the coordinates' operation order;
 * with neither, the pool's bits.  Non-finite attributes: unspecified values, never an out-of-range access.  Attributes take no LDS:
 * svnet_batch_supported does not ask about them.                                                                                 */
#define SVNET_BATCH_MAX_ATTR 32      /* the most attribute channels per point */
#define SVNET_BATCH_FIRST_SHUFFLED 0 /* the first N points of the cloud, in random order */
#define SVNET_BATCH_SUBSET 1         /* N of all P points, in random order */
#define SVNET_BATCH_FIRST_ORDERED 2  /* the first N points as stored */
#define SVNET_BATCH_ROTATE_NONE 0
#define SVNET_BATCH_ROTATE_Z 1       /* uniform angle about z */
#define SVNET_BATCH_ROTATE_SO3 2     /* uniform rotation */
typedef struct svnet_batch_desc {
    const float* data;    /* [M,P,3] pool, point-major */
    const int64_t* label; /* [M] */
    const int64_t* seg;   /* [M,P] or NULL */
    const int64_t* order; /* [L] pool indices in epoch order; an entry outside 0 .. M-1 poisons its slot (NaN, -1) and reads nothing */
    int64_t M, P, L;
    int64_t B, N;         /* the output buffers' batch size and points per cloud, N <= P */
    int64_t first, count; /* slot b < count holds position first + b of `order`; 1 <= count <= B, first + count <= L */
    int64_t seed, epoch;
    int select_mode;      /* SVNET_BATCH_FIRST_SHUFFLED / _SUBSET / _FIRST_ORDERED */
    int scale_shift;      /* 0 / 1: x * scale + shift per axis, scale ~ U(2/3, 3/2), shift ~ U(-0.2, 0.2) per cloud */
    int rotate;           /* SVNET_BATCH_ROTATE_*: R x, applied after scale and shift */
    int64_t num_cat;      /* columns of onehot */
    float* x;             /* [B,3,N] */
    int64_t* y;           /* [B] */
    int64_t* seg_out;     /* [B,N] in x's point order, or NULL */
    float* onehot;        /* [B,num_cat] one-hot of the label, or NULL */
    float* params;        /* [B,16]: 3 scales, 3 shifts, 9 rotation entries (row-major), 0 */
    /* per-point attributes (normals, colours); all zero = none, which is what a descriptor written before ABI 431 says */
    const float* attr;    /* [M,P,A] pool attributes, point-major, or NULL */
    int64_t A;            /* 1 .. SVNET_BATCH_MAX_ATTR when attr is given */
    int64_t attr_vectors; /* the first attr_vectors groups of three channels are direction vectors; 0 <= 3 attr_vectors <= A */
    float* attr_out;      /* [B,A,N] channel-first in x's point order, or NULL (then attr is not read) */
} svnet_batch_desc;
/* 1 when svnet_batch_assemble_f32 takes the shape, else 0: a pure host function. */
int svnet_batch_supported(int64_t P, int64_t N, int select_mode);
int svnet_batch_assemble_f32(const svnet_batch_desc* d, void* stream);

/* ------------------------------------------------------------------ farthest point sampling and the resampled pool
 * (models/utils/pointnet_util.py:63-84 farthest_point_sample; data.py:203-256 ModelNet40_v2(uniform=True) with data.py:15-20 pc_normalize)
 * svnet_fps_f32: xyz [M,P,3], start [M] (the reference draws it with torch.randint; here it is an input), idx [M,npoint]:
 *     mind[p] = fp32(1e10), f = start[m];  npoint times: idx[i] = f, d_c = fl(x[p,c] - x[f,c]),
 *     dist = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2)), mind[p] = dist < mind[p] ? dist : mind[p], f = the SMALLEST p among the
 *     maxima of mind.  Single-rounded fp32, never an fma: given the start, bit-identical to the reference's CPU result.  Coordinates
 *     must be finite (NaN / Inf: undefined order, never an out-of-range index).  A start outside 0 .. P-1 is clamped into the cloud.
 *     One workgroup per cloud; 1 <= npoint <= P <= 16384 (SVNET_E_UNSUPPORTED past it).  svnet_fps_tier: which kernel form a P takes
 *     (0 .. 4: P <= 64, 1024, 4096, 10240, 16384), -1 = unsupported; svnet_fps_supported: 1 / 0.  Both are pure host functions.
 * svnet_pool_gather_f32: out[m,n,:] = data[m, idx[m,n], :] (data [M,P,3], idx [M,N]) and, when seg_out is given, seg_out[m,n] =
 *     seg[m, idx[m,n]] (seg [M,P]); one launch, one workgroup per cloud.  normalize != 0 applies pc_normalize to every selection:
 *     c = the float64 mean of its N points rounded once to fp32 (summed in a fixed order: bit-reproducible), d = fl(p - c),
 *     m = max_n sqrt(fl(fl(d_0 d_0 + d_1 d_1) + d_2 d_2)), out = fl(d / m).  An index outside 0 .. P-1 reads nothing: NaN row, seg -1. */
int svnet_fps_supported(int64_t P, int64_t npoint);
int svnet_fps_tier(int64_t P);
int svnet_fps_f32(const float* xyz, int64_t M, int64_t P, int64_t npoint, const int64_t* start, int64_t* idx, void* stream);
int svnet_pool_gather_f32(const float* data, const int64_t* seg, const int64_t* idx, int64_t M, int64_t P, int64_t N, int normalize,
                          float* out, int64_t* seg_out, void* stream);
/* out[m,n,:] = attr[m, idx[m,n], :] for rows of A floats (attr [M,P,A], idx [M,N], out [M,N,A]; 1 <= A <= SVNET_BATCH_MAX_ATTR): the
 * attributes of a resampled pool, bit for bit, one launch.  An index outside 0 .. P-1 reads nothing: a NaN row.  N * A <= 2^31 - 1 and
 * M * ceil(N A / 256) <= 2^31 - 1, past that SVNET_E_UNSUPPORTED.                                                                 */
int svnet_pool_gather_attr_f32(const float* attr, const int64_t* idx, int64_t M, int64_t P, int64_t N, int64_t A, float* out,
                               void* stream);

/* ------------------------------------------------------------------ feature propagation: sampled points -> dense cloud
 * (models/utils/pointnet_util.py:281-308 PointNetFeaturePropagation.forward without its MLP: three nearest sampled points,
 * inverse-squared-distance weights, weighted sum).  The gradient with respect to feat: svnet_three_interpolate_bwd_f32 below.  Per cloud, query [P,3], ref [N,3], feat [D,N] (channel-first), fp32,
 * every operation rounded once and never contracted into an fma, both divisions correctly rounded:
 *     d_c = fl(query[p,c] - ref[n,c]),  dist[p,n] = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))    (the difference form of svnet_fps_f32:
 *         never negative, exactly 0 at a coincident point; the reference's expanded form -2 q.r + |q|^2 + |r|^2 is NOT used)
 *     idx[p,0..2], dist3[p,0..2]: the min(3, N) smallest dist[p,:], ascending, the LOWER index first among equals; a slot no candidate
 *         took (slots past N when N < 3; candidates whose distance is NaN or +inf are never taken) holds index 0 and dist3 = +inf
 *     rec_j = fl(1 / fl(dist3_j + fp32(1e-8))),  s = fl(fl(rec_0 + rec_1) + rec_2),  weight[p,j] = fl(rec_j / s)   (an empty slot: 0)
 *     out[d,p] = fl(fl(fl(feat[d,i_0] w_0) + fl(feat[d,i_1] w_1)) + fl(feat[d,i_2] w_2))       (N = 1: w_0 = 1, out = feat[d,0])
 * svnet_three_nn_f32: query [B,P,3], ref [B,N,3] -> idx [B,P,3] int64, dist3 [B,P,3], weight [B,P,3].  Every index written lies in
 *     0 .. N-1 whatever the coordinates hold (NaN / Inf: unspecified neighbours, in range).
 * svnet_three_interpolate_f32: feat [B,D,N], idx, weight [B,P,3] -> out [B,D,P].  An index outside 0 .. N-1 is clamped into it.
 * One thread per query point, one launch each, no workspace.  1 <= N <= 32768 (the k-NN's limit), P >= 1, D >= 1,
 * B * ceil(P / 256) <= 2^31 - 1; past that SVNET_E_UNSUPPORTED.  svnet_propagate_supported (1 / 0, without the B term) and
 * svnet_propagate_tile (the sampled points per LDS tile of svnet_three_nn_f32: the N at which its loop takes a second tile) are pure
 * host functions.                                                                                                                  */
int svnet_propagate_supported(int64_t P, int64_t N, int64_t D);
int svnet_propagate_tile(void);
int svnet_three_nn_f32(const float* query, const float* ref, int64_t B, int64_t P, int64_t N, int64_t* idx, float* dist3, float* weight,
                       void* stream);
int svnet_three_interpolate_f32(const float* feat, const int64_t* idx, const float* weight, int64_t B, int64_t D, int64_t N, int64_t P,
                                float* out, void* stream);

/* ------------------------------------------------------------------ ball query and neighbourhood grouping: centres -> local groups
 * (models/utils/pointnet_util.py:87-107 query_ball_point, 110-143 sample_and_group without its sampling).  The gradient with respect to points: svnet_group_points_bwd_f32 below.  Per cloud,
 * xyz [N,3], new_xyz [S,3], points [N,D] (channel-last, or NULL with D = 0), fp32, every operation rounded once and never contracted:
 *     d_c = fl(new_xyz[s,c] - xyz[n,c]),  dist[s,n] = fl(fl(fl(d_0 d_0) + fl(d_1 d_1)) + fl(d_2 d_2))    (the difference form of svnet_fps_f32;
 *         the reference's expanded form -2 a.b + |a|^2 + |b|^2 is NOT used)
 *     point n is inside group s when dist[s,n] <= r2 (the reference: sqrdists > radius ** 2 is outside); a NaN distance is never inside
 *     idx[s,0..nsample-1]: the first nsample inside points in ASCENDING POINT INDEX; slots past the number found hold the first inside
 *         index; count[s] = min(found, nsample).  An empty group (the reference would write index N and fail): count 0, every slot 0.
 *     out[s,j,c] = fl(xyz[idx[s,j],c] - new_xyz[s,c]) for c = 0..2 (point minus centre),  out[s,j,3+d] = points[idx[s,j],d] bit for bit
 * svnet_ball_query_f32: xyz [B,N,3], new_xyz [B,S,3] -> idx [B,S,nsample] int64, count [B,S] int32.  Every index written lies in
 *     0 .. N-1 whatever the coordinates and r2 hold.  One wave per centre, leaving its candidate loop once the group is full.
 * svnet_group_points_f32: idx [B,S,nsample] -> out [B,S,nsample,3+D].  An index outside 0 .. N-1 is clamped into it, never followed.
 * One launch each, no workspace.  1 <= nsample <= N <= 32768 (the k-NN's limit), S >= 1, D >= 0; B * ceil(S / 32) <= 2^31 - 1 for the
 * query and B * S * nsample <= 2^31 - 1 for the grouping; past that SVNET_E_UNSUPPORTED.  svnet_group_supported (1 / 0, without the
 * B terms) and svnet_ball_query_tile (the points per LDS tile of svnet_ball_query_f32: the N at which its candidate loop takes a
 * second tile) are pure host functions.                                                                                            */
int svnet_group_supported(int64_t N, int64_t S, int64_t nsample, int64_t D);
int svnet_ball_query_tile(void);
int svnet_ball_query_f32(const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, float r2, int64_t nsample, int64_t* idx,
                         int* count, void* stream);
int svnet_group_points_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N, int64_t S,
                           int64_t nsample, int64_t D, float* out, void* stream);

/* ------------------------------------------------------------------ gradients of grouping and interpolation (autograd supplies them in the
 * reference: models/utils/pointnet_util.py:166-207, 270-320).  Both are scatters; here each is a reverse list per destination and a
 * per-destination sum in a fixed order.  No float atomic: two runs give the same bits.  Per cloud:
 * svnet_pointset_reverse_i32: idx [R,K] int64 -> rev_start [N+1], rev_edge [R*K] int32.  Edge e = r K + j points to
 *     n = idx[r,j] clamped into 0 .. N-1 (the clamp svnet_three_interpolate_f32 and svnet_group_points_f32 follow); nothing is skipped.
 *     List n = rev_edge[rev_start[n] .. rev_start[n+1]) holds every edge that points to n exactly once, in ASCENDING e.  One launch,
 *     no workspace, no atomics.  1 <= N <= 32768, 1 <= R * K <= 2^31 - 1, B * ceil(N / tile) <= 2^31 - 1; past that
 *     SVNET_E_UNSUPPORTED.  svnet_pointset_reverse_supported (1 / 0, without the B term), svnet_pointset_reverse_tile (the
 *     destinations one workgroup owns, a quarter of them per wave: the N at which a cloud takes a second workgroup) and
 *     svnet_pointset_reverse_chunk (the edges per LDS chunk: the R * K at which the edge loop takes a second chunk) are pure host
 *     functions.
 * With the edges of list n e_1 < e_2 < ... and the terms t_i below: grad[n] = fl(fl(fl(t_1 + t_2) + t_3) + ...); one term gives t_1, an
 * empty list +0.0, which is written.  Every product and sum is rounded once and never contracted.
 * svnet_three_interpolate_bwd_f32: dout [B,D,P], weight [B,P,3], the reverse lists of idx [B,P,3] -> dfeat [B,D,N];
 *     e_i = 3 p_i + j_i, t_i = fl(dout[d,p_i] weight[p_i,j_i]).  Slots past min(3, N) are ordinary edges (to point 0, weight 0).
 *     No gradient goes to weight or to the coordinates.  1 <= D <= 524280.
 * svnet_group_points_bwd_f32: dgrouped [B,S,nsample,3+D], the reverse lists of idx [B,S,nsample] -> dpoints [B,N,D];
 *     t_i = dgrouped[s_i,j_i,3+c].  Padded slots and the slots of an empty group are ordinary edges.  Columns 0..2 (the gradients of
 *     the coordinates) are not produced.  D >= 1.                                                                                   */
int svnet_pointset_reverse_supported(int64_t R, int64_t K, int64_t N);
int svnet_pointset_reverse_tile(void);
int svnet_pointset_reverse_chunk(void);
int svnet_pointset_reverse_i32(const int64_t* idx, int64_t B, int64_t R, int64_t K, int64_t N, int32_t* rev_start, int32_t* rev_edge,
                               void* stream);
int svnet_three_interpolate_bwd_f32(const float* dout, const float* weight, const int32_t* rev_start, const int32_t* rev_edge, int64_t B,
                                    int64_t D, int64_t N, int64_t P, float* dfeat, void* stream);
int svnet_group_points_bwd_f32(const float* dgrouped, const int32_t* rev_start, const int32_t* rev_edge, int64_t B, int64_t N, int64_t S,
                               int64_t nsample, int64_t D, float* dpoints, void* stream);

/* ------------------------------------------------------------------ multi-scale grouping: one pass over the cloud for R radii
 * (models/utils/pointnet_util.py:210-267 PointNetSetAbstractionMsg).  `scales` = R, 1 .. SVNET_MSG_MAX_SCALES; r2 [R] fp32 and
 * nsample [R] int64 are HOST arrays, read during the call and handed to the kernels by value: no device copy, no host read of device
 * memory, so every call below can be captured.  Ktot = sum nsample[i], off_i = nsample[0] + .. + nsample[i-1].  Radii need not be
 * ascending and may repeat.  Distance, membership, order, padding, the empty group and the clamp are those of the block above:
 * the query and the grouping kernel are the same ones (csrc/group.hip states each once for 1 .. R scales; the single-scale calls
 * launch the one-scale form).
 * svnet_ball_query_msg_f32: xyz [B,N,3], new_xyz [B,S,3] -> idx [B,S,Ktot] int64, count [B,S,R] int32.  A centre's row is the R lists
 *     end to end: columns off_i .. off_i + nsample[i] - 1 and count[..,i] are exactly what svnet_ball_query_f32 gives for
 *     (r2[i], nsample[i]).  One launch: a candidate's distance is computed once, every scale that is not yet full takes its own
 *     ballot, the wave leaves a centre when all its scales are full.  Every index written lies in 0 .. N-1.
 * svnet_group_points_msg_f32: one launch over idx [B,S,Ktot] -> R separate contiguous outputs out_i [B,S,nsample[i],D+3] (out0 .. out3,
 *     the ones past `scales` ignored).  ATTRIBUTES FIRST: columns 0..D-1 = points[idx,:] bit for bit, columns D..D+2 =
 *     fl(xyz[idx,c] - new_xyz[s,c]); D = 0 gives [..,3].  An index outside 0 .. N-1 is clamped into it, never followed.
 * svnet_group_points_msg_bwd_f32: the R upstream gradients dg_i [B,S,nsample[i],D+3] (dg0 .. dg3) and the reverse lists of the
 *     concatenated idx (svnet_pointset_reverse_i32 with R = S, K = Ktot) -> dpoints [B,N,D] by the ordered sum of the block above:
 *     ascending edge e = s Ktot + j, that is per centre scale 0's slots, then scale 1's, ...; t_i = column c (the attributes come
 *     first) of the gradient of the scale slot j lies in.  No float atomic: two runs give the same bits.  D >= 1.
 * 1 <= scales <= 4, every 1 <= nsample[i] <= N <= 32768, S >= 1, D >= 0 (svnet_group_msg_supported: 1 / 0, a pure host function);
 * B * ceil(S / 32) <= 2^31 - 1 workgroups and B * S * Ktot <= 2^31 - 1 are refused in the calls with SVNET_E_UNSUPPORTED.          */
#define SVNET_MSG_MAX_SCALES 4
int svnet_group_msg_supported(int64_t N, int64_t S, int64_t scales, const int64_t* nsample, int64_t D);
int svnet_ball_query_msg_f32(const float* xyz, const float* new_xyz, int64_t B, int64_t N, int64_t S, int64_t scales, const float* r2,
                             const int64_t* nsample, int64_t* idx, int* count, void* stream);
int svnet_group_points_msg_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t B, int64_t N, int64_t S,
                               int64_t scales, const int64_t* nsample, int64_t D, float* out0, float* out1, float* out2, float* out3,
                               void* stream);
int svnet_group_points_msg_bwd_f32(const float* dg0, const float* dg1, const float* dg2, const float* dg3, const int32_t* rev_start,
                                   const int32_t* rev_edge, int64_t B, int64_t N, int64_t S, int64_t scales, const int64_t* nsample, int64_t D,
                                   float* dpoints, void* stream);

/* ------------------------------------------------------------------ fused set-abstraction level for inference: group, shared MLP, max
 * (models/utils/pointnet_util.py:166-267, the eval-mode forward of PointNetSetAbstraction / PointNetSetAbstractionMsg after the query).
 * A level has L layers, 1 <= L <= SVNET_SA_MAX_LAYERS, of 1x1 convolution + BatchNorm (running statistics) + ReLU; its input width is
 * C0 = 3 + D, its layer widths C1 .. CL.  fl() is rounding to fp32; every operation is rounded once.
 * svnet_sa_fold_f32: one layer's convolution W [O,C], b [O] and BatchNorm gamma, beta, running_mean, running_var [O] -> Wf [O,C], bf [O]
 *     (plain, unpadded, caller-owned).  One launch, no host read: it can be captured and repeated after the parameters change.
 *         invstd[o] = fl(1 / fl(sqrt(fl(var[o] + eps))))     (svnet_bn_eval_stats_f32's; division and square root correctly rounded)
 *         s[o] = fl(gamma[o] invstd[o]);   Wf[o,c] = fl(W[o,c] s[o]);   bf[o] = fl(fl(fl(b[o] - mean[o]) s[o]) + beta[o])
 *     never contracted.  1 <= O, 1 <= C, O * C <= 2^31 - 1.
 * svnet_sa_fused_f32: per cloud xyz [N,3], new_xyz [S,3], points [N,D] (NULL when D = 0), idx [S,K] int64 with row stride idx_ld >= K
 *     (a scale's columns of a concatenated table are used where they lie), count [S] int32 with element stride count_ld or NULL;
 *     wf and bf are HOST arrays of L device pointers (the folded layers) and widths a HOST array of the L widths C1 .. CL, read during the
 *     call and handed to the kernel by value: no device copy, no workspace, one launch.
 *         row j of centre s: n = idx[s,j] clamped into 0 .. N-1 (svnet_group_points_f32's clamp); h0 = [fl(xyz[n,c] - new_xyz[s,c]) c = 0..2 |
 *         points[n,:] bit for bit] with xyz_last = 0, [points[n,:] | the three differences] with xyz_last = 1 (the multi-scale order).
 *         per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc > 0 ? acc : +0.
 *         out[b, c_off + o, s] = max_j hL_j[o], channel-first into out [B,C_total,S]; the other channels are left as they are.
 *     The products run on v_mfma_f32_16x16x4_f32, bit for bit that fmaf chain; K is never split, so a value does not depend on how rows,
 *     columns or centres are tiled, and the zero padding of K adds exact zeros.  With count, the slots >= max(count[s], 1) are skipped:
 *     they repeat slot 0 (svnet_ball_query_f32's padding and empty group), so the maximum is that of all slots.  Inputs are assumed
 *     finite.  svnet_sa_fused_supported (1 / 0, a pure host function): 1 <= K <= N <= 32768, S >= 1, 0 <= D <= 321 (C0 <= 324),
 *     1 <= L <= 4, every 1 <= width <= 256.  B * ceil(S / centres per workgroup) <= 2^31 - 1 and B * S * idx_ld <= 2^31 - 1 are refused in
 *     the call with SVNET_E_UNSUPPORTED.  svnet_sa_fused_rows_tile: the grouped rows one workgroup multiplies at a time - a group of
 *     more slots than that takes further tiles, a smaller one shares its tile with the next centres.                                 */
#define SVNET_SA_MAX_LAYERS 4
int svnet_sa_fold_f32(const float* W, const float* b, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, int64_t O, int64_t C, float eps, float* Wf, float* bf, void* stream);
int svnet_sa_fused_supported(int64_t N, int64_t S, int64_t K, int64_t D, int64_t L, const int64_t* widths);
int svnet_sa_fused_rows_tile(void);
int svnet_sa_fused_f32(const float* xyz, const float* new_xyz, const float* points, const int64_t* idx, int64_t idx_ld, const int* count,
                       int64_t count_ld, int64_t B, int64_t N, int64_t S, int64_t K, int64_t D, int64_t L, const int64_t* widths,
                       const void* wf, const void* bf, int xyz_last, float* out, int64_t C_total, int64_t c_off, void* stream);

/* ------------------------------------------------------------------ fused feature-propagation level for inference: interpolate, skip, MLP
 * (models/utils/pointnet_util.py:84-92, the eval-mode forward of PointNetFeaturePropagation behind svnet_three_nn_f32).  A level has L
 * layers, 1 <= L <= SVNET_SA_MAX_LAYERS, of 1x1 convolution + BatchNorm (running statistics) + ReLU, folded by svnet_sa_fold_f32 (a
 * Conv1d weight [O,C,1] is a [O,C] matrix); its input width is C0 = D1 + D2.  fl() is rounding to fp32; every operation is rounded once.
 * svnet_fp_fused_f32: per cloud idx [N,3] int64 and weight [N,3], exactly as svnet_three_nn_f32 writes them; points2 [D2,S], the sampled
 *     level's features, channel-first (svnet_three_interpolate_f32's feat); points1 [D1,N], the skip features, channel-first, or NULL
 *     with D1 = 0; wf, bf, widths as in svnet_sa_fused_f32: HOST arrays read during the call, handed to the kernel by value.  No
 *     device copy, no workspace, one launch.
 *         input row of point p: h0 = [ points1[0..D1-1, p] bit for bit | y[0..D2-1] ], the order of cat([points1, interpolated]), with
 *             y[d] = fl(fl(fl(f[d,i0] w0) + fl(f[d,i1] w1)) + fl(f[d,i2] w2)),  f = points2, w_j = weight[p,j],
 *             i_j = idx[p,j] clamped into 0 .. S-1: svnet_three_interpolate_f32's arithmetic word for word, S < 3 included, where the
 *             empty slots are index 0 with weight 0.
 *         per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc > 0 ? acc : +0.
 *         out[b, c_off + o, p] = hL_p[o], channel-first into out [B,C_total,N]; the other channels are left as they are.
 *     The products run on v_mfma_f32_16x16x4_f32, bit for bit that fmaf chain; K is never split, so a value does not depend on how rows
 *     or columns are tiled, and the zero padding of K adds exact zeros.  Inputs are assumed finite.
 *     svnet_fp_fused_supported (1 / 0, a pure host function): N >= 1, 1 <= S <= 32768, D1 >= 0, D2 >= 1, D1 + D2 <= 1536, 1 <= L <= 4,
 *     every 1 <= width <= 256, ceil(N / rows) <= 2^31 - 1.  B * ceil(N / rows) > 2^31 - 1 is refused in the call with
 *     SVNET_E_UNSUPPORTED.  svnet_fp_fused_rows_tile: the consecutive points one workgroup takes - the largest of 64, 32 and 16 whose two
 *     activation buffers fit in 160 KB of LDS; 0 outside the limits on D1, D2, L and the widths.                                      */
int svnet_fp_fused_supported(int64_t N, int64_t S, int64_t D1, int64_t D2, int64_t L, const int64_t* widths);
int svnet_fp_fused_rows_tile(int64_t D1, int64_t D2, int64_t L, const int64_t* widths);
int svnet_fp_fused_f32(const int64_t* idx, const float* weight, const float* points2, const float* points1, int64_t B, int64_t N, int64_t S,
                       int64_t D1, int64_t D2, int64_t L, const int64_t* widths, const void* wf, const void* bf, float* out, int64_t C_total,
                       int64_t c_off, void* stream);

/* ------------------------------------------------------------------ fused global set-abstraction level for inference: all points, shared MLP, max
 * (models/utils/pointnet_util.py:49-63 with group_all, the eval-mode forward of PointNetSetAbstraction behind sample_and_group_all: one
 * group of all N points of a cloud, coordinates first and NOT centred - the reference subtracts nothing there).  A level has L layers,
 * 1 <= L <= SVNET_SA_MAX_LAYERS, of 1x1 convolution + BatchNorm (running statistics) + ReLU, folded by svnet_sa_fold_f32; its input width
 * is C0 = 3 + D.  fl() is rounding to fp32; every operation is rounded once, nothing is contracted but the stated fmaf.
 * svnet_sa_global_f32: per cloud xyz [3,N] and points [D,N] (NULL with D = 0), channel-first as the module receives them: no transposed
 *     copy is made; wf, bf, widths as in svnet_sa_fused_f32: HOST arrays read during the call, handed to the kernel by value.
 *         row p, 0 <= p < N: h0 = [ xyz[0..2, p] | points[0..D-1, p] ], bit for bit.
 *         per layer and output o: acc = bf[o]; for c ascending acc = fmaf(h[c], Wf[o,c], acc); h'[o] = acc > 0 ? acc : +0.
 *         out[b, c_off + o] = max over p in [0, N) of hL_p[o], into out [B,C_total] (that is [B,C_total,1]); the other channels are left
 *         as they are.
 *     The products run on v_mfma_f32_16x16x4_f32, bit for bit that fmaf chain; K is never split, so no value depends on how rows, columns
 *     or clouds are tiled, and the zero padding of K adds exact zeros.  A workgroup takes svnet_sa_global_rows_tile consecutive points
 *     of a cloud; the rows of its tile past N never enter the maximum (a zero row is not neutral: its output is the ReLU of the bias
 *     chain).  The workgroups of a cloud meet in out by an unsigned-integer maximum on the bit patterns - the values are >= +0, such
 *     floats order as their bit patterns, and an integer maximum has no order: the bits are reproducible; there are no float atomics -
 *     after a first small launch of the same call has set exactly the channels c_off .. c_off + C_L - 1 of every cloud to +0.  Two
 *     launches on `stream`, no workspace, no host read: capturable.  Inputs are assumed finite.
 *     svnet_sa_global_supported (1 / 0, a pure host function): 1 <= N <= 32768, 0 <= D <= 1024, 1 <= L <= 4, every 1 <= width <= 1024.
 *     B * ceil(N / rows) > 2^31 - 1 is refused in the call with SVNET_E_UNSUPPORTED.
 *     svnet_sa_global_rows_tile (a pure host function): rows = the largest of 64, 48, 32 and 16 with
 *         4 rows (stride0 + stride1) + 4 pad16(C_L) <= 160 KB of LDS,
 *     where buffer l & 1 holds layer l's input rows, stride_p is the widest row of buffer p padded to a multiple of 4 floats and, where
 *     that is a multiple of 8, by 4 more (csrc/mlp_tile.h), and pad16 rounds up to a multiple of 16; 0 outside the limits on D, L and
 *     the widths.  The whole envelope fits at 16 rows (D 1024, four layers of 1024: 16 x 2056 floats + 1024 maxima = 133 KB).           */
int svnet_sa_global_supported(int64_t N, int64_t D, int64_t L, const int64_t* widths);
int svnet_sa_global_rows_tile(int64_t D, int64_t L, const int64_t* widths);
int svnet_sa_global_f32(const float* xyz, const float* points, int64_t B, int64_t N, int64_t D, int64_t L, const int64_t* widths,
                        const void* wf, const void* bf, float* out, int64_t C_total, int64_t c_off, void* stream);

/* ------------------------------------------------------------------ fused vector-neuron edge level for inference: tables, leaky rule, mean
 * (models/vn_layers.py:50-78, the eval-mode forward of VNLinearLeakyReLU over 2C -> O vector channels, on the edge feature
 * [x_j - x_i | x_i] of models/utils/vn_util.py:23-49 get_graph_feature, followed by mean_pool over the k neighbours: one edge level of
 * models/vn_dgcnn_cls.py with pooling = 'mean').  The level is linear in the edge feature in front of its non-linearity,
 * W [x_j - x_i | x_i] = W_a x_j + (W_b - W_a) x_i, so the products are taken once per point and an edge adds two table rows.
 * fl() is rounding to fp32; every operation is rounded once, nothing is contracted but the stated fmaf.  EPS = fl(1e-6).
 * Od is the number of direction rows: O, or 1 (share_nonlinearity: every o uses row 0).  R = 2 (O + Od).
 * svnet_vn_fold_f32: w_feat [O,2C] (map_to_feat.weight), w_dir [Od,2C] (map_to_dir.weight), BatchNorm gamma, beta, running_mean,
 *     running_var [O] -> folded, C R + 2 O floats, caller-owned: WT [C][R] | s [O] | t [O].  One launch, no host read.
 *         A_f = w_feat[:, :C], D_f = fl(w_feat[:, C:] - w_feat[:, :C]); A_d, D_d likewise from w_dir; column r of WT is row r of
 *         [A_f | A_d | D_f | D_d];  invstd = fl(1 / fl(sqrt(fl(var + eps)))), s = fl(gamma invstd), t = fl(beta - fl(mean s)).
 * svnet_vn_tables_f32: x [B,C,3,N] -> workspace [TN | TC], each [B][N][3 (O + Od)] floats.  Per point n, component a and row:
 *     a c-ascending chain acc = +0; acc = fmaf(x[c,a,n], M[row,c], acc) - Pn with M = A_f, Qn with A_d (into TN), Pc with D_f, Qc with
 *     D_d (into TC).  A table row is [P: a O + o | Q: 3 O + a Od + od].  K is never split: no value depends on tiling.  One launch.
 * svnet_vn_edge_mean_f32: the tables, idx [B,N,k] int64 and folded -> out [B,O,3,N].  Per edge (n, j), m = idx[n,j] clamped into
 *     0 .. N-1, per o (od = o, or 0 with Od = 1):
 *         p[a] = fl(Pn[m,o,a] + Pc[n,o,a]);  d[a] = fl(Qn[m,od,a] + Qc[n,od,a])
 *         q = fmaf(p2, p2, fmaf(p1, p1, fl(p0 p0)));  r = fl(fl(sqrt(q)) + EPS);  nb = fmaf(r, s[o], t[o]);  g = fl(nb / r);  p'[a] = fl(p[a] g)
 *         dot = fmaf(p'2, d2, fmaf(p'1, d1, fl(p'0 d0)));  dd = fmaf(d2, d2, fmaf(d1, d1, fl(d0 d0)))
 *         w = p' if dot >= 0, else c = fl(dot / fl(dd + EPS)) and w[a] = fmaf(-c, d[a], p'[a])
 *         y[a] = fmaf(slope, p'[a], fl(fl(1 - slope) w[a]))
 *     out[o,a,n] = fl((sum over j ascending from +0 of y_j[o,a]) / fl(k)).  One launch, no host read, no atomics: capturable,
 *     reproducible.  Inputs are assumed finite.
 * svnet_vn_supported (1 / 0, a pure host function): 1 <= k <= 64, k <= N <= 32768, 1 <= C <= 128, 1 <= O <= 128, Od = O or 1.
 * svnet_vn_workspace_bytes (a pure host function): 2 B N 3 (O + Od) floats in bytes; 0 outside the limits.  B > 65535 is refused by
 *     the tables call with SVNET_E_ARG, B * ceil(N / 16) > 2^31 - 1 by the edge call with SVNET_E_UNSUPPORTED.                       */
int svnet_vn_supported(int64_t N, int64_t k, int64_t C, int64_t O, int64_t Od);
size_t svnet_vn_workspace_bytes(int64_t B, int64_t N, int64_t O, int64_t Od);
int svnet_vn_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, int64_t C, int64_t O, int64_t Od, float eps, float* folded, void* stream);
int svnet_vn_tables_f32(const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, int64_t Od, float* workspace,
                        size_t workspace_bytes, void* stream);
int svnet_vn_edge_mean_f32(const float* workspace, size_t workspace_bytes, const int64_t* idx, const float* folded, int64_t B, int64_t N,
                           int64_t k, int64_t C, int64_t O, int64_t Od, float slope, float* out, void* stream);

/* ------------------------------------------------------------------ fused vector-neuron tail for inference: point level, cloud mean, standardise and pool
 * (models/vn_dgcnn_cls.py tail: conv5, the mean over the points, VNStdFeature (models/vn_layers.py) with normalize_frame = False and
 * the [amax | mean] pool, in eval mode).  fl() is rounding to fp32; every operation is rounded once, nothing is contracted but the
 * stated fmaf.  EPS = fl(1e-6).  Inputs are assumed finite.  Every call launches on `stream`, reads nothing back and uses no atomics:
 * capturable, reproducible.
 * POINT LEVEL: the eval forward of a VNLinearLeakyReLU on [B, C + Cg, 3, N] whose last Cg input channels are constant over each cloud
 * and are given as g [B,Cg,3] (Cg may be 0: g and workspace may then be null).  K = C + Cg, Od = O or 1 (share_nonlinearity: every o uses
 * direction row 0), R = O + Od.
 * svnet_vn_point_fold_f32: w_feat [O,K] (map_to_feat.weight), w_dir [Od,K] (map_to_dir.weight), BatchNorm gamma, beta, running_mean,
 *     running_var [O] -> folded, K R + 2 O floats, caller-owned: WT [K][R] | s [O] | t [O]; column r of WT is row r of W = [w_feat | w_dir]
 *     stacked; invstd = fl(1 / fl(sqrt(fl(var + eps)))), s = fl(gamma invstd), t = fl(beta - fl(mean s)), as svnet_vn_fold_f32.  One launch.
 * svnet_vn_point_f32: x [B,C,3,N], g [B,Cg,3], folded -> out [B,O,3,N].  One launch, and one small launch in front of it with Cg > 0.
 *         cloud term   per cloud b, row r of W and component a: u = +0; for c ascending over Cg: u = fmaf(g[b,c,a], W[r, C + c], u).
 *                      It lies in the workspace, [B][3][R] floats.
 *         point term   per (b, n, a) and row r: acc = u[b,r,a] (+0 with Cg = 0); for c ascending over C: acc = fmaf(x[b,c,a,n], W[r,c], acc).
 *                      K is never split: no value depends on tiling.  p[o,a] are the w_feat rows, d[od,a] the w_dir rows (od = o, or 0).
 *         norm, leaky  the edge level's arithmetic (svnet_vn_edge_mean_f32 above) on p and d:
 *                      q = fmaf(p2, p2, fmaf(p1, p1, fl(p0 p0)));  r = fl(fl(sqrt(q)) + EPS);  nb = fmaf(r, s[o], t[o]);  g = fl(nb / r);  p'[a] = fl(p[a] g)
 *                      dot = fmaf(p'2, d2, fmaf(p'1, d1, fl(p'0 d0)));  dd = fmaf(d2, d2, fmaf(d1, d1, fl(d0 d0)))
 *                      w = p' if dot >= 0, else c = fl(dot / fl(dd + EPS)) and w[a] = fmaf(-c, d[a], p'[a])
 *                      out[b,o,a,n] = fmaf(slope, p'[a], fl(fl(1 - slope) w[a])).
 * svnet_vn_point_supported (1 / 0, a pure host function): 1 <= N <= 32768, 1 <= C <= 512, 0 <= Cg <= 512, 1 <= O <= 512, Od = O or 1.
 * svnet_vn_point_workspace_bytes (a pure host function): 3 B R floats in bytes with Cg > 0, else 0; 0 outside the limits or 1 <= B <= 65535.
 * CLOUD MEAN: svnet_vn_cloud_mean_f32: x [B,C,3,N] -> m [B,C,3].  The order is the contract's, not the tiling's: run j holds n in
 *     [64 j, min(N, 64 j + 64)); a run's sum is n-ascending plain additions from +0; m = fl((the runs' sums added j-ascending from +0) / fl(N)).
 *     1 <= N <= 32768, 1 <= C <= 512.  One launch.
 * STANDARDISE AND POOL: svnet_vn_std_pool_f32: x [B,C,3,N], g [B,Cg,3] (constant channels; null with Cg = 0), y [B,Cy,3,N] (vn2's output),
 *     w_lin [3,Cy] (vn_lin.weight) -> h [B, 6 I], I = C + Cg.
 *         frame rows   z[k][a](n) = +0; for c ascending over Cy: z = fmaf(y[b,c,a,n], w_lin[k,c], z).
 *         coordinates  v_i = x[b,i,:,n] for i < C, g[b,i-C,:] otherwise: e[i,k](n) = fmaf(v_i[2], z[k][2], fmaf(v_i[1], z[k][1], fl(v_i[0] z[k][0]))).
 *         pool         h[b, 3 i + k] = max over n of e (a -0 counts as +0); h[b, 3 I + 3 i + k] = the mean of e under the cloud-mean rule.
 *     The workgroups of a cloud meet through per-run maxima and sums in the workspace, [2][runs][B][3 I] floats with runs = ceil(N / 64), and
 *     a finishing launch that adds the runs' sums in order.  Two launches.
 * svnet_vn_std_pool_supported (1 / 0, a pure host function): 1 <= N <= 32768, 1 <= C <= 512, 0 <= Cg <= 512, 1 <= Cy <= 512.
 * svnet_vn_std_pool_workspace_bytes (a pure host function): 2 ceil(N / 64) B 3 (C + Cg) floats in bytes; 0 outside the limits or 1 <= B <= 65535.
 * Errors: a null pointer or B outside 1 .. 65535 is SVNET_E_ARG, a shape outside the limits SVNET_E_UNSUPPORTED, a short workspace
 * SVNET_E_WORKSPACE; svnet_last_error names the entry.                                                                               */
int svnet_vn_point_supported(int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od);
size_t svnet_vn_point_workspace_bytes(int64_t B, int64_t Cg, int64_t O, int64_t Od);
int svnet_vn_point_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, int64_t C, int64_t Cg, int64_t O, int64_t Od, float eps, float* folded, void* stream);
int svnet_vn_point_f32(const float* x, const float* g, const float* folded, int64_t B, int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od,
                       float slope, void* workspace, size_t workspace_bytes, float* out, void* stream);
int svnet_vn_cloud_mean_f32(const float* x, int64_t B, int64_t C, int64_t N, float* m, void* stream);
int svnet_vn_std_pool_supported(int64_t N, int64_t C, int64_t Cg, int64_t Cy);
size_t svnet_vn_std_pool_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t Cg);
int svnet_vn_std_pool_f32(const float* x, const float* g, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cg,
                          int64_t Cy, void* workspace, size_t workspace_bytes, float* h, void* stream);

/* ------------------------------------------------------------------ fused two-layer vector-neuron edge level for inference: two layers per edge, mean
 * (models/vn_dgcnn_partseg.py: get_graph_feature -> conv1 -> conv2 -> pool1 and conv3 -> conv4 -> pool2 with pooling = 'mean', in eval
 * mode: two VNLinearLeakyReLU layers per edge in front of the mean over the k neighbours).  Layer 1 (C -> O1, Od1 direction rows) is the
 * edge level above: its tables come from svnet_vn_tables_f32 with svnet_vn_fold_f32's folded1.  Layer 2 (O1 -> O2, Od2 direction rows)
 * acts on layer 1's non-linear output, a dense product per edge; it is folded by svnet_vn_point_fold_f32 with Cg = 0:
 * folded2 = WT [O1][O2 + Od2] | s2 [O2] | t2 [O2].  The conventions (fl(), fmaf, EPS, Od) are the edge level's.
 * svnet_vn_edge2_mean_f32: layer 1's tables (workspace), idx [B,N,k] int64, folded1, folded2 -> out [B,O2,3,N].  Per edge (n, j),
 *     m = idx[n,j] clamped into 0 .. N-1:
 *         layer 1   y1[c,a], c < O1: svnet_vn_edge_mean_f32's per-edge y (edge, norm, leaky on folded1 with slope1), before its sum.
 *         layer 2   per row r of W2 = [w_feat2 | w_dir2] stacked and component a: acc = +0; for c ascending over O1:
 *                   acc = fmaf(y1[c,a], W2[r,c], acc).  K is never split: no value depends on tiling.  p[o,a] are the w_feat2 rows,
 *                   d[od,a] the w_dir2 rows (od = o, or 0 with Od2 = 1);  y2 = the norm / leaky rule on p, d, s2[o], t2[o] with slope2.
 *     out[b,o,a,n] = fl((sum over j ascending from +0 of y2_j[o,a]) / fl(k)).  One launch that writes 3 O2 floats per point and nothing
 *     else: layer 1's outputs stay on the chip.  No host read, no atomics: capturable, reproducible.  Inputs are assumed finite.
 * svnet_vn_edge2_supported (1 / 0, a pure host function): 1 <= k <= 64, k <= N <= 32768, 1 <= C, O1, O2 <= 128, Od1 = O1 or 1, Od2 = O2 or 1.
 * Errors as svnet_vn_edge_mean_f32: a null pointer or B < 1 is SVNET_E_ARG, a shape outside the limits SVNET_E_UNSUPPORTED (as is
 * B * ceil(N / P) > 2^31 - 1 workgroups, P >= 1 the points of one), a workspace below svnet_vn_workspace_bytes(B, N, O1, Od1)
 * SVNET_E_WORKSPACE; svnet_last_error names the entry.                                                                              */
int svnet_vn_edge2_supported(int64_t N, int64_t k, int64_t C, int64_t O1, int64_t Od1, int64_t O2, int64_t Od2);
int svnet_vn_edge2_mean_f32(const float* workspace, size_t workspace_bytes, const int64_t* idx, const float* folded1, const float* folded2,
                            int64_t B, int64_t N, int64_t k, int64_t C, int64_t O1, int64_t Od1, int64_t O2, int64_t Od2,
                            float slope1, float slope2, float* out, void* stream);

/* ------------------------------------------------------------------ frame coordinates per point (models/vn_dgcnn_partseg.py: the einsum of the
 * levels' features with VNStdFeature's frame, unpooled).  svnet_vn_std_coords_f32: x [B,C,3,N], y [B,Cy,3,N] (vn2's output), w_lin [3,Cy]
 * (vn_lin.weight) -> e [B,3C,N]: e[b, 3 i + k, n] = the coordinates rule of svnet_vn_std_pool_f32 on v_i = x[b,i,:,n] and its frame rows
 * z[k] - the same device functions, so max over n of e is that entry's h[b, 3 i + k] bit for bit.  One launch, stores along n, no host
 * read, no atomics.  svnet_vn_std_coords_supported (1 / 0, a pure host function): 1 <= N <= 32768, 1 <= C <= 512, 1 <= Cy <= 512.
 * Errors: a null pointer or B outside 1 .. 65535 is SVNET_E_ARG, a shape outside the limits SVNET_E_UNSUPPORTED.                       */
int svnet_vn_std_coords_supported(int64_t N, int64_t C, int64_t Cy);
int svnet_vn_std_coords_f32(const float* x, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cy, float* e,
                            void* stream);

/* ------------------------------------------------------------------ fused vector-neuron cross edge level for inference
 * (models/vn_pointnet_cls.py: get_graph_feature_cross -> conv_pos -> mean over k with pooling = 'mean', in eval mode: a VNLinearLeakyReLU
 * over 3 -> O vector channels on the edge feature [x_j - x_i | x_i | x_j x x_i] of models/utils/vn_util.py:52-76, the cloud being ONE
 * vector channel).  The cross product depends on the pair, so there are no point tables: one launch computes the feature per edge.
 * svnet_vn_cross_fold_f32: w_feat [O,3] (map_to_feat.weight), w_dir [Od,3] (map_to_dir.weight), BatchNorm gamma, beta, running_mean,
 *     running_var [O] -> folded, 3 (O + Od) + 2 O floats: W [O + Od][3] = [W_f | W_d] stacked | s [O] | t [O], s and t as svnet_vn_fold_f32.
 *     One launch.
 * svnet_vn_edge_cross_mean_f32: x [B,1,3,N], idx [B,N,k] int64, folded -> out [B,O,3,N].  Per edge (n, j), m = idx[n,j] clamped into
 *     0 .. N-1 before any address is formed, xi = x[:,n], xj = x[:,m], every operation rounded once to fp32:
 *         edge     e0[a] = xj[a] - xi[a];  e1[a] = xi[a];  e2 = xj x xi: e2[0] = fl(xj[1] xi[2]) - fl(xj[2] xi[1]),
 *                  e2[1] = fl(xj[2] xi[0]) - fl(xj[0] xi[2]),  e2[2] = fl(xj[0] xi[1]) - fl(xj[1] xi[0]).
 *         product  per row r of W and component a: acc = +0; for c = 0, 1, 2: acc = fmaf(e_c[a], W[r,c], acc).  p = the W_f rows, d the
 *                  W_d rows (row 0 for every o with Od = 1).
 *         norm, leaky, mean   as svnet_vn_edge_mean_f32 above, on p, d, s[o], t[o] and slope.
 *     One launch that writes 3 O floats per point and nothing else; no workspace, no atomics, no host read; capturable.
 * svnet_vn_cross_supported (1 / 0, a pure host function): 1 <= k <= 64, k <= N <= 32768, 1 <= O <= 128, Od = O or 1.
 * Errors: a null pointer or B outside 1 .. 65535 is SVNET_E_ARG, a shape outside the limits SVNET_E_UNSUPPORTED.                       */
int svnet_vn_cross_supported(int64_t N, int64_t k, int64_t O, int64_t Od);
int svnet_vn_cross_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                            const float* running_var, int64_t O, int64_t Od, float eps, float* folded, void* stream);
int svnet_vn_edge_cross_mean_f32(const float* x, const int64_t* idx, const float* folded, int64_t B, int64_t N, int64_t k, int64_t O, int64_t Od,
                                 float slope, float* out, void* stream);

/* ------------------------------------------------------------------ norm-only vector-neuron point layer (models/vn_pointnet_cls.py: bn3(conv3(x)),
 * a VNLinear followed by a VNBatchNorm with no leaky rule, in eval mode).  The point kernel of svnet_vn_point_f32 with its epilogue
 * exchanged: no direction rows, no constant channels.
 * svnet_vn_point_norm_fold_f32: w_feat [O,C], BatchNorm gamma, beta, running_mean, running_var [O] -> folded, C O + 2 O floats:
 *     WT [C][O] | s [O] | t [O].  One launch.
 * svnet_vn_point_norm_f32: x [B,C,3,N], folded -> out [B,O,3,N]: the point term of svnet_vn_point_f32 with u = +0 (the c-ascending fmaf
 *     chain over C, K never split), then q, r, g of the norm rule and out[o,a,n] = fl(p[a] g).  One launch.
 * svnet_vn_point_norm_supported (1 / 0, a pure host function): 1 <= N <= 32768, 1 <= C <= 512, 1 <= O <= 512.
 * Errors: a null pointer or B outside 1 .. 65535 is SVNET_E_ARG, a shape outside the limits SVNET_E_UNSUPPORTED.                       */
int svnet_vn_point_norm_supported(int64_t N, int64_t C, int64_t O);
int svnet_vn_point_norm_fold_f32(const float* w_feat, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                 int64_t C, int64_t O, float eps, float* folded, void* stream);
int svnet_vn_point_norm_f32(const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, float* out, void* stream);

/* ------------------------------------------------------------------ the wide envelope of the vector-neuron tail (models/vn_pointnet_partseg.py:
 * conv5 + bn5 170 -> 682, std_feature over 682 + 682 channels).  THE NAMING RULE: every entry of the three sections above that begins
 * svnet_vn_point_, svnet_vn_point_norm_, svnet_vn_cloud_mean_, svnet_vn_std_pool_ or svnet_vn_std_coords_ has a twin whose name carries
 * _wide behind that stem: svnet_vn_point_wide_f32, svnet_vn_point_norm_wide_fold_f32, svnet_vn_std_pool_wide_workspace_bytes ...  A twin has
 * its entry's arguments, buffers, contract (cloud term first, c ascending, K never split, runs of 64, the norm and leaky rules), launches
 * and errors, word for word, and one other envelope, shared by all of them:
 *     1 <= C, O, Cy <= 768, 0 <= Cg <= 768, 1 <= N <= 32768, 1 <= B <= 65535, Od = O or 1.
 * The workspace formulas are the entries' own: svnet_vn_point_wide_workspace_bytes = 3 B (O + Od) floats in bytes with Cg > 0, else 0;
 * svnet_vn_std_pool_wide_workspace_bytes = 2 ceil(N / 64) B 3 (C + Cg) floats in bytes; 0 outside the wide limits.
 * Inside the base envelope a twin runs the kernel its entry runs and returns its bits; the base entries keep refusing 513.  Above 512
 * channels the point kernel holds one image of x at 16 points per workgroup (4 x 48 C bytes of LDS: 131 KB at 682, 144 KB at 768).      */
int svnet_vn_point_wide_supported(int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od);
size_t svnet_vn_point_wide_workspace_bytes(int64_t B, int64_t Cg, int64_t O, int64_t Od);
int svnet_vn_point_wide_fold_f32(const float* w_feat, const float* w_dir, const float* gamma, const float* beta, const float* running_mean,
                                 const float* running_var, int64_t C, int64_t Cg, int64_t O, int64_t Od, float eps, float* folded, void* stream);
int svnet_vn_point_wide_f32(const float* x, const float* g, const float* folded, int64_t B, int64_t N, int64_t C, int64_t Cg, int64_t O, int64_t Od,
                            float slope, void* workspace, size_t workspace_bytes, float* out, void* stream);
int svnet_vn_point_norm_wide_supported(int64_t N, int64_t C, int64_t O);
int svnet_vn_point_norm_wide_fold_f32(const float* w_feat, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                                      int64_t C, int64_t O, float eps, float* folded, void* stream);
int svnet_vn_point_norm_wide_f32(const float* x, const float* folded, int64_t B, int64_t N, int64_t C, int64_t O, float* out, void* stream);
int svnet_vn_cloud_mean_wide_f32(const float* x, int64_t B, int64_t C, int64_t N, float* m, void* stream);
int svnet_vn_std_pool_wide_supported(int64_t N, int64_t C, int64_t Cg, int64_t Cy);
size_t svnet_vn_std_pool_wide_workspace_bytes(int64_t B, int64_t N, int64_t C, int64_t Cg);
int svnet_vn_std_pool_wide_f32(const float* x, const float* g, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cg,
                               int64_t Cy, void* workspace, size_t workspace_bytes, float* h, void* stream);
int svnet_vn_std_coords_wide_supported(int64_t N, int64_t C, int64_t Cy);
int svnet_vn_std_coords_wide_f32(const float* x, const float* y, const float* w_lin, int64_t B, int64_t N, int64_t C, int64_t Cy, float* e,
                                 void* stream);

/* ------------------------------------------------------------------ fused binary chain for inference (models/bipointnet.py in eval mode:
 * the shared binary MLP of BiSTN3d, BiSTNkd and BiPointNetEncoder - Conv1d(BiLinearLSR) + BatchNorm1d + hardtanh per layer - with its
 * optional bmm(x^T, T) in front and its maximum over the cloud behind).  fl() is rounding to fp32; every operation is rounded once;
 * nothing is contracted but the stated fmaf; inputs are assumed finite.  sgn(0) = 0: ternary, as everywhere in this library.
 * svnet_bi_fold_f32: one BiLinearLSR W [O,K], its 0-dim scale (a device pointer) and BatchNorm gamma, beta, running_mean, running_var
 *     [O] - or all four NULL - in one launch of one workgroup, no host read:
 *         S = the float64 sum of W: lane t of 1024 adds W[t], W[t + 1024], .. in that order (row-major flat index), then the tree
 *             sh[i] += sh[i + s] for s = 512, 256 .. 1;   m = fl(S / (O K)) (the float64 quotient, rounded once)
 *         S[o,k] = sgn(fl(W[o,k] - m))
 *         with BatchNorm: invstd and s = fl(gamma invstd) as svnet_sa_fold_f32; a[o] = fl(scale s[o]); b[o] = fl(beta[o] - fl(mean[o] s[o]))
 *         without: a[o] = scale, b[o] = +0
 *     -> w_i8 (NULL to skip; svnet_bi_packed_bytes(O, K) bytes, K <= 512, the signs as int8 [32 ceil(O/32)][32 ceil(K/32)], zero filled,
 *        O <= 2048), the form svnet_bi_chain_f32 reads; s_f32 (NULL to skip): the signs as floats [O,K], for svnet_binweight_prepare_f32
 *        and the existing binary linear entries (the fully connected layers behind a maximum); ab: a [O] | b [O].  O K <= 2^24.
 * svnet_bi_chain_f32: x [B,C0,N] channel-first, trans [B,C0,C0] or NULL, L layers of widths[l] (a HOST array), w and ab HOST arrays of L
 *     device pointers: a binary layer's w_i8 and a | b; with first_fp the first layer's Wf [O,C0] and bf [O] of svnet_sa_fold_f32 (the
 *     Linear's bias is its b).  Per cloud and point n:
 *         u[j] = x[j,n] bit for bit without trans; with it u[j] = +0, then for c ascending u[j] = fmaf(x[c,n], trans[c,j], u[j])
 *         fp layer:      t[o] = bf[o]; for c ascending t[o] = fmaf(u[c], Wf[o,c], t[o])
 *         binary layer:  d[o] = sum_c sgn(h[c]) S[o,c], an exact integer; t[o] = fmaf((float)d[o], a[o], b[o]); the next layer reads h = t
 *         pool = 0:      out[b,o,n] = t[o], clamped into [-1,1] with clamp set, out [B,O,N]
 *         pool = 1:      out[b,o] = fl(max over n < N of t_n[o] + offset), out [B,O]; order-free, no float atomics: the kernel keeps
 *                        the integer extreme of d per channel and tile (max where a >= 0, min where a < 0: t is monotone in d), a
 *                        cloud of more than svnet_bi_chain_rows_tile points combines its tiles' partial maxima in a finishing launch
 *                        of the same call, through `workspace` (svnet_bi_chain_workspace_bytes(B, N, O): 0 for one tile).
 *     No host read, no atomics; capturable; two runs give the same bits.
 * svnet_bi_chain_supported (1 / 0, a pure host function): 1 <= N <= 32768, 1 <= L <= 4, C0 <= 64 with trans or first_fp, the fp layer's
 *     width <= 512, every binary layer's input width <= 512, the last width <= 2048.
 * Errors: a null pointer, B outside 1 .. 65535 or a workspace that is too small is SVNET_E_ARG, a shape outside the limits
 * SVNET_E_UNSUPPORTED.                                                                                                             */
size_t svnet_bi_packed_bytes(int64_t O, int64_t K);
int svnet_bi_fold_f32(const float* W, const float* scale, const float* gamma, const float* beta, const float* running_mean,
                      const float* running_var, int64_t O, int64_t K, float eps, int8_t* w_i8, float* s_f32, float* ab, void* stream);
int svnet_bi_chain_supported(int64_t C0, int64_t N, int64_t L, const int64_t* widths, int first_fp, int has_trans);
int svnet_bi_chain_rows_tile(void);
size_t svnet_bi_chain_workspace_bytes(int64_t B, int64_t N, int64_t O);
int svnet_bi_chain_f32(const float* x, const float* trans, int64_t B, int64_t C0, int64_t N, int64_t L, const int64_t* widths, int first_fp,
                       const void* w, const void* ab, int pool, int clamp, float offset, void* workspace, size_t workspace_bytes, float* out,
                       void* stream);

/* ------------------------------------------------------------------ epoch metrics (main_cls_dgcnn.py:187-251, main_partseg_dgcnn.py:185-279,
 * utils.py:68-91 calculate_shape_IoU; the accuracy scores of sklearn.metrics are functions of the confusion matrix)
 * Both forms ACCUMULATE into a caller-owned device state and hand nothing to the host:
 *     state, as int64 words: conf[C*C] (row = true class, column = predicted class) | rows | invalid | loss_sum (a float64)
 * svnet_metrics_state_bytes gives its size; svnet_metrics_reset zero-fills it and marks all `capacity` shape slots empty (one launch).
 * Per valid row: the prediction is the LOWEST index among the row's maxima, a NaN counting as the maximum (torch.max over a dim on the
 * CPU), and loss_sum grows by the row's cal_loss term in the fp32 arithmetic of svnet_smooth_ce_f32 (csrc/smooth_ce.h).  A row whose target lies outside
 * 0 .. C-1 (the batch assembly's -1 poison included) indexes nothing: it is counted in `invalid` and otherwise skipped.  Integer counts
 * are integer atomics; loss_sum is added in a fixed order by a finishing launch of the same call (no float atomics): two identical
 * passes give identical bits.  `count`: the valid leading rows / clouds (0: nothing is launched).  `workspace`: scratch of
 * svnet_metrics_workspace_bytes for B rows (N = 0, the cls form) or B clouds of N points (the seg form); contents need not survive.
 *
 * cls: logits [R,C], target [R].
 * seg: logits [B,num_part,N] (the part-segmentation models' layout; rows = points, C = num_part), seg [B,N], label [B];
 *      part_start / part_num [num_cat] (device): the parts of category c are part_start[c] .. part_start[c] + part_num[c] - 1.
 *      Per valid cloud b, over ALL its points with the prediction taken over all num_part channels: for each part p of the cloud's
 *      category I = #(pred == p and seg == p), U = #(pred == p or seg == p), part IoU = 1 when U == 0, else I / U in float64;
 *      shape_iou[first + b] = (sum over p ascending) / part_num, shape_cat[first + b] = label[b].  A label outside 0 .. num_cat-1 (or
 *      a part range outside 0 .. num_part-1): shape_iou = NaN, shape_cat = SVNET_METRICS_CAT_INVALID.  first + count > capacity is
 *      refused with SVNET_E_UNSUPPORTED, as are num_part > 4096 and B > 65535.                                                      */
#define SVNET_METRICS_CAT_EMPTY (-1)   /* shape_cat of a slot no call has filled since the reset */
#define SVNET_METRICS_CAT_INVALID (-2) /* shape_cat of a cloud whose label was out of range */
size_t svnet_metrics_state_bytes(int64_t C);
size_t svnet_metrics_workspace_bytes(int64_t B, int64_t C, int64_t N);
int svnet_metrics_reset(void* state, int64_t C, double* shape_iou, int64_t* shape_cat, int64_t capacity, void* stream);
int svnet_metrics_cls_f32(const float* logits, const int64_t* target, int64_t R, int64_t C, int64_t count, float eps, void* state,
                          void* workspace, size_t workspace_bytes, void* stream);
int svnet_metrics_seg_f32(const float* logits, const int64_t* seg, const int64_t* label, int64_t B, int64_t num_part, int64_t N,
                          const int64_t* part_start, const int64_t* part_num, int64_t num_cat, int64_t count, int64_t first, float eps,
                          void* state, double* shape_iou, int64_t* shape_cat, int64_t capacity, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ------------------------------------------------------------------ diagnostics (no reference counterpart)
 * One thread writes the constant-rate device clock (s_memrealtime: 100 MHz ticks) to *slot when the stream reaches it: the start
 * times of a captured step's launches WITHOUT a profiler (svnet_amd._lib.StepClock, tools/step_clock.py).                          */
int svnet_stamp_u64(uint64_t* slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVNET_HIP_H */
