/* roreg_hip.h -- C-ABI of libroreg_hip.so: the MI355X (gfx950) kernels behind RoReg's per-pair
 * registration hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name ends in _host; buffers are owned by the caller;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); nothing synchronises;
 *   - every entry point returns 0 on success, non-zero on failure (roreg_last_error() has the text);
 *   - tensors are C-contiguous; "f32 [B,C,60]" means float32 with 60 fastest;
 *   - group tables (P 60x60, Nei 60x13) are uploaded once with roreg_set_group_tables().
 *
 * Each entry cites the reference code it replaces (paths relative to the RoReg checkout).
 */
#ifndef ROREG_HIP_H
#define ROREG_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------------ */
/* Version of THIS header.  It is bumped whenever an existing entry point changes its argument list or a shared struct its size
 * (2: round 2's per-keypoint block scales -- roreg_gf_finalize, roreg_inv_descriptor, roreg_et_gather, roreg_dense_split/_f16x2,
 * roreg_lt_prepare_batch, roreg_group_conv_f16x2, roreg_lt_task 80 -> 96 bytes; 3: round 3 -- roreg_ransac_score / roreg_refine /
 * roreg_ransac_batch take `w_f32`, the scores' storage type; roreg_group_conv_split / _f16x2 take an LDS slot order; roreg_ft_nonlin /
 * roreg_irrep_gemm_f16x2 take the plane-layout flags; 4: round 4 -- additions only (roreg_nn_search_ex / roreg_knn_search_ex / roreg_pdist and the entries marked "v4"),
 * bumped so that a binding can rely on them; 5: round 5 -- additions only, the entries marked "v5": roreg_sinkhorn_batch3 (+ its workspace size),
 * roreg_linear_path, roreg_linear_cat3, roreg_gemm_persistent, roreg_ft_nonlin_packed, roreg_group_conv_f16x2_packed; roreg_sinkhorn_batch2's `recompute` also takes 2); 6: round 6 -- additions only, the entries marked "v6" -- and, still under 6, the entries marked "v6b" and "v6c"
 * (additions only: no argument list and no struct changed; v6h = the pose-graph optimiser roreg_pg_workspace, roreg_pg_optimize_batch; v6g = the dense pair evaluation roreg_icp_eval_workspace, roreg_icp_eval_batch; v6f = the thin-layer switch roreg_gemm_thin; v6e = the voxel-grid entries roreg_voxel_workspace, roreg_voxel_downsample; v6c = the dense ICP entries roreg_icp_grid_size, roreg_icp_grid_build, roreg_icp_batch_workspace, roreg_icp_batch; v6d = the point-to-plane entries roreg_icp_normals,
 * roreg_icp_plane_batch_workspace, roreg_icp_plane_batch; v6i = the plane-to-plane entries roreg_icp_gicp_batch_workspace, roreg_icp_gicp_batch; v6j = the sparse-convolution entries roreg_sparse_*; v6m = the spatial-compatibility entries roreg_sc2_workspace, roreg_sc2_hypotheses_batch; v6n = the FPFH entries roreg_fpfh_*; v6o = the FPFH matcher's entries roreg_fpfh_match_workspace, roreg_fpfh_match_batch; v6q = the grid k-nearest-neighbour entry roreg_grid_knn).  A binding must compare roreg_abi_version() with the ROREG_ABI_VERSION it was written against and
 * refuse to call a library that answers differently (roreg_amd/hip.py:lib() does). */
#define ROREG_ABI_VERSION 6
int roreg_abi_version(void);
const char *roreg_last_error(void);

/* Upload the icosahedral tables: P[a*60+g] = index(R_g R_a) ("60_60.npy"), Nei[g*13+k]
 * ("Nei_Index_in_SO3_ordered_13.npy"), R[60*9] float64 ("Rotation.npy").  Host pointers.
 * Replaces the per-module np.load(...).cuda() at network/group_feat.py:12-14, rot_detect.py:39-40,
 * eqv_trans.py:83-86, rot_coh_match.py:127, test/estimator.py:78,374-375. */
int roreg_set_group_tables(const int32_t *P_host, const int32_t *Nei_host, const double *R_host);

/* ---- icosahedral group convolution (the MFMA kernel) --------------------------------------------
 * out[b,o,j] = bias[o] + sum_c sum_k W[o,c,k] * act(x)[b,c,gather[j*KS+k]]  (+ residual[b,o,j])
 *   act(x) = relu(x*bn_scale[c] + bn_shift[c]) when bn_scale != NULL, else x.
 * x is [B,Cin,Lin], out/residual are [B,Cout,Lout]; gather is int32 [Lout*KS] with values in [0,Lin).
 * For the full conv Lin=Lout=60, KS=13, gather=Nei.  Pruned layers (ET: only the group columns that can
 * reach g=0 are live) use Lout<60 and a composed gather; KS=1 gives the 1x1 convs of the ET head.
 * wpack is the weight tensor re-laid out by roreg_group_conv_pack_weights().
 * Replaces: data_process gather + BatchNorm2d(eval)+ReLU+Conv2d(C,O,(1,13)) at network/group_feat.py:16-33,
 * network/ops.py:11-64, network/eqv_trans.py:88-117,130-136, network/rot_detect.py:41,46. */
size_t roreg_group_conv_packed_size(int Cin, int Cout, int KS);            /* in floats */
int roreg_group_conv_pack_weights(const float *W_host /* [Cout,Cin,KS] */, int Cin, int Cout, int KS,
                                  float *wpack_host /* roreg_group_conv_packed_size floats */);
/* Small problems (few output tiles, long reduction) are split along the channel axis; the partial sums
 * go through a caller-owned workspace and are reduced in a fixed order (deterministic).  Size in floats,
 * 0 when the launch needs none. */
size_t roreg_group_conv_workspace_size(int B, int Cin, int Cout, int Lin, int Lout, int KS);
int roreg_group_conv(const float *x, const float *wpack, const float *bias,
                     const float *bn_scale, const float *bn_shift, const float *residual,
                     float *out, const int32_t *gather,
                     int B, int Cin, int Cout, int Lin, int Lout, int KS,
                     float *workspace, size_t workspace_floats, void *stream);

/* The same convolution with f32 accuracy on the bf16 matrix cores: operands as three bf16 pieces, six cross products, f32 accumulate
 * (2.67x fewer matrix-core cycles than the f32-input MFMA; measured error = the f32 kernel's).  KS = 13, Cin % 16 == 0,
 * Cout % 256 == 0, no residual.  wsplit: bf16 bits, layout [3 planes][KS][Cin/16][2 k-octets][Cout][8 channels]
 * (plane p of W[o, 16*(c/16) + 8*h + e, k]; the pieces are round-to-nearest-even of the exact remainders). */
int roreg_group_conv_split(const float *x, const void *wsplit, const float *bias, const float *bn_scale, const float *bn_shift,
                           float *out, const int32_t *gather,
                           const int32_t *lds_order /* nullable device int32 [Lin]: LDS slot of every input column (distinct values in [0, lds_stride); < 0 for a
                           column no output gathers) -- an execution hint that spreads the gathered operand reads over the LDS banks
                           (tools/lds_perm_search.py); results do not depend on it */, int lds_stride,
                           int B, int Cin, int Cout, int Lin, int Lout, int KS, void *stream);

/* Dense layer on row-major activations with the same f32-accurate 3 x bf16 split:
 *   out[b][o] = bias[o] + sum_k W[o][k] * act_k(x[b][k]) (+ residual[b][o]),  act_k(v) = max(v*scale[k] + shift[k], 0) or identity (scale NULL).
 * x [B][K] f32 (K % 16 == 0), out [B][O]; residual element (b, o) is read at residual[(b*O + o) * residual_stride] (1 = a dense [B][O]
 * tensor; 48 = column 0 of a [B][O][48] group-domain tensor: the ET trunk's identity short cut without a gathering copy).  wsplit: bf16 bits [3 planes][K/16][2 k-octets][round_up(O,256)][8] (zero rows beyond O).
 * Used for the ET trunk's last layer (K = 512*13: the 13-column stencil of the single live output column, gather folded into the weight
 * order; network/eqv_trans.py:101-117, network/ops.py:58-62) and the 1x1 head (network/eqv_trans.py:91-99,130-136). */
int roreg_dense_split(const float *x, const void *wsplit, const float *bias, const float *scale, const float *shift,
                      const float *residual, int residual_stride, float *out, int B, int K, int O, void *stream);

/* fp16 x 2 variants of the two entries above (half the matrix-core work; operands as hi + lo fp16 under a power-of-two block scale, see
 * roreg_irrep_gemm_f16x2).  The block is ONE ROW (keypoint / correspondence) b of x: its scale is derived on the device from the bound
 * |act(x[b])| <= act_smax * in_rowmax_dev[b] + act_tmax (act_smax = max |scale| or 1, act_tmax = max |shift| or 0; in_rowmax_dev [B] =
 * max |x[b]| maintained by the producing kernel), so a row's result never depends on which other rows share the launch (the reference's
 * batch-size independence, test/extractor.py:51-58, test/estimator.py:338-352).  The weights were scaled by 2^w_exp when split (layouts as
 * above with two planes hi, lo of fp16 bits).  out_rowmax_dev (nullable, [B], zeroed by the caller) receives max |out[b]| for the next layer. */
int roreg_group_conv_f16x2(const float *x, const void *wsplit2, int w_exp, const float *bias, const float *bn_scale, const float *bn_shift,
                           float act_smax, float act_tmax, const float *in_rowmax_dev, float *out, float *out_rowmax_dev,
                           const int32_t *gather, const int32_t *lds_order /* as roreg_group_conv_split */, int lds_stride,
                           int B, int Cin, int Cout, int Lin, int Lout, int KS, void *stream);
int roreg_dense_f16x2(const float *x, const void *wsplit2, int w_exp, const float *bias, const float *scale, const float *shift,
                      float act_smax, float act_tmax, const float *in_rowmax_dev, const float *residual, int residual_stride, float *out,
                      float *out_rowmax_dev, int B, int K, int O, void *stream);
/* v5: the ET trunk's 256 -> 512 convolution (network/eqv_trans.py:101-117, network/ops.py:46-57) fed by roreg_ft_nonlin_packed: x_words [B,Cin,Lin] holds
 * fp16 hi | fp16 lo << 16 of ReLU(BN(x[b])) * 2^e_b with e_b derived from in_bound_dev[b] (the bound the producer scaled with) -- BatchNorm, ReLU and
 * the operand split happened in the producer, the kernel's staging only regroups the halves.  Same outputs as roreg_group_conv_f16x2 up to the
 * block scale (a propagated bound instead of the tracked row maximum: measured 4.6-5.3 of the 22 bits). */
int roreg_group_conv_f16x2_packed(const uint32_t *x_words, const void *wsplit2, int w_exp, const float *bias, const float *in_bound_dev,
                                  float *out, float *out_rowmax_dev, const int32_t *gather, const int32_t *lds_order, int lds_stride,
                                  int B, int Cin, int Cout, int Lin, int Lout, int KS, void *stream);

/* eqv_raw [B,32,60] -> eqv = eqv_raw / max(||.||_2 over 32 ch, 1e-4) per (b,g);
 * inv = mean_g(eqv_raw) / max(||.||, 1e-4)  (inv may be NULL).  network/group_feat.py:38-43. */
int roreg_gf_finalize(const float *eqv_raw, void *eqv, int eqv_bf16 /* store eqv as bfloat16 (round to nearest even) instead of float32 */,
                      float *inv, int B, void *stream);

/* ---- detector ------------------------------------------------------------------------------------
 * enc [B,16,60] -> scores[b] = std_a( sum_f sum_g fn[f,P[a,g]] fn[f,g] ), fn = enc/||enc||_2 over 16 ch,
 * unbiased std over the 60 a's.  network/rot_detect.py:47-52. */
int roreg_det_score(const float *enc, float *scores, int B, void *stream);

/* ---- descriptors / nearest neighbours ------------------------------------------------------------
 * eqv [N,32,60] -> inv [N,32] = mean_g / (||.||_2 + 1e-5).  test/matcher.py:69-72. */
int roreg_inv_descriptor(const void *eqv, int eqv_bf16 /* eqv is stored as bfloat16; float32 arithmetic on the stored values */, float *inv, int N,
                         void *stream);

/* For every source row the nearest target row: d = sqrt(sum_f (s_f-t_f)^2 + 1e-7) accumulated in f order
 * (fp32, no FMA), first minimum wins.  src [m,F], tgt [n,F] row-major; optional row index lists
 * (src_rows/tgt_rows, int64, NULL = identity) select sampled keypoints without a gather copy.
 * idx_out int64 [m] (position within the target list), dist_out f32 [m] (may be NULL); scratch is m
 * uint64 of caller-owned workspace (packed (distance,index) keys merged across target slices by atomicMin).
 * Replaces knn_module.KNN(1).__call__ -> find_nn_gpu  (utils/knn_search.py:17-66,138-156). */
int roreg_nn_search(const float *src, const int64_t *src_rows, int m,
                    const float *tgt, const int64_t *tgt_rows, int n, int F,
                    int64_t *idx_out, float *dist_out, uint64_t *scratch, void *stream);

/* v4: roreg_nn_search with the distance type of modified_knn_matcher.find_nn_gpu (utils/knn_search.py:26-66): squared = 0 is 'L2' (the
 * function above), squared = 1 is 'SquareL2' = sum_f (s_f-t_f)^2 itself (no 1e-7, no root; find_nn_gpu's own default): the first minimum of
 * THAT value wins, which may differ from the 'L2' winner where two roots round to the same float. */
int roreg_nn_search_ex(const float *src, const int64_t *src_rows, int m,
                       const float *tgt, const int64_t *tgt_rows, int n, int F, int squared,
                       int64_t *idx_out, float *dist_out, uint64_t *scratch, void *stream);

/* v4: the whole distance matrix out[i*n+j] of modified_knn_matcher.pdist (utils/knn_search.py:17-24), A [m,F], B [n,F], any F >= 1;
 * squared as above. */
int roreg_pdist(const float *A, int m, const float *B, int n, int F, int squared, float *out, void *stream);

/* The mutual matcher for a batch of pairs (test/matcher.py:90-107 for every pair of a scene), on the matrix cores and bit-exact:
 * approximate squared distances |s|^2+|t|^2-2s.t as 3 x bf16 split MFMAs give row / column minima; every entry within a proven margin
 * of its row (column) minimum is re-evaluated with the literal formula of roreg_nn_search and merged "first minimum wins"
 * (csrc/mfma_match.hip).  Task p: sampled descriptors desc0[rows0[i]] (m0 rows) and desc1[rows1[j]] (m1 rows), F = 32, rows NULL =
 * identity; the mutual pairs (rows0 value, rows1 value) are written in increasing i to match_out + p*pitch*2 (pitch = max_m rounded up
 * to even), their number to counts_out[p].  tasks_dev is a DEVICE array; max_m >= every m0, m1.
 * workspace: roreg_mutual_match_batch_workspace(n_tasks, max_m) bytes. */
typedef struct {
    const float *desc0, *desc1;
    const int64_t *rows0, *rows1;
    int32_t m0, m1;
} roreg_match_task;
size_t roreg_mutual_match_batch_workspace(int n_tasks, int max_m);
int roreg_mutual_match_batch(const roreg_match_task *tasks_dev, int n_tasks, int max_m, int64_t *match_out, int32_t *counts_out,
                             void *workspace, size_t workspace_bytes, void *stream);

/* k nearest (k<=8) targets per source in increasing distance, first index on ties; idx_out int64 [m,k].
 * Replaces KNN(k>=2) -> find_knn_gpu (utils/knn_search.py:68-103), used by NMS_sample with F=3, k=5
 * (test/matcher.py:21-23). */
size_t roreg_knn_search_workspace(int m, int n);
int roreg_knn_search(const float *src, int m, const float *tgt, int n, int F, int k,
                     int64_t *idx_out, void *workspace /* roreg_knn_search_workspace bytes: targets are scanned in slices that fill the chip;
                     NULL = one thread per source scans everything */, size_t workspace_bytes, void *stream);

/* v4: roreg_knn_search with the distance type (squared as in roreg_nn_search_ex) and, optionally, the k distances (dist_out f32 [m,k] or
 * NULL): modified_knn_matcher.find_knn_gpu (utils/knn_search.py:68-103). */
int roreg_knn_search_ex(const float *src, int m, const float *tgt, int n, int F, int k, int squared, int64_t *idx_out, float *dist_out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* roreg_knn_search for several clouds per launch: the point lists are stacked, seg_src / seg_tgt are DEVICE int32 [n_seg+1] row
 * offsets, a source only sees the targets of its own segment; idx_out int64 [m_total,k] holds indices LOCAL to the segment (the NMS
 * sampling of every cloud of a scene in two launches, test/matcher.py:21-23). */
size_t roreg_knn_search_seg_workspace(long long m_total, int n_seg, int max_m, int max_n);
int roreg_knn_search_seg(const float *src, const float *tgt, const int32_t *seg_src, const int32_t *seg_tgt, int n_seg, long long m_total,
                         int max_m, int max_n, int F, int k, int64_t *idx_out, void *workspace, size_t workspace_bytes, void *stream);

/* Mutual check + ordered compaction: for i in 0..m-1 (increasing) keep (i, nn01[i]) iff nn10[nn01[i]]==i;
 * pairs are mapped through sample0/sample1 (int64, NULL = identity) and written to match_out int64 [*,2];
 * *count_out (device int32) receives the number kept.  test/matcher.py:98-107. */
int roreg_mutual_matches(const int64_t *nn01, const int64_t *nn10, int m, int n /* entries of nn10 */,
                         const int64_t *sample0, const int64_t *sample1,
                         int64_t *match_out, int32_t *count_out, void *stream);

/* ---- estimator -----------------------------------------------------------------------------------
 * Per correspondence b: cor[a] = sum_f ( sum_g d1[f,P[a,g]] d2[f,g] ), argmax_a (first max).
 * d1 = feats1[rows1[b]], d2 = feats0[rows0[b]] with feats* f32 [N,32,60]; rows* int64 (NULL = b itself).
 * idx_out int64 [M]; cor_out f32 [M,60] optional.
 * Replaces extractor_dr_index.Batch_Des2R_torch (test/estimator.py:85-89) and the gathers at :108-110. */
int roreg_des2r(const float *feats1, const int64_t *rows1, const float *feats0, const int64_t *rows0,
                int M, int64_t *idx_out, float *cor_out, void *stream);

/* Generalised 60x60 group cross-correlation: cor[b,a] = sum_f sum_g A[f, T[a,g]] * B[f,g] with A = perm_feats[perm_rows[b]],
 * B = bcast_feats[bcast_rows[b]] and T = P (transpose_table=0) or P^T (transpose_table=1: T[a,g] = P[g,a]).
 * idx_out (first argmax) and cor_out (all 60 values) are each optional.  roreg_des2r is the transpose_table=0 case; the
 * matcher's R_indicator (network/rot_coh_match.py:154-163) is the transpose_table=1 case in both orientations. */
int roreg_group_corr(const float *perm_feats, const int64_t *perm_rows, const float *bcast_feats, const int64_t *bcast_rows,
                     int M, int transpose_table, int64_t *idx_out, float *cor_out, void *stream);

/* v4: all 60 correlations of roreg_group_corr as ONE [60 x 32] . [32 x 60] float32 matrix product per point on the matrix cores (C[p,g] = sum_f
 * A[f,p] B[f,g]) + the 60 coset sums cor[a] = sum_g C[T[a,g], g]: the permutation addresses the result instead of every multiply-add
 * (csrc/corr_mfma.hip; HBM-bound instead of LDS-bound).  The literal kernel's function in another summation order (float32 throughout,
 * ~1e-6 |A||B| apart): for the correlation as a FEATURE (the stacked matcher's R_indicator); no arg-max. */
int roreg_group_corr_mfma(const float *perm_feats, const int64_t *perm_rows, const float *bcast_feats, const int64_t *bcast_rows, int M,
                          int transpose_table, float *cor_out, void *stream);

/* The same arg-max (test/estimator.py:85-89, bit for bit) with 10x fewer operations: the 60 correlations are first BOUNDED in the irrep
 * domain of the icosahedral group -- cor[a] = sum_rho sum_ij rho(a)[j][i] (sum_f X2_f(rho) X1_f(rho)^T)[i][j], sum_d d^3 = 244
 * multiply-adds per channel instead of 3600, from per-keypoint coefficients computed once per cloud (roreg_feat_coefs) -- and only the
 * candidates within a rigorous margin of the bound's maximum (near ties, duplicates) are re-evaluated with the literal formula in the
 * reference's evaluation order from the group-domain rows; the first maximum of those is returned.
 * coef1 / coef0 = roreg_feat_coefs(feats1 / feats0) [*,32,60] f32; feats* are float32 or (feat_bf16) bfloat16 [*,32,60].
 * roreg_set_des2r_tables uploads the index / representation tables (roreg_amd/fourier.py derives them from the multiplication table and
 * checks the identity to 1e-12): ia, ib uint8 [60][5] (coefficient indices of the k-th product term of entry q = (rho,i,j)), cnt uint8 [60]
 * (terms = d), NT float32 [60 (q)][60 (a)] = rho(a)[j][i].  roreg_des2r_recheck_count: how many correspondences took the exact path. */
int roreg_set_des2r_tables(int transpose_table /* 0: x[P[a,.]] (Des2R); 1: x[P[.,a]] (R_indicator) */, const uint8_t *ia_host,
                           const uint8_t *ib_host, const uint8_t *cnt_host, const float *NT_host);
/* All 60 correlations of roreg_group_corr from the coefficient rows alone (no arg-max, no re-check): cor_out [M,60] f32, equal to the
 * literal float32 evaluation to its rounding level (~1e-6 |d1||d2|).  For the matcher's R_indicator feature (network/rot_coh_match.py:154-163). */
int roreg_group_corr_irrep(const float *perm_coefs, const int64_t *perm_rows, const float *bcast_coefs, const int64_t *bcast_rows, int M,
                           int transpose_table, float *cor_out, void *stream);
int roreg_des2r_irrep(const float *coef1, const int64_t *rows1, const float *coef0, const int64_t *rows0, const void *feats1,
                      const void *feats0, int feat_bf16, int M, int64_t *idx_out, void *stream);
int roreg_des2r_recheck_count(int reset, int32_t *count_out);
/* out[b,c,q] (f32 [B,C,60]) = sum_g F[q][g] x[b,c,g]: the orthonormal group-Fourier coefficients of a group-domain tensor x [B,C,60]
 * (float32, or bfloat16 with x_bf16) in per-keypoint layout -- the operand of roreg_des2r_irrep.  split as roreg_ft_nonlin. */
int roreg_feat_coefs(const void *x, int x_bf16, float *out, int B, int C, int split, void *stream);

/* Build the ET network input x [M,128,60] = cat(before1[r1][:, :, P[a]], before0[r0], after1[r1][:, :, P[a]],
 * after0[r0]) for correspondence rows (r0,r1) and anchor a=pre_idx[b].
 * Replaces batch_create + the per-row permutation loop (test/estimator.py:293-306; network/eqv_trans.py:126-129). */
int roreg_et_gather(const void *before0, const void *before1, const void *after0, const void *after1,
                    int feat_bf16 /* the four feature tensors are bfloat16 instead of float32 (BASELINE config 5) */,
                    const int64_t *rows0, const int64_t *rows1, const int64_t *pre_idx, int M,
                    float *x_out, void *stream);

/* q [M,4] f32 (un-normalised head output) -> q/||q||; R = R(q) (fp32 arithmetic as utils/r_eval.py:90-106
 * on float32 inputs) promoted to f64, times Rgroup[a] (the float32-rounded table, as test/estimator.py:279);
 * t = key0 - key1 R^T (f64).  Trans_out f64 [M,3,4]; quat_out f32 [M,4] optional (normalised).
 * Replaces eqv_trans.py:137 and test/estimator.py:350-366. */
int roreg_quat_to_trans(const float *q, const int64_t *anchor, const double *keys0, const int64_t *rows0,
                        const double *keys1, const int64_t *rows1, int M,
                        double *Trans_out, float *quat_out, void *stream);

/* One-shot RANSAC scoring (fp64, no FMA).  For hypothesis h (3x4 row-major in Trans[hyp_rows[h]], hyp_rows
 * int64, NULL = identity): overlap[h] = sum_{i: ||k0_i - (R k1_i + t)||^2 < ird^2} w_i / M, accumulated in
 * increasing i.  k0,k1 f64 [M,3] (already gathered by match), w f64 [M].  best_out (device int32[1]) gets
 * the first h with the strictly greatest overlap (estimator.py:430-436; -1 if every overlap is 0);
 * mask_out (uint8 [H,M], optional) the inlier masks.
 * w_f32 != 0: the scores are the rotation-coherence matcher's float32 array (test/matcher.py:210; every w_i is a float32 value): the
 * reference's np.sum(scores[inliers]) is then numpy's PAIRWISE float32 reduction over the compacted inlier array and its quotient by M a
 * float32 division (test/estimator.py:381), which the kernel rebuilds bit for bit, so that hypotheses whose overlaps tie only after
 * float32 rounding keep the reference's order under the strict `>` of :433; overlap_out holds those float32 values widened.
 * Replaces yohoo_ransac.overlap_cal and the hypothesis loop (test/estimator.py:377-382,426-436). */
int roreg_ransac_score(const double *k0, const double *k1, const double *w, int w_f32, int M,
                       const double *Trans, const int64_t *hyp_rows, int H, double ird,
                       double *overlap_out, int32_t *best_out, uint8_t *mask_out, void *stream);

/* Refinement step: inliers of T_in (3x4 taken from T_in, or from Trans[hyp_rows[*best]] when best!=NULL)
 * at threshold `dist`; weights w/sum(w); weighted centroids; H = (k0-c0)^T diag(w) (k1-c1); R = U V^T of
 * the 3x3 SVD (no reflection guard); t = c0 - c1 R^T.  T_out f64 [4,4].  The SVD runs on the device
 * (one-sided Jacobi); when H is rank-deficient (<= 2 inliers, collinear inliers) U V^T is not unique and the
 * reference's value is whatever LAPACK's null-space basis gives, so stats_out exposes H, the centroids and
 * the weight sum for a host LAPACK evaluation of exactly that case.  w_f32 != 0 (float32 scores, as in roreg_ransac_score): the
 * normalisation scores / np.sum(scores) runs in float32 like the reference's (:50), pairwise sum and per-weight float32 quotient.
 * Replaces refiner.Refine_trans (test/estimator.py:28-72). */
int roreg_refine(const double *k0, const double *k1, const double *w, int w_f32, int M,
                 const double *T_in, int t_in_stride /* 4 for 3x4/4x4 rows */,
                 const double *Trans, const int64_t *hyp_rows, const int32_t *best,
                 double dist, double *T_out, double *stats_out /* optional f64[16]: H(9), c0(3), c1(3), sum w */,
                 void *stream);

/* The local-transform stage (Des2R + ET input assembly, then quaternion -> 3x4 transform) of every pair of a scene in 2 + 1 launches
 * around the one batched ET trunk pass (test/estimator.py:85-111,293-366 per pair; same arithmetic as roreg_des2r / roreg_et_gather /
 * roreg_quat_to_trans, bit-identical).  Task p evaluates its n correspondences matches[sel[i]] (sel NULL = the first n rows); output
 * rows [off, off+n): dr_out int64, x_out [*,128,60] f32 (ET input; NULL = Des2R only, the YOHO-C estimator's DR_index),
 * Trans_out [*,3,4] f64.  tasks_dev is a DEVICE array. */
typedef struct {
    const void *before0, *before1, *after0, *after1;   /* the clouds' group features [*,32,60]: float32, or bfloat16 with flags bit 1 */
    const double *keys0, *keys1;
    const int64_t *matches;
    const int64_t *sel;
    int32_t n, pad_;
    int64_t off;
    const float *coef0, *coef1;                        /* roreg_feat_coefs(after0 / after1) [*,32,60] f32, needed with flags bit 0 */
} roreg_lt_task;
/* flags: bit 0 = Des2R through the irrep-domain bound + exact re-check (roreg_des2r_irrep; tasks carry coef0 / coef1), else the literal
 * kernel; bit 1 = the features are bfloat16 (needs bit 0). */
int roreg_lt_prepare_batch(const roreg_lt_task *tasks_dev, int n_tasks, int max_n, int flags, int64_t *dr_out, float *x_out,
                           const float *bn_scale /* [128] */, const float *bn_shift, float *x_bound_out /* nullable, with x_out: per output row
                           sqrt(60) max |ReLU(bn_scale_c x + bn_shift_c)| = roreg_row_bound(x_out, bn) computed while assembling (the block scale of the
                           fp16 x 2 Conv_init GEMM, network/eqv_trans.py:88) */, void *stream);
int roreg_lt_finish_batch(const roreg_lt_task *tasks_dev, int n_tasks, int max_n, const float *q_all, const int64_t *dr_all,
                          double *Trans_out, void *stream);
/* v6b: the ET input without its copy.  roreg_role_max: per keypoint of a cloud the four maxima over (c, g) of ReLU(fma(v, bn_scale[k*32 + c], bn_shift[k*32 + c])),
 * k = 0: `before` as the permuted side (cloud 1 of a pair), 1: `before` as cloud 0, 2: `after` as cloud 1, 3: `after` as cloud 0 -> out [N,4] f32 (bn = the
 * [128] BatchNorm constants of Conv_init).  A maximum over a channel's 60 group elements does not depend on the permutation, so
 * roreg_lt_prepare_rows forms from them the very float roreg_lt_prepare_batch's x_bound_out holds: it runs Des2R like roreg_lt_prepare_batch and
 * writes dr_out, rows_out [total][4] (the addresses of each output row's four source blocks, ET channel order) and x_bound_out [total], and no x.
 * roles_dev: DEVICE array [n_tasks][2] of the tasks' role tables (cloud 0's, cloud 1's; [*,4] f32 each); roreg_lt_task is unchanged. */
int roreg_role_max(const void *before, const void *after, int feat_bf16, const float *bn_scale /* [128] */, const float *bn_shift, float *out,
                   int N, void *stream);
/* v6b: the same maxima from kernels that read the tensors anyway.  roreg_row_bound_roles = roreg_row_bound(x, no BatchNorm, C = 32) on a cloud's `before`
 * features + columns 0 and 1 of role_out [B,4] (role_scale / role_shift: the 64 entries of channels 0..63); roreg_inv_descriptor_roles = roreg_inv_descriptor
 * + columns 2 and 3 (the 64 entries of channels 64..127). */
int roreg_row_bound_roles(const void *x_spatial, int x_bf16, float *bound_out, const float *role_scale, const float *role_shift, float *role_out, int B,
                          void *stream);
int roreg_inv_descriptor_roles(const void *eqv, int eqv_bf16, float *inv, const float *role_scale, const float *role_shift, float *role_out, int N,
                               void *stream);
int roreg_lt_prepare_rows(const roreg_lt_task *tasks_dev, const float *const *roles_dev, int n_tasks, int max_n, int flags, int64_t *dr_out,
                          uint64_t *rows_out, float *x_bound_out, void *stream);

/* The estimator tail of every pair of a scene in five launches: gather the matched keypoints, score the <= max_iter hypotheses
 * (one wavefront each), first strictly-greatest overlap, refine at 2*ird from the winning local transform, refine at ird from that
 * (test/estimator.py:405-443 per pair; same arithmetic order as roreg_ransac_score / roreg_refine, so results are bit-identical).
 * tasks_dev: DEVICE array; koff = prefix sum of M over the tasks; total_M = sum of M; max_M / max_H >= every M / H.
 * Outputs per task: best_out[p] (hypothesis index or -1), T1/T2 [p][16] row-major 4x4, stats1/stats2 [p][16] as roreg_refine. */
typedef struct {
    const double *keys0, *keys1;   /* keypoints of the two clouds [*,3] f64 */
    const int64_t *matches;        /* [M,2] interleaved rows (cloud 0, cloud 1) */
    const double *w;               /* [M] match scores, NULL = ones (test/matcher.py:109) */
    const double *Trans;           /* [*,3,4] f64 local transforms */
    const int64_t *hyp_rows;       /* [H] rows of Trans in hypothesis order, NULL = identity */
    int32_t M, H;
    int64_t koff;
} roreg_ransac_task;
size_t roreg_ransac_batch_workspace(int n_tasks, long long total_M, int max_H);
int roreg_ransac_batch(const roreg_ransac_task *tasks_dev, int n_tasks, long long total_M, int max_M, int max_H, double ird,
                       int w_f32 /* the tasks' scores are float32 values: numpy's float32 reductions, see roreg_ransac_score */,
                       int32_t *best_out, double *T1_out, double *stats1_out, double *T2_out, double *stats2_out,
                       void *workspace, size_t workspace_bytes, void *stream);

/* v4: one more refinement at `dist`, from the given transforms T_in [n_sel][16], of the tasks sel_dev[0..n_sel) (device int32) of an EARLIER
 * roreg_ransac_batch call: tasks_dev, total_M and workspace are that call's (its workspace still holds the gathered keypoints).  T_out /
 * stats_out [n_sel][16] as roreg_refine.  One launch for all of them: the engine's second refinement of the pairs whose first one had a
 * rank-deficient covariance and was closed by host LAPACK (test/estimator.py:53-72 per pair). */
int roreg_refine_batch(const roreg_ransac_task *tasks_dev, const int32_t *sel_dev, int n_sel, long long total_M, const double *T_in,
                       double dist, int w_f32, double *T_out, double *stats_out, const void *workspace, void *stream);

/* Seeded shuffles, HOST function (no device work): for every job j, `np.random.seed(seeds[j])` followed by, for each of its per_job lists
 * (sizes int32 [n_jobs][per_job]), `idx = np.arange(n); np.random.shuffle(idx); idx[:take]` -- numpy's legacy MT19937 stream and its
 * Fisher-Yates shuffle, replayed bit for bit.  out int64 [n_jobs][per_job][take] (-1 beyond a list's length).  Replaces the per-pair
 * Python loops of the matcher's keypoint sampling (test/matcher.py:83-88: two lists per pair, take = keynum) and of the one-shot
 * estimator's hypothesis order (test/estimator.py:423-425: one list per pair, take = max_iter) when every pair has a generator stream of
 * its own; jobs are spread over n_threads host threads. */
int roreg_mt_shuffle_prefix(const uint32_t *seeds, int n_jobs, const int32_t *sizes, int per_job, int take, int64_t *out, int n_threads);

/* v6.  The same shuffles from ONE running stream, HOST function: the process-global generator an unseeded Test.py consumes (test/matcher.py:83-88,
 * test/estimator.py:423-425).  key[624] / *pos: np.random.get_state()'s MT19937 key and position on entry, the stream's state after the last
 * list on return (for np.random.set_state); `for n in sizes: idx = np.arange(n); np.random.shuffle(idx); idx[:take]`, list after list on one
 * thread.  out int64 [n_lists][take] (-1 beyond a list's length). */
int roreg_mt_stream_shuffle_prefix(uint32_t *key, int32_t *pos, const int32_t *sizes, int n_lists, int take, int64_t *out);

/* YOHO-C hypothesis draws, HOST function (no device work): replays the generator calls of the reference's sampling loop
 * (test/estimator.py:220-230: np.random.choice(range(60), p=prob), then np.random.choice(bin_members, 3)) over a block of raw MT19937
 * words drawn by the caller from the global generator.  cdf f64 [60] = prob.cumsum()/prob.sum(); bin_size int32 [60] = members per
 * rotation bin; at most max_iter hypotheses and max_tries + 1 tries.  bin_out int32 [max_iter], pick_out int64 [max_iter,3] (positions
 * inside the bin's member list).  Returns 3 when the block is too short (retry with more words); *words_used = words consumed. */
int roreg_yohoc_draw(const uint32_t *words, long long n_words, const double *cdf, const int32_t *bin_size, int max_iter, int max_tries,
                     int32_t *bin_out, int64_t *pick_out, int32_t *n_hyp_out, long long *words_used);

/* v4: row gathers of several (source, row list) pairs in ONE launch -- task t copies rows[0..n) of src (row_bytes each, a multiple of 8) to
 * consecutive rows of dst; tasks_dev is a DEVICE array, max_n >= every n.  The stacked matcher's per-pair sample gathers
 * (feats[sample], keys[sample]: test/matcher.py:187-197 for every pair of a group). */
typedef struct {
    const void *src;
    const int64_t *rows;
    void *dst;
    int32_t n, pad_;
} roreg_gather_task;
int roreg_gather_rows_batch(const roreg_gather_task *tasks_dev, int n_tasks, int max_n, int row_bytes, void *stream);

/* Gather rows: out[i] = src[rows[i]] for f64 [.,3] keypoints (estimator.py:407-408). */
int roreg_gather_rows_f64(const double *src, const int64_t *rows, int M, int width, double *out, void *stream);

/* ---- rotation-coherence matcher (Match_ot, network/rot_coh_match.py) ---------------------------------
 * Per-point tensors are position-major: [points, channels] or [points, k, channels] float32.
 *
 * roreg_topk_dot: for every row of A [m,32] the k (16, 8 or 1) rows of B [n,32] with the largest dot product, descending,
 * lower index first on ties; replaces score_mat + the full descending argsort of Knn_index_extract
 * (rot_coh_match.py:8-12,34-45) without materialising the m x n matrix.  ws: roreg_topk_dot_workspace_size floats.
 *
 * Several pairs per launch ("segments"): the per-point tensors of the pairs are concatenated, seg* are DEVICE int32 [n_seg+1] row
 * offsets (in points), and every per-pair quantity (neighbour search, InstanceNorm statistics, column maxima, Sinkhorn) stays inside
 * its pair with the arithmetic of the one-pair call, bit for bit.  In roreg_topk_dot a row of A's segment p searches B's segment p and
 * idx_out holds GLOBAL rows of B; max_m / max_n = the largest segment.  seg pointers NULL = one pair (the remaining segment arguments
 * are ignored). */
size_t roreg_topk_dot_workspace_size(int m, int n, int k);
int roreg_topk_dot(const float *A, int m, const float *B, int n, int k, int64_t *idx_out, float *val_out /* optional [m,k] */,
                   float *ws, size_t ws_floats, const int32_t *segA, const int32_t *segB, int n_seg, int max_m, int max_n, void *stream);

/* y [L,Cout] = x [L,Cin] W^T + b  (the 1x1 Conv2d layers: attention projections / merge, first and residual convs of
 * mlp_2layer and Contextnorm; rot_coh_match.py:14-32,63-81,95-119): one float32 fmaf chain per (row, output), inputs ascending, starting from the bias.
 * v5: that chain runs on the matrix cores (v_mfma_f32_32x32x2_f32 is a float32 fmaf chain over k on gfx950, bit for bit: csrc/linear_chain.hip);
 * roreg_linear_path(1) selects the vector-pipe kernels instead (same bits; returns the previous setting, 0 = matrix cores).
 * v6: the matrix-core kernels are software-pipelined (lc2_kernel); roreg_linear_path(2) = the matrix cores through round 5's kernels (A/B, tests).
 * Every entry point that rests on the fma-chain property (roreg_linear / _cat3, roreg_mlp_tail, roreg_mlp_head, roreg_topk_dot's MFMA kernel, the
 * matrix-free read-out of roreg_sinkhorn_batch3) verifies it ONCE per process on the device (1024 outputs: cancelling pairs, zeros, subnormal
 * products) in front of its first launch and returns 4 with roreg_last_error() naming the vector-pipe switches if the hardware disagrees. */
int roreg_linear(const float *x, int L, int Cin, const float *W /* [Cout,Cin] */, const float *b, int Cout, float *y, void *stream);
int roreg_linear_path(int path);
/* v5: y [m * k, Cout] (Cout = 64 | 32) = W [pos[r] (32) | table[idx[r]] (32) | conf[r / k] (32)] + b -- roreg_linear on the value MLP's input
 * (rot_coh_match.py:95-119) without materialising its [m * k, 96] rows: the kernel's row staging reads the three sources.  The same chains on the same
 * values: bitwise roreg_linear on the concatenated rows.  Matrix-core path only (with roreg_linear_path(1) build the rows and call roreg_linear). */
int roreg_linear_cat3(const float *pos /* [m*k,32] */, const float *table /* [n,32] */, const int64_t *idx /* [m*k] rows of table */,
                      const float *conf /* [m,32] */, int m, int k, const float *W /* [Cout,96] */, const float *b, int Cout, float *y, void *stream);
/* v4: the same layer on the matrix cores for Cin >= 32 (other shapes: roreg_linear): fp16 hi + lo operands under exact per-row / per-tensor
 * power-of-two scales, all four cross products, f32 accumulate (<= 6e-7 of sum |w||x| per element: the level of the fmaf chain, other
 * rounding); one kernel for every L, a row's result depends on that row alone.  csrc/linear_mfma.hip; used by the stacked matcher. */
int roreg_linear_mfma(const float *x, int L, int Cin, const float *W /* [Cout,Cin] */, const float *b, int Cout, float *y, void *stream);

/* InstanceNorm2d(affine=False) statistics of h [L,C] over all L positions -> mean_rstd [2C] = mean, 1/sqrt(var_biased+eps).
 * ws: 2*C*256 doubles.  (rot_coh_match.py:19,68)   With segments (seg_off in points, `mult` rows of h per point): one statistic
 * per pair, mean_rstd [n_seg][2C], ws n_seg*2*C*256 doubles. */
int roreg_instnorm_stats(const float *h, int L, int C, float eps, float *mean_rstd, double *ws, const int32_t *seg_off, int n_seg,
                         int mult, void *stream);

/* y [L,32] += W2 relu((h - mean) * rstd) + b2  (closing conv of mlp_2layer / Contextnorm; y already holds the residual conv);
 * with segments every row uses the statistics of its pair. */
int roreg_mlp_tail(const float *h, int L, int Cmid, const float *mean_rstd, const float *W2 /* [32,Cmid] */, const float *b2,
                   float *y, const int32_t *seg_off, int n_seg, int mult, void *stream);
/* v4: roreg_mlp_tail on the matrix cores (as roreg_linear_mfma; the normalisation + ReLU are applied while the operand is split). */
int roreg_mlp_tail_mfma(const float *h, int L, int Cmid, const float *mean_rstd, const float *W2 /* [32,Cmid] */, const float *b2,
                   float *y, const int32_t *seg_off, int n_seg, int mult, void *stream);

/* ctx [L,120] = [R [L,60] | max over the points of the row's pair of R]  (Self_attention_block's ambiguity context,
 * rot_coh_match.py:201-202).  ws: n_seg*(256+1)*60 floats. */
int roreg_context_colmax(const float *R, int L, const int32_t *seg_off, int n_seg, int max_len, float *ctx_out, float *ws, void *stream);

/* Core of MultiHeadedAttention(4 heads, d_model 32) on k-NN neighbourhoods (rot_coh_match.py:84-119): qp [m,32] projected
 * queries; kp / vp projected keys / values, either dense [m,k,32] or a per-point table [n,32] addressed through idx [m,k].
 * x_out [m,32] (input of the merge conv).  Channel c belongs to head c%4, dim c/4 (the reference's .view(b,8,4,-1)). */
int roreg_knn_attention(const float *qp, const float *kp, const float *vp, const int64_t *idx, int k_is_table, int v_is_table,
                        int m, int k, float *x_out, void *stream);

/* Small data-movement / normalisation steps of the matcher graph (see csrc/rm.hip for the op list). */
int roreg_rm_elementwise(int op, const float *a, const float *b, const float *c, const int64_t *idx, int L, int k, int C,
                         float *out, float *ws, void *stream);

/* Log-domain Sinkhorn with dustbins + mutual-argmax read-out (rot_coh_match.py:285-314,363,369-379).  The coupling scores
 * <src_final[i], tgt_final[j]> ([m,32] x [n,32]) are formed on the fly; Z_out [(m+1),(n+1)]; matches0 [m], matches1 [n] (-1 = unmatched), mscores0/1 (exp of the row maximum for mutual matches).
 * ws: roreg_sinkhorn_workspace_size floats (the coupling matrix and its transpose stay resident across the 2*iters passes). */
size_t roreg_sinkhorn_workspace_size(int m, int n);
int roreg_sinkhorn(const float *src_final, int m, const float *tgt_final, int n, float alpha, int iters, float *Z_out,
                   int64_t *matches0, int64_t *matches1, float *mscores0, float *mscores1, float *ws, size_t ws_floats, void *stream);

/* The same for several pairs per launch (2*iters + 5 launches for all of them): descriptors concatenated by seg_src / seg_tgt (device
 * and host copies of the int32 offsets), read-outs concatenated the same way with indices LOCAL to the pair; the coupling matrix
 * itself is not returned.  Each iteration reads the matrix once (rows in the log domain, column sums by fma of the same exponentials);
 * read-outs equal the one-pair call's (indices identical on the tests, scores to rounding).  consts: DEVICE copy of the 4*n_seg floats of roreg_sinkhorn_batch_consts (a host function: the host
 * logf values the one-pair call uses). */
size_t roreg_sinkhorn_batch_workspace_size(int n_seg, int max_m, int max_n, long long total_m, long long total_n);
int roreg_sinkhorn_batch_consts(const int32_t *seg_src_host, const int32_t *seg_tgt_host, int n_seg, float *consts_host);
int roreg_sinkhorn_batch(const float *src_final, const float *tgt_final, const int32_t *seg_src, const int32_t *seg_tgt,
                         const int32_t *seg_src_host, const int32_t *seg_tgt_host, const float *consts, int n_seg, float alpha, int iters,
                         int64_t *matches0, int64_t *matches1, float *mscores0, float *mscores1, float *ws, size_t ws_floats,
                         void *stream);

/* v4: roreg_sinkhorn_batch with the choice of how the iterations see the coupling matrix.  recompute = 0: the function above (the matrix is
 * materialised and read once per iteration: 4 (m+1)(n+1) bytes per pair and iteration from HBM).  recompute = 1: the iterations never read
 * a matrix -- every pass recomputes the scores <s_i, t_j> on the matrix cores from the L2-resident descriptors (fp16 hi + lo operands, f32
 * accumulate; potentials, dustbins and padding ride in one more MFMA) and only exponentiates and adds (csrc/ot_flash.hip); same read-outs
 * (indices identical on the tests, scores to 1e-6).  The matrix is still built once per pair for the read-out.  A pair whose TARGET cloud
 * has at most 2559 points (yoho_mat's default keynum 2500, test/matcher.py:152) recomputes the scores ONCE per iteration (a 32-row strip's
 * exponentials stay in registers between the row and the column sums); a longer one (`Test.py --keynum 5000`, test/evaluator.py:20,46)
 * twice (rows, then columns) -- or, recompute = 2, once, with two cooperating workgroups per strip up to 5119 points.  The form is chosen
 * per pair, so a pair's result does not depend on what is stacked beside it.
 * ws: roreg_sinkhorn_batch2_workspace_size floats. */
size_t roreg_sinkhorn_batch2_workspace_size(int n_seg, int max_m, int max_n, long long total_m, long long total_n);
int roreg_sinkhorn_batch2(const float *src_final, const float *tgt_final, const int32_t *seg_src, const int32_t *seg_tgt,
                          const int32_t *seg_src_host, const int32_t *seg_tgt_host, const float *consts, int n_seg, float alpha, int iters,
                          int64_t *matches0, int64_t *matches1, float *mscores0, float *mscores1, float *ws, size_t ws_floats,
                          int recompute, void *stream);
/* v5: the same, and (Z_out non-null, n_seg == 1) the pair's log-coupling matrix Z [(m+1) x (n+1)] row-major = ((Z0 + u) + v) - norm, the
 * `scores` of Match_ot.forward (network/rot_coh_match.py:313,366) -- so that forward() and the stacked path run ONE set of Sinkhorn kernels.
 * With recompute != 0 and Z_out == NULL nothing materialises a matrix: the mutual arg-max read-out (rot_coh_match.py:369-379) is taken from float32
 * MFMA chains over the descriptors (bitwise the fmaf chains the matrix held) with the potentials added in the reference's association, and the
 * workspace (roreg_sinkhorn_batch3_workspace_size) shrinks from 2 (m+1)(n+1) floats per pair to ~4 (m+n). */
size_t roreg_sinkhorn_batch3_workspace_size(int n_seg, int max_m, int max_n, long long total_m, long long total_n, int recompute, int want_Z);
int roreg_sinkhorn_batch3(const float *src_final, const float *tgt_final, const int32_t *seg_src, const int32_t *seg_tgt,
                          const int32_t *seg_src_host, const int32_t *seg_tgt_host, const float *consts, int n_seg, float alpha, int iters,
                          int64_t *matches0, int64_t *matches1, float *mscores0, float *mscores1, float *ws, size_t ws_floats,
                          int recompute, float *Z_out, void *stream);
/* v6 (host function): write n files -- file q = headers[q] (header_len[q] bytes, e.g. a .npy header) followed by data[q] (nbytes[q] bytes) -- on
 * n_threads host threads: the device-resident engine's StageFileWriter leaves the reference's ~1800 small per-pair .npy files of a 449-pair scene
 * (test/matcher.py:108-109, test/estimator.py:111,367) through it instead of one np.save each.  Returns 0, or 1 + the index of the first failure. */
int roreg_write_files(const char *const *paths, const void *const *headers, const int32_t *header_len, const void *const *data,
                      const int64_t *nbytes, int n, int n_threads);
/* v6 (host function): the YOHO-C hypothesis draws (test/estimator.py:119-137, 214-230) of n_pairs pairs, pair p from its own generator stream
 * np.random.RandomState(seeds[p]): anchors = the pairs' coarse rotations (Des2R index of the correspondences hypotheses are drawn from),
 * concatenated, pair p at [offsets[p], offsets[p+1]).  rows_out [n_pairs][max_iter][3]: the three correspondences (positions in the pair's list)
 * of each hypothesis; n_hyp_out [n_pairs]: how many were drawn, or -1 when no rotation bin holds two correspondences -- the reference then
 * answers np.random.rand(4, 4) (giveup_out [n_pairs][16], recalltime 50000).  Same words of the same streams as the Python loop, on n_threads. */
int roreg_yohoc_draw_many(const uint32_t *seeds, int n_pairs, const int64_t *anchors, const int64_t *offsets, int max_iter, int max_tries,
                          int64_t *rows_out, int32_t *n_hyp_out, double *giveup_out, int n_threads);
/* v6: mlp_2layer / Contextnorm (network/rot_coh_match.py:14-32, 63-81): the first convolution (Cin -> C1, output h [L, C1]) and the residual
 * branch (Cin -> 32, output y [L, 32]) in ONE launch -- the float32 fmaf chains of roreg_linear on the matrix cores, bit for bit, the input tile
 * staged once, the next tile's rows in flight under the chains -- plus the per-pair InstanceNorm statistics of h (mean_rstd [n_seg][2 C1], the
 * operand of roreg_mlp_tail) from per-tile float64 channel sums added in a fixed per-pair order: roreg_instnorm_stats' numbers in another
 * association (float64 sums rounded to float32: the same floats but for an ulp once in ~1e8 values).  x [L, Cin], or x == NULL and
 * pos / table / idx / conf (m, k; L = m k; Cin = 96): the value MLP's rows as in roreg_linear_cat3.  Served: (Cin, C1) = (3, 64), (64, 64),
 * (96, 64), (120, 128) on the matrix-core path; returns 3 and launches nothing otherwise (call roreg_linear x 2 + roreg_instnorm_stats).
 * ws: roreg_mlp_head_workspace(L, n_seg, C1) doubles. */
size_t roreg_mlp_head_workspace(int L, int n_seg, int C1);
int roreg_mlp_head(const float *x, const float *pos, const float *table, const int64_t *idx, const float *conf, int m, int k, int L, int Cin,
                   const float *W1, const float *b1, int C1, const float *Wr, const float *br, float *h, float *y, const int32_t *seg_off,
                   int n_seg, int mult, float eps, float *mean_rstd, double *ws, void *stream);
/* v6: the recomputed iterations stop PER PAIR at the fixed point of the float32 iteration u <- log_mu - LSE(Z + v), v <- log_nu - LSE(Z + u)
 * (network/rot_coh_match.py:285-292).  Every iteration records the largest step any of the pair's m + n + 2 potentials took, in units of
 * max(2^-22 |u|, 2^-20) (log2 units: 2 .. 4 units in the last place of the float32 potential); the pair's remaining iterations are skipped once
 * (a) an iteration's largest step is <= 1 unit, or (b) it is <= 8 units and not smaller than the previous iteration's: the
 * potentials then only jitter in their last bits (the recomputed scores are re-rounded whenever a potential moves by an ulp).  The reference
 * always runs `iters` (= 100) iterations; past that point they move nothing but those bits, so matches are unchanged and scores agree to
 * float32 noise (tests/test_hip_rm.py and tests/test_hip_fullsize.py hold both settings to the reference's goldens).  A pair whose potentials
 * keep moving runs all `iters`.  (b) also stops a slowly converging pair (contraction ~0.88 per iteration: clustered descriptors) once its steps are
 * 4 .. 6 units, at iteration 81 .. 87 of 100: its log-couplings are then 3.6e-5 .. 6.4e-5 from a float64 evaluation of all 100 iterations, inside
 * the 1e-4 contract but 7 .. 12 times the float32 reference's own distance (tests/test_sinkhorn_convergence.py).  roreg_sinkhorn_early_exit(on): 1 = stop settled pairs (default; ROREG_OT_EARLY_EXIT=0 in the
 * environment starts with 0), 0 = always `iters` iterations, < 0 = query; returns the previous setting.  roreg_sinkhorn_iteration_stats: sum
 * of the iterations run and number of pairs over the recomputed-iteration calls since the last reset (synchronises `stream`; host pointers). */
int roreg_sinkhorn_early_exit(int on);
int roreg_sinkhorn_iteration_stats(long long *iterations, long long *pairs, int reset, void *stream);

/* ---- group-Fourier evaluation of the group convolution (csrc/fourier.hip, roreg_amd/fourier.py) ---------------
 * In the basis of the five real irreps (d = 1,3,3,4,5) the 13-stencil group conv is one dense GEMM per irrep,
 *   Out_rho [d*O][d*B] = W_rho [d*O][d*C] . X_rho [d*C][d*B]      (row-major, keypoints fastest),
 * 244 instead of 780 multiply-adds per (o,c) pair; same network function as roreg_group_conv (network/group_feat.py:16-33).
 * roreg_set_fourier_tables: F [60 (q = (rho,i,l))][60 (g)], the orthonormal transform (host pointer).
 * roreg_irrep_gemm_tiles:   fills / counts the (irrep, m-tile, n-tile) work list of one layer.
 * roreg_irrep_gemm:         the five GEMMs in one launch; X/Out/Wpack are host arrays of 5 device pointers; Wpack[rho] is
 *                           roreg_group_conv_pack_weights(KS=1) of the [round_up(d*O,128)][d*C] matrix.  Add (nullable): 5 device
 *                           pointers shaped like Out; Out = W.X + Add (the residual short cut of network/ops.py:46-64 taken in the
 *                           irrep domain).
 * roreg_ft_nonlin:          per (keypoint, channel): inverse transform (or group-domain input) -> + bias (+ bias2)
 *                           (+ group-domain residual) -> BatchNorm(eval)+ReLU (optional) -> forward transform (or group-domain
 *                           output [B,C,60], or only the Lout columns selected by g_map -- the ET trunk keeps 45 live columns).
 *                           Coefficients are one flat buffer of 60*C*Bp floats, Bp = B rounded up to 32: irrep rho occupies
 *                           [off_rho*C*Bp, off_{rho+1}*C*Bp) as the row-major GEMM operand [d*C][d*Bp] (row (l,c); columns blocked by
 *                           32 keypoints: column = (b/32)*(32*d) + i*32 + b%32; pad keypoints hold zeros).  roreg_irrep_gemm* is
 *                           called with B := Bp. */
int roreg_set_fourier_tables(const float *F_host);
size_t roreg_irrep_gemm_tiles(int O, int B, int32_t *tiles_host);            /* 128-row m-tiles */
size_t roreg_irrep_gemm_tiles_m(int O, int B, int tile_m /* 128 | 256 */, int32_t *tiles_host);
int roreg_irrep_gemm(const float *const *X, float *const *Out, const float *const *Add, const float *const *Wpack, int C, int O, int B,
                     const int32_t *tiles_dev, int n_tiles, void *stream);
/* Same GEMMs on the bf16 matrix cores with f32 accuracy: every operand is split into three bf16 pieces and the six cross products
 * of order <= 4 are accumulated in f32 (error at the f32 rounding level; 2.67x fewer matrix-core cycles than the f32-input MFMA).
 * Wsplit[rho]: uint16 bf16 bits, layout [3 splits][d*C/16][2 k-octets][round_up(d*O,128)][8]. */
int roreg_irrep_gemm_split(const float *const *X, float *const *Out, const float *const *Add, const void *const *Wsplit, int C, int O, int B,
                           const int32_t *tiles_dev, int n_tiles, void *stream);
/* The same GEMMs with fp16 x 2 operands and power-of-two block scaling (half the matrix-core work of the bf16 x 3 split).  The block is
 * ONE KEYPOINT: all coefficients of keypoint b (every channel, every irrep) share the scale 2^e(b), e(b) = 14 - exponent(x_bound_dev[b]),
 * where x_bound_dev [B] is a bound on |coefficient| known BEFORE the coefficients exist (below), so the producer roreg_ft_nonlin(split = 2)
 * writes them already split -- X[rho] holds 32-bit words fp16(x 2^e) | fp16(x 2^e - hi) << 16 at the float pitch -- and the GEMM only
 * permutes bytes while staging.  hi + lo keep 22 significant bits of every operand within ~11 binades of the bound and an absolute error
 * below 2^-39 of the bound beneath that; products hi.hi + hi.lo + lo.hi, f32 accumulate, exact rescale per column by 2^-(e(b) + w_exp).
 * A keypoint's output depends on its own column only: results are independent of batch composition (test/extractor.py:51-58).
 * Bound propagation: with next_u_dev / next_v_dev [O] and out_bound_dev [B] (zeroed by the caller) the epilogue reduces
 * max over (o, q) of u_o |T_oq(b)| + v_o per keypoint (atomic max), which bounds the coefficients of the NEXT transform's output when
 * u_o = 60 |bn_scale_o| and v_o = sqrt(60) (|bn_scale_o| |bias_o| + |bn_shift_o|) (orthonormal transform: |IFT(T)(g)| <= sqrt(60) max_q |T_q|,
 * |FT(x)_q| <= sqrt(60) max_g |x(g)|).  Wsplit2[rho]: fp16 bits, layout [2 (hi, lo)][d*C/16][2 k-octets][round_up(d*O,128)][8]. */
int roreg_irrep_gemm_f16x2(const float *const *X, float *const *Out, const float *const *Add, const void *const *Wsplit2,
                           const float *x_bound_dev, int w_exp, const float *next_u_dev, const float *next_v_dev, float *out_bound_dev,
                           int C, int O, int B, const int32_t *tiles_dev, int n_tiles,
                           int tile_m /* 128 | 256 (O % 256 == 0): the m-tile the list was built with; 256 = 8-wave workgroups */,
                           int x_planes /* X[rho] is in HALF-BLOCK layout (roreg_ft_nonlin out_planes): row pitch and 32-column blocks of the word layout, but every
                           128-byte block holds its 32 fp16 hi values followed by its 32 lo values (each half in the column order 0, 16, 1, 17, ...) instead of 32
                           words hi | lo << 16; the
                           activations then reach LDS by LDS-DMA and the matrix cores through transposing LDS reads, no register staging
                           (needs tile_m = 256); x_planes = 1: 32x32x16 MFMAs, results bitwise those of the word layout; x_planes = 2 (round 4): the same
                           operands and LDS images under v_mfma_f32_16x16x32_f16 (K = 32 per step: ~4 % faster, the same error bound, last bits differ) */, void *stream);
/* v5: how the x_planes = 2 kernel is launched.  0: one 8-wave workgroup per 256 x 256 tile (round 4).  1: PERSISTENT workgroups, one per CU, that walk
 * the list's per-XCD streams and request the next tile's first operand stages before they store the finished one (irrep_gemm_xdma16p_kernel,
 * csrc/fourier.hip).  2: 4-wave workgroups on 256 x 128 HALF tiles in 80 KB of LDS, two per CU, so that one's prologue and epilogue run under the
 * other's loop (irrep_gemm_xdma16h_kernel).  The same MFMA sequence per output element in all three: bitwise the same results.  Other values:
 * query.  Returns the previous setting; the initial one is the environment's ROREG_GEMM_PERSIST (unset = the default). */
int roreg_gemm_persistent(int on);
/* v6f (addition, ROREG_ABI_VERSION stays 6): the extractor's two thin layers in roreg_irrep_gemm_f16x2 with word-layout activations (x_planes = 0)
 * and no residual.  1 (the initial setting unless the environment says ROREG_GEMM_THIN=0): C == 32 with O % 32 == 0, O <= 512 runs
 * irrep_gemm_thin_k_kernel (a workgroup owns 256 columns and all rows, the activations are fetched once) and O == 32 runs irrep_gemm_thin_m_kernel
 * (no padded rows, the activation panel is read once); the tile list is not used.  0: the generic kernel.  The same MFMA sequence per output
 * element either way: bitwise the same results and the same propagated bound.  Other values: query.  Returns the previous setting. */
int roreg_gemm_thin(int on);
/* v6k (additions, ROREG_ABI_VERSION stays 6): the end of the extractor in one pass per keypoint (fp16 x 2, float32 storage).
 * roreg_irrep_gemm_f16x2_rows: Conv_out (O = 32, word-layout activations X[rho] as roreg_irrep_gemm_f16x2 takes them, no residual, no propagated bound) on
 * irrep_gemm_thin_m_kernel's loop with the result in PER-KEYPOINT ROWS, T3r [B][60][32] float32 (B % 32 == 0, the padded count): element [b][q][o] is
 * coefficient q = off_rho + i d + l of channel o, the value roreg_irrep_gemm_f16x2 stores at row (l, o), column (b / 32) 32 d + 32 i + b % 32 of Out[rho] --
 * the same arithmetic per element, another address. */
int roreg_irrep_gemm_f16x2_rows(const float *const *X, float *T3r, const void *const *Wsplit2, const float *x_bound_dev, int w_exp, int C, int B, void *stream);
/* roreg_gf_finish: from T3r and the extractor's input x [B][32][60] (float32) to everything a cloud keeps, one wave per keypoint, bit for bit what these
 * four launches produce (network/group_feat.py:37-45, test/matcher.py:69-72):
 *     raw    = roreg_ft_nonlin(Xin = T3, bias = b_out, resid_spatial = x, out_spatial, split = 2)      (IFT(T3) + b_out) + x
 *     eqv    = roreg_gf_finalize(raw)                                                                  raw / clamp_min(|raw|_2 over the channels, 1e-4)
 *     inv    = roreg_inv_descriptor(eqv) or roreg_inv_descriptor_roles(eqv, ..)                        (role_out columns 2 and 3; role_* all NULL: no roles)
 *     eqv_ft = roreg_feat_coefs(eqv, split = 2)                                                        [B][32][60]
 * Both transforms run with columns = the keypoint's channels; a column is one (keypoint, channel) pair there as here, with its own block scale. */
int roreg_gf_finish(const float *T3r, const float *x, const float *b_out, const float *role_scale /* [64] */, const float *role_shift /* [64] */,
                    float *eqv, float *inv, float *role_out /* [B][4] */, float *eqv_ft, int B, void *stream);
/* 1 (the initial setting unless the environment says ROREG_GF_FINISH=0): callers that can (RegistrationEngine) end the extractor with the two entries above;
 * 0: with the four launches.  The library only keeps the setting.  Other values: query.  Returns the previous setting. */
int roreg_gf_finish_route(int on);
/* bound_out[b] (b < round_up(B,32); 0 for pad keypoints) = sqrt(60) max_{c,g} |act(x[b,c,g])| >= every coefficient of FT(act(x[b])), act =
 * ReLU(bn_scale_c x + bn_shift_c) or the identity (bn NULL): the x_bound of a layer whose input is a group-domain tensor [B,C,60]. */
int roreg_row_bound(const void *x_spatial, int x_bf16 /* x is bfloat16 instead of float32 */, const float *bn_scale, const float *bn_shift,
                    float *bound_out, int B, int C, void *stream);
int roreg_ft_nonlin(const float *Xin /* flat [60*C*B] */, const float *x_spatial, const float *bias,
                    const float *bias2, const float *bn_scale, const float *bn_shift, const float *resid_spatial,
                    float *Xout /* flat [60*C*B] */, float *out_spatial /* [B,C,Lout] */,
                    const int32_t *g_map /* optional [60]: group column -> compact output column (< Lvalid) or -1 */,
                    int Lout /* row pitch of the compact output, >= Lvalid; pad columns are zero */, int Lvalid,
                    int B, int C, int split /* 0: f32-input MFMA; 1: 3 x bf16 split MFMAs; 2: fp16 x 2 with per-column (per-keypoint) power-of-two scales */,
                    const float *out_bound /* split = 2 with Xout: per-keypoint bound [round_up(B,32)] on |coefficient|; Xout then holds the fp16 hi/lo
                                              words roreg_irrep_gemm_f16x2 consumes (NOT floats) */,
                    float *out_rowmax /* optional, with out_spatial: [B], zeroed by the caller; receives max |out_spatial[b]| per keypoint (the block
                                         scale of roreg_group_conv_f16x2) */,
                    int spatial_bf16 /* x_spatial / resid_spatial point to bfloat16 tensors (BASELINE config 5: group features stored as bf16) */,
                    int out_planes /* split = 2 with Xout: write Xout in the HALF-BLOCK layout roreg_irrep_gemm_f16x2(x_planes = 1) consumes */,
                    void *stream);
/* v5: the inverse transform + bias + BatchNorm + ReLU of roreg_ft_nonlin with the group-domain result [B,C,Lout] written as WORDS fp16 hi | fp16 lo << 16
 * of value * 2^e_b, e_b = the block exponent of out_bound[b] (a bound on |ReLU(BN(.))| of row b that exists before the tensor does: the producing
 * GEMM's propagated bound with u_o = sqrt(60) |scale_o|, v_o = |scale_o| |bias_o| + |shift_o|) -- the operand of roreg_group_conv_f16x2_packed.
 * raw_col (nullable, [B,C] float32): the value BEFORE BatchNorm / ReLU at group element raw_g (ET's identity short cut, eqv_trans.py:112-117). */
int roreg_ft_nonlin_packed(const float *Xin, const float *bias, const float *bn_scale, const float *bn_shift, uint32_t *out_words,
                           const int32_t *g_map, int Lout, int Lvalid, int B, int C, const float *out_bound, float *raw_col, int raw_g,
                           void *stream);
/* v6b: roreg_ft_nonlin(x_spatial = the ET input [B,128,60] of roreg_lt_prepare_batch, split = 2, Xout) without that tensor: row b, channel k*32 + c is read
 * from rows[b][k] (roreg_lt_prepare_rows) at channel c, through P[dr[b]] for k = 0 and 2.  Same words as the two-step route, bit for bit. */
int roreg_ft_nonlin_gathered(const uint64_t *rows /* [B][4] */, const int64_t *dr /* [B] */, int feat_bf16, const float *bn_scale /* [128] */,
                             const float *bn_shift, float *Xout, int B, const float *out_bound /* [round_up(B,32)] */, int out_planes, void *stream);

/* ---- v6c: dense point-to-point ICP of registered pairs (csrc/icp.hip) ---------------------------------------------------------------
 * No reference counterpart: the reference stops at the keypoint transform; this refines it on the full clouds without leaving the device.
 * Semantics (tests/_icp_oracle.py restates them in numpy): coordinates are float32, all arithmetic widens them to float64; per iteration
 * p' = ((R_r0 x + R_r1 y) + R_r2 z) + t_r, nearest target point by d2 = (dx dx + dy dy) + dz dz with exact ties going to the lowest original
 * target row, inlier iff d2 <= max_dist^2, centroids over the inliers, H = sum (q - c_q)(p - c_p)^T in a second pass,
 * R+ = U diag(1, 1, det(U V^T)) V^T, t+ = c_q - R+ c_p.  No floating-point atomics: every sum goes through fixed per-workgroup slots.
 *
 * v6c, no reference counterpart.  A grid is one device buffer: this 64-byte descriptor, the cloud's points sorted by cell as 16-byte records
 * (x, y, z, original row as bits; ascending original row inside a cell) and int32 cell starts [cells + 2] (the first cells + 1 are the table).
 * Cell edge = the smallest max_dist * 2^s that keeps the table within 2^24 cells over the bounding box [lo, hi] padded by one cell.
 * roreg_icp_grid_size (HOST function, lo / hi host pointers) fills *desc_host and returns the buffer's bytes; *workspace_bytes: what
 * roreg_icp_grid_build needs. */
typedef struct roreg_icp_grid_desc {
    double origin[3];                  /* corner of cell (0,0,0) = lo - edge */
    double edge;
    int32_t dims[3];
    int32_t n;                         /* points */
    int64_t cells;                     /* dims[0] * dims[1] * dims[2], x fastest */
    int64_t reserved;
} roreg_icp_grid_desc;
size_t roreg_icp_grid_size(const double *lo_host, const double *hi_host, int n, double max_dist, roreg_icp_grid_desc *desc_host,
                           size_t *workspace_bytes);
/* v6c, no reference counterpart.  Counting sort of points [n,3] f32 into `grid`: cell ids, integer histogram, exclusive scan, fill, then
 * every cell put in ascending original row (so neither the tie rule nor any summation order depends on atomic timing). */
int roreg_icp_grid_build(const float *points, const roreg_icp_grid_desc *desc_host, void *grid, void *workspace, size_t workspace_bytes,
                         void *stream);
/* v6c, no reference counterpart.  One pair: target grid (cloud 0), source grid (cloud 1, SAME max_dist: its records are the source points in
 * cell order, which keeps neighbouring queries on neighbouring target cells), T0 [4,4] f64 (k0 ~ k1 R^T + t), and the pair's first slot:
 * pair p owns ceil(n_src / 1024) consecutive slots (one per 1024-point chunk of the sorted source), slot0 = the sum over the pairs before it.
 * A pair's chunking depends on the pair alone, so its result is bit-identical whatever batch it runs in. */
typedef struct roreg_icp_task {
    const void *tgt_grid;
    const void *src_grid;
    const double *T0;
    int32_t n_src;
    int32_t slot0;
} roreg_icp_task;
size_t roreg_icp_batch_workspace(int n_tasks, long long total_slots);
/* v6c, no reference counterpart.  max_iter rounds of (search, covariance, solve) enqueued with no host synchronisation; a pair that converged
 * (rotation step < tol_deg degrees AND translation step < tol_t), lost its support (fewer than 3 inliers or rank(H) <= 1: T kept) or started
 * from a non-finite T0 sets a device-side word that makes its later workgroups return at once.
 * work: int32 [n_work, 2] rows (pair, chunk), pair < 0 = padding; workgroup b takes row b (the binding deals a pair's rows to one of eight
 * interleaved streams, b % 8: its target cells then stay in one XCD's L2 -- speed only).
 * Outputs: T_out [n,4,4] f64, iters_out (searches executed), inliers_out and rmse_out (of the last executed search), status_out
 * (0 converged, 1 max_iter, 2 no_support, 3 non-finite T0: returned unchanged, iters 0, inliers 0, rmse NaN).
 * assign_out (nullable, int32 [total_slots * 1024]): at slot0 * 1024 + source ORIGINAL row the target ORIGINAL row of the last executed
 * search, -1 = no inlier.  stats_out (nullable, f64 [n,16]): n, c_q, c_p, H (row-major) of the last executed iteration. */
int roreg_icp_batch(const roreg_icp_task *tasks, int n_tasks, const int32_t *work, int n_work, long long total_slots, double max_dist,
                    int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out, double *rmse_out,
                    int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6d: surface normals and point-to-plane ICP (csrc/icp.hip; additions, ROREG_ABI_VERSION stays 6) --------------------------------------
 * No reference counterpart.  Semantics (tests/_icp_plane_oracle.py restates them in numpy):
 * Normals of a cloud for (radius r, min_neighbors k): the neighbourhood of point i is every point j of the cloud, itself included, with
 * d2 = (dx dx + dy dy) + dz dz <= r r (the search's formula; membership exact, a point at exactly r is in).  On the offsets y_j = x_j - x_i
 * (exact): the count m and ybar = sum y / m, then C = sum (y - ybar)(y - ybar)^T in a second pass, both in ascending cell and ascending
 * original row inside a cell, the sums carried with their rounding errors (two-sum / two-product) so that the rounded C is the same from any
 * grid of the cloud; C = V diag(lambda) V^T by cyclic Jacobi; the normal is the unit eigenvector of the smallest eigenvalue, sign as it comes.
 * Valid iff m >= k and lambda_mid > 1e-8 lambda_max; an invalid row carries the zero vector.
 * One point-to-plane iteration under (R, t): the v6c search unchanged (nearest row, d2 <= max_dist^2, ties to the lowest row, first-pass
 * slots); c = R c_p + t, c_p the centroid of the untransformed source points of all distance inliers; a correspondence counts iff it is a
 * distance inlier and its target normal n is valid: p' = R p + t, a = p' - c, e = n . (p' - q), J = [a x n, n]; A = sum J J^T, b = -sum J e
 * through fixed (pair, chunk) slots; A = V diag(lambda) V^T by cyclic Jacobi; no_support (T kept) when n_valid < 6 or
 * lambda_min <= 1e-10 lambda_max; else x = V diag(1 / lambda) V^T b = (w, v), dR = exp([w]x), R+ = dR R, t+ = dR (t - c) + c + v.
 * Convergence test, max_iter, non-finite T0, the done word and the status codes are v6c's; inliers = n_valid, rmse = sqrt(sum e^2 / n_valid).
 *
 * v6d, no reference counterpart.  out [n,4] f64 in ORIGINAL row order = (nx, ny, nz, m) per point of the cloud whose grid (built for any
 * radius) is `grid`. */
int roreg_icp_normals(const void *grid, double radius, int min_neighbors, double *out, void *stream);
/* v6d, no reference counterpart.  roreg_icp_task with the target cloud's normal table (roreg_icp_normals' out). */
typedef struct roreg_icp_plane_task {
    const void *tgt_grid;
    const void *src_grid;
    const double *tgt_normals;
    const double *T0;
    int32_t n_src;
    int32_t slot0;
} roreg_icp_plane_task;
/* v6d, no reference counterpart. */
size_t roreg_icp_plane_batch_workspace(int n_tasks, long long total_slots);
/* v6d, no reference counterpart.  roreg_icp_batch's argument list over roreg_icp_plane_task: max_iter rounds of (search, plane pass, solve).
 * stats_out (nullable, f64 [n,32]): n_valid, c (3), the 21 upper entries of A row by row, b (6), sum e^2 of the last executed iteration. */
int roreg_icp_plane_batch(const roreg_icp_plane_task *tasks, int n_tasks, const int32_t *work, int n_work, long long total_slots, double max_dist,
                          int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out, double *rmse_out,
                          int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6i: plane-to-plane (generalized) ICP (csrc/icp.hip; additions, ROREG_ABI_VERSION stays 6) -------------------------------------------------
 * No reference counterpart.  Semantics (tests/_icp_gicp_oracle.py restates them in numpy): the v6c search and the v6d linearisation centre
 * c = R c_p + t unchanged; for every distance inlier (source record p, assigned target record q): p' = R p + t, d = p' - q, a = p' - c;
 * n_q the target normal at q's original row, n_p the source normal at p's original row, m = R n_p; kappa = 1 - epsilon;
 * S = 2 I - kappa (n_q n_q^T + m m^T), which is C_q + R C_p R^T for the surface-aligned covariances C = V diag(1, 1, epsilon) V^T =
 * I - kappa n n^T; M = S^-1 by the adjugate over the determinant (eigenvalues of S in [2 epsilon, 2]); J = [-[a]x, I] (the plane method's J is
 * n^T times this one); A = sum J^T M J, b = -sum J^T M d, and sum d^T M d, through fixed (pair, chunk) slots in the v6d layout.  A zero normal
 * row contributes no n n^T term (that point's covariance is the identity): nothing is skipped, so n_valid = n = the distance inliers, and
 * with both tables zero (or epsilon = 1) the weighting is uniform.  M is held fixed within an iteration.  The solve is v6d's: 6x6 Jacobi,
 * no_support (T kept) when n < 6 or lambda_min <= 1e-10 lambda_max, x = (w, v), dR = exp([w]x), R+ = dR R, t+ = dR (t - c) + c + v.
 * inliers = n, rmse = sqrt(sum d^T M d / n): the whitened residual, not a Euclidean distance (v6g gives that).
 *
 * v6i, no reference counterpart.  roreg_icp_task with both clouds' normal tables (roreg_icp_normals' out: [n,4] f64, 32-byte aligned, in
 * original row order) and the pair's epsilon, 0 < epsilon <= 1 (the caller checks it: the records live on the device).  56 bytes. */
typedef struct roreg_icp_gicp_task {
    const void *tgt_grid;
    const void *src_grid;
    const double *tgt_normals;
    const double *src_normals;
    const double *T0;
    double epsilon;
    int32_t n_src;
    int32_t slot0;
} roreg_icp_gicp_task;
/* v6i, no reference counterpart. */
size_t roreg_icp_gicp_batch_workspace(int n_tasks, long long total_slots);
/* v6i, no reference counterpart.  roreg_icp_plane_batch's argument list over roreg_icp_gicp_task: max_iter rounds of (search, gicp pass, solve).
 * stats_out (nullable, f64 [n,32]): n, c (3), the 21 upper entries of A row by row, b (6), sum d^T M d of the last executed iteration. */
int roreg_icp_gicp_batch(const roreg_icp_gicp_task *tasks, int n_tasks, const int32_t *work, int n_work, long long total_slots, double max_dist,
                         int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out, double *rmse_out,
                         int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6p: robust losses in the point-to-plane and plane-to-plane iterations (csrc/icp.hip, csrc/icp_math.h; additions, ROREG_ABI_VERSION stays 6) --
 * No reference counterpart.  Semantics (tests/_icp_robust_oracle.py restates them in numpy): iteratively re-weighted least squares inside the
 * second pass of v6d and v6i.  With the loss's scale k > 0 (finite) and u = r / k the weight of a correspondence is
 *   huber: 1 if |u| <= 1 else 1 / |u|;  cauchy: 1 / (1 + u^2);  gm (Geman-McClure): 1 / (1 + u^2)^2;  tukey: (1 - u^2)^2 if |u| <= 1 else 0
 * (csrc/icp_math.h robust_weight: all four continuous in r; an overflowing u^2 gives 0 or 1 / |u|, never NaN).
 * plane: r = e, v6d's signed plane residual; A = sum w J J^T, b = -sum w J e.
 * gicp:  r = sqrt(2 epsilon d^T M d) -- where both normals agree, the point-to-plane distance in metres plus epsilon times the tangential one,
 *        so that one scale means the same under both methods --; A = sum w J^T M J, b = -sum w J^T M d.
 * Unchanged under a loss: the search, the distance gate and the centre c (all distance inliers, unweighted); which correspondences count;
 * slot word 0 (the count) and word 28 (sum e^2 / sum d^T M d, unweighted: inliers and rmse keep their meaning across losses); the 29-word
 * slot layout; the solve with its n_valid < 6 and lambda_min <= 1e-10 lambda_max tests (all-zero weights give A = 0, hence no_support with T
 * kept); the convergence test and the status codes.  Every task carries its own loss and scale; a pair's bits depend on neither the batch nor
 * the other tasks' losses. */
typedef enum roreg_icp_loss {
    ROREG_ICP_LOSS_NONE = 0,           /* weight 1: the unweighted sums (through the weighted kernel) */
    ROREG_ICP_LOSS_HUBER = 1,
    ROREG_ICP_LOSS_CAUCHY = 2,
    ROREG_ICP_LOSS_GM = 3,
    ROREG_ICP_LOSS_TUKEY = 4
} roreg_icp_loss;
/* v6p, no reference counterpart.  roreg_icp_plane_task followed by the loss: 56 bytes.  The caller checks loss and scale (the records live on
 * the device). */
typedef struct roreg_icp_plane_robust_task {
    const void *tgt_grid;
    const void *src_grid;
    const double *tgt_normals;
    const double *T0;
    int32_t n_src;
    int32_t slot0;
    double scale;                      /* k > 0, finite, in the unit of the coordinates */
    int32_t loss;                      /* roreg_icp_loss */
    int32_t reserved;
} roreg_icp_plane_robust_task;
/* v6p, no reference counterpart.  roreg_icp_gicp_task followed by the loss: 72 bytes. */
typedef struct roreg_icp_gicp_robust_task {
    const void *tgt_grid;
    const void *src_grid;
    const double *tgt_normals;
    const double *src_normals;
    const double *T0;
    double epsilon;
    int32_t n_src;
    int32_t slot0;
    double scale;
    int32_t loss;
    int32_t reserved;
} roreg_icp_gicp_robust_task;
/* v6p, no reference counterpart. */
size_t roreg_icp_plane_robust_batch_workspace(int n_tasks, long long total_slots);
size_t roreg_icp_gicp_robust_batch_workspace(int n_tasks, long long total_slots);
/* v6p, no reference counterpart.  roreg_icp_plane_batch's / roreg_icp_gicp_batch's argument list over the robust records.  stats_out (nullable,
 * f64 [n,32]): n_valid, c (3), the 21 upper entries of the WEIGHTED A row by row, the weighted b (6), the unweighted sum e^2 / sum d^T M d. */
int roreg_icp_plane_robust_batch(const roreg_icp_plane_robust_task *tasks, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                 double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out,
                                 double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes,
                                 void *stream);
int roreg_icp_gicp_robust_batch(const roreg_icp_gicp_robust_task *tasks, int n_tasks, const int32_t *work, int n_work, long long total_slots,
                                double max_dist, int max_iter, double tol_deg, double tol_t, double *T_out, int32_t *iters_out, int32_t *inliers_out,
                                double *rmse_out, int32_t *status_out, int32_t *assign_out, double *stats_out, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- v6g: read-only evaluation of a dense pair under a given transform (csrc/icp.hip; additions, ROREG_ABI_VERSION stays 6) -------------
 * No reference counterpart (the reference reads gt.info, it never computes one).  Semantics (tests/_dense_eval_oracle.py restates them in
 * numpy): coordinates are float32 widened to float64; T [4,4] f64 in the engine's convention k0 ~ k1 R^T + t, cloud 0 the target, cloud 1
 * the source, the upper-left block taken to be a rotation.
 * Forward (source -> target under T): exactly the v6c search: p' = ((R_r0 x + R_r1 y) + R_r2 z) + t_r, nearest target row by
 * d2 = (dx dx + dy dy) + dz dz, exact ties to the lowest original target row, a correspondence iff d2 <= max_dist^2.  Over the
 * correspondences, x the UNtransformed source point: n01, S01 = sum d2, sum x (3) and sum x x^T (6; every product of two widened float32
 * values is exact in float64, only the summation rounds).
 * Backward (target -> source): the same search with the roles swapped under the inverse taken by transposition, Rinv = R^T,
 * tinv_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2): n10 and S10.
 * Per pair: rmse01 = sqrt(S01 / n01), rmse10 likewise (NaN when the count is 0); overlap1 = n01 / n_src, overlap0 = n10 / n_tgt (NaN for
 * an empty cloud); the 6x6 information matrix in Redwood's order and scaling, the one RR_cal.computeTransformationErr consumes with
 * e = (t, vector part of the unit quaternion): Lambda = sum G^T G, G = [I3 | -2 [x]x], i.e. Lambda_tt = n01 I, Lambda_tr = -2 [sum x]x,
 * Lambda_rt = Lambda_tr^T, Lambda_rr = 4 (tr(M) I - M), M = sum x x^T (its diagonal formed as the sum of the two other squares).  x is in
 * the source frame because inv(gt) @ pose acts there; the factor 2 is the quaternion's half angle: with it e^T Lambda e / Lambda[0,0] is
 * the mean squared displacement of the correspondences to first order.
 * Status: 0 ok (zero correspondences included: Lambda = 0), 1 = T not finite (counts 0, both rmse NaN, Lambda = 0).
 * Determinism: no floating-point atomics; every sum goes through fixed (task, chunk) slots of 1024 sorted source records and the slots are
 * reduced in ascending chunk order by one finishing kernel, so a pair's bits do not depend on the batch it runs in nor on the radius its
 * TARGET grid was built for.  The SOURCE grid's record order (hence the radius it was built for) does fix the summation order.
 *
 * v6g, HOST function: bytes of workspace for n_pairs pairs whose 2 n_pairs tasks own total_slots slots. */
size_t roreg_icp_eval_workspace(int n_pairs, long long total_slots);
/* v6g.  tasks: 2 n_pairs rows of roreg_icp_task with T0 read as T: row p is pair p forward (tgt_grid = cloud 0, src_grid = cloud 1, n_src =
 * cloud 1's points), row n_pairs + p the same pair backward: the grids SWAPPED, n_src = cloud 0's points, the SAME T (the kernel inverts it);
 * every row owns ceil(n_src / 1024) slots from its slot0.  work: int32 [n_work, 2] rows (task, chunk) over all 2 n_pairs tasks, task < 0 =
 * padding (roreg_icp_batch's placement).  One search launch over all rows and one finishing launch, no host synchronisation.
 * stats_out f64 [n,8] = (n01, n10, overlap0, overlap1, rmse01, rmse10, S01, S10); info_out f64 [n,36] = Lambda row-major in the order
 * (t, r); status_out int32 [n]; assign_out (nullable, int32 [total_slots * 1024]): at slot0 * 1024 + the task's query ORIGINAL row the
 * matched ORIGINAL row of the other cloud, -1 = none (forward tasks: target row per source row; backward: source row per target row). */
int roreg_icp_eval_batch(const roreg_icp_task *tasks, int n_pairs, const int32_t *work, int n_work, long long total_slots, double max_dist,
                         double *stats_out, double *info_out, int32_t *status_out, int32_t *assign_out, void *workspace, size_t workspace_bytes,
                         void *stream);

/* ---- v6e: voxel-grid downsampling of a dense cloud (csrc/voxel.hip; additions, ROREG_ABI_VERSION stays 6) -------------------------------
 * The reference's first upstream step (testset.py: ME.utils.sparse_quantize(xyz / voxel_size, return_index=True) and
 * np.floor(xyz / voxel_size)) with every output defined independently of scheduling; tests/_voxel_oracle.py restates it in numpy and the
 * device equals it exactly.  points [n,3] f32; per axis k = floor((double)x / voxel), one float64 division (-0.0 falls in voxel 0); valid
 * keys -2^20 <= k < 2^20.  Voxels are numbered 0..m-1 in ascending order of their lowest original row.  Outputs (capacity n, the first m
 * rows defined): coords int32 [m,3]; first int32 [m] (lowest original row of the voxel, strictly ascending); counts int32 [m]; inverse int32
 * [n] (voxel number of every row); centroid f64 [m,3] = (sum of (double)x over the members in ascending original row, starting from the
 * first member -- sequential, no tree, no floating-point atomic) / count, one float64 division.  info int32 [2] = (m, flags): flags bit 0 = a
 * row has a non-finite coordinate, bit 1 = a key is out of range, bit 2 = the table overflowed (cannot happen at capacity >= 2n); such
 * rows take no voxel and get inverse = -1, and the caller reads info back (the call's one synchronising copy) and refuses the result.
 *
 * v6e, HOST function: bytes of workspace for n rows (0 <= n <= 2^30; 0 otherwise). */
size_t roreg_voxel_workspace(int n);
/* v6e.  No host synchronisation inside; the workspace is cleared by the call itself.  n == 0: info = (0, 0), nothing else is touched. */
int roreg_voxel_downsample(const float *points, int n, double voxel, int32_t *inverse, int32_t *first, int32_t *counts, int32_t *coords,
                           double *centroid, int32_t *info, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6h: multiway registration, batched Levenberg-Marquardt optimisation of pose graphs (csrc/pose_graph.hip, csrc/pg_math.h; additions,
 * ROREG_ABI_VERSION stays 6) -------------------------------------------------------------------------------------------------------------
 * No reference counterpart.  tests/_pose_graph_oracle.py restates the semantics in numpy.  Everything is float64.
 * A graph has C nodes and E edges.  Pose P_c [4,4] maps cloud c into the world (overlap_matrix's convention).  Edge k = (i, j, T_k, Lambda_k),
 * i != j: T_k maps cloud j into cloud i (the engine's PairResult transform for (id0 = i, id1 = j)); Lambda_k is v6g's information matrix.
 * Duplicate edges are legal, in either orientation.  Every upper-left 3x3 block is taken to be a rotation: inverses go by transposition.
 * Residual: E_k = T_k^-1 P_i^-1 P_j, e_k = (t(E_k), vector part of the unit quaternion of R(E_k) with w >= 0, by Shepperd's four-branch rule),
 * chi2_k = e_k^T Lambda_k e_k = RR_cal.computeTransformationErr(E_k, Lambda_k) * Lambda_k[0,0].
 * Cost: c = sum rho_k.  tau <= 0: rho = chi2, w = 1.  tau > 0 (metres): mu = tau^2 Lambda[0,0], rho = mu chi2 / (mu + chi2),
 * w = (mu / (mu + chi2))^2 (Geman-McClure).  An edge with Lambda[0,0] == 0 contributes nothing and reports w = 0.
 * Update: P_c <- P_c [Exp(omega_c), v_c; 0, 1], delta_c = (v_c, omega_c), Rodrigues with the series below 1e-8; the Jacobians are the exact
 * first derivatives of e_k under that right perturbation: J_j = blockdiag(R_E, (w I + [qv]x) / 2), J_i = -J_j Ad(M^-1), M = P_i^-1 P_j.
 * System: H = sum w_k J_k^T Lambda_k J_k, g = sum w_k J_k^T Lambda_k e_k with the weights frozen at the current poses; the anchor and every
 * node that is not reachable from it through the edge list are left out (var = -1) and keep their initial pose; an edge with such an end
 * contributes nothing.  One round: solve (H + lambda diag(H)) delta = -g by Cholesky; P' = P Exp(delta), c' its cost; if every
 * |v_c| <= tol_t and |omega_c| <= tol_rot, or |c - c'| <= tol_cost c: take P' and stop (converged); else if c' < c: accept,
 * lambda <- max(lambda / 10, 1e-12); else reject, lambda <- 10 lambda.  A pivot that is not positive and finite is a rejected round.
 * lambda > 1e12 after a rejection ends the run (stalled); max_iter rounds end it (max_iter); a non-finite pose, transform, information
 * matrix, option or starting cost ends it before the first round (nonfinite: the poses stay at their initial values, both costs NaN).
 * Determinism: no floating-point atomics, every sum has one owner and a fixed order; a graph's bits depend neither on the batch it runs in
 * nor on its place in it.
 *
 * One graph of the batch.  node0 / edge0 / act0 / h0 are running totals over the graphs before it (nodes, edges, optimised nodes, and
 * sum (6 n_act)^2: the graph's H in the workspace); n_act = the optimised nodes (reachable, not the anchor). */
typedef struct roreg_pg_graph {
    int32_t node0, n_nodes, edge0, n_edges, act0, n_act, anchor, reserved0;
    int64_t h0;
    double tau, lambda0, tol_t, tol_rot, tol_cost, reserved1;
} roreg_pg_graph;   /* 88 bytes */
/* v6h, HOST function: bytes of workspace for the batch; 0 if a graph has more than 256 nodes or 65536 edges or the table is inconsistent. */
size_t roreg_pg_workspace(const roreg_pg_graph *graphs_host, int n_graphs);
/* v6h.  graphs_host: the descriptor table in host memory (limits, sizes), graphs: the same table on the device.  Device tables, all built
 * by the caller from integers only: edge_i, edge_j int32 [E_total] (node numbers inside the graph), edge_graph int32 [E_total];
 * transforms f64 [E_total,16]; infos f64 [E_total,36]; var int32 [C_total] (the node's block 0..n_act-1 in its graph's system, ascending
 * in the node number, or -1); inc_ptr int32 [C_total + 1] / inc_edge int32 [2 E_total]: per node its incident edges (numbers in the whole
 * table) in ascending order; act_graph / act_node int32 [A_total]: the optimised nodes, graph after graph in ascending node; walk int32
 * [A_total,2]: per graph from act0, (node, edge) in the order the initial poses are composed (P_j = P_i T_k or P_i = P_j T_k^-1 from the
 * edge's other end, which comes earlier in the walk or is the anchor).  has_init != 0: poses f64 [C_total,16] holds the initial poses and
 * walk is not read; otherwise the anchor and the unreachable nodes start at the identity and the others are composed along the walk.
 * All max_iter rounds are enqueued, no host synchronisation; a finished graph's workgroups return at once.
 * Outputs: poses (in place); cost_out f64 [G,2] = (starting cost, final cost); iters_out, status_out int32 [G] (0 converged, 1 max_iter,
 * 2 stalled, 3 nonfinite); weights_out, chi2_out f64 [E_total] at the final poses; history_out f64 [G,max_iter,4] = (c, c', lambda of the
 * round, decision: 1 accepted, 2 rejected, 3 rejected for a pivot (c' NaN), 4 taken and stopped; 0 = round not run).
 * For tests and tools, nullable, copies of the FIRST round's intermediate tables: lin_out f64 [E_total,56] = per edge (e 6, chi2, w, R_E 9,
 * Q 9, A 9, B 9, D 9, 3 unused) with J_j = blockdiag(R_E, Q), J_i = -[[A, B], [0, D]]; H_out f64 [sum (6 n_act)^2]: every graph's H
 * row-major, only the lower triangle defined; gd_out f64 [2, 6 A_total] = g, then delta.  They are undefined for a graph that is nonfinite. */
int roreg_pg_optimize_batch(const roreg_pg_graph *graphs_host, const roreg_pg_graph *graphs, int n_graphs, const int32_t *edge_i,
                            const int32_t *edge_j, const int32_t *edge_graph, const double *transforms, const double *infos, const int32_t *var,
                            const int32_t *inc_ptr, const int32_t *inc_edge, const int32_t *act_graph, const int32_t *act_node,
                            const int32_t *walk, int has_init, int max_iter, double *poses, double *cost_out, int32_t *iters_out,
                            int32_t *status_out, double *weights_out, double *chi2_out, double *history_out, double *lin_out, double *H_out,
                            double *gd_out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6j: sparse 3-D convolutions, the pieces of the FCGF backbone (csrc/sparse_conv.hip; additions, ROREG_ABI_VERSION stays 6) -------------
 * The reference's backbone is ResUNetBN2C on MinkowskiEngine (backbone/fcgf/resunet.py); tests/_sparse_conv_oracle.py restates the definitions
 * in numpy, roreg_amd/backbone/fcgf.py composes the network from these entries.
 * A sparse tensor at tensor stride ts: coordinates int32 [n,4] rows (item, x, y, z), x, y, z multiples of ts, unique, every item's rows one
 * contiguous segment in ascending item.  Limits: 0 <= item < 2^15 and -2^15 <= x, y, z < 2^15 (the item shares a 63-bit key with three 16-bit
 * axes; at a 2.5 cm voxel that is +-819 m).  A row outside them sets bit 1 of info[1] (bit 2: the table overflowed, cannot happen at capacity
 * >= 2n); the caller reads info back and refuses the result.  Nothing aliases: a neighbour query outside the limits is absent.
 * Kernel offsets: odd k, kappa = kx + k ky + k^2 kz (x fastest; kernel_region.hpp coordinate_at), offset (k_axis - k / 2) * step per axis.
 *
 * v6j, HOST function: bytes of workspace for a table of n rows (0 <= n <= 2^30; 0 otherwise). */
size_t roreg_sparse_map_workspace(int n);
/* v6j.  Stride 2: the coarse coordinate of c is floor(c / (2 ts)) (2 ts) per axis (a floor: -1 -> -2).  Coarse rows are numbered in ascending
 * order of their lowest fine row (this project's rule; MinkowskiEngine's order is a property of its hash map).  cuts int32 [n_items + 1]: the
 * items' segment starts among the fine rows.  Outputs: coarse int32 [m,4] (capacity n), parent int32 [n] (coarse row of every fine row),
 * coarse_cuts int32 [n_items + 1], info int32 [2] = (m, flags).  Workspace: roreg_sparse_map_workspace(n).  No host synchronisation. */
int roreg_sparse_stride_map(const int32_t *coords, int n, int ts, const int32_t *cuts, int n_items, int32_t *coarse, int32_t *parent,
                            int32_t *coarse_cuts, int32_t *info, void *workspace, size_t workspace_bytes, void *stream);
/* v6j.  map int32 [n_out, k^3]: map[u, kappa] = the row of coords_in at coords_out[u] + offset(kappa) * step in the same item, or -1.
 * Stride 1: in = out, step = ts.  Stride 2: in = fine, out = coarse, step = ts_fine.  Transposed (kernel 3, stride 2, output coordinates the
 * encoder's): in = coarse, out = fine, step = -ts_fine, the strided map with in and out swapped (coordinate_map_manager.cpp:756-806).
 * k odd, 1..7.  info int32 [2] = (0, flags of coords_in).  Workspace: roreg_sparse_map_workspace(n_in).  Indices on n_out k^3 are 64-bit. */
int roreg_sparse_kernel_map(const int32_t *coords_in, int n_in, const int32_t *coords_out, int n_out, int k, int step, int32_t *map,
                            int32_t *info, void *workspace, size_t workspace_bytes, void *stream);
/* v6j.  y[u, o] = sum over kappa ascending with map[u, kappa] >= 0, over c ascending, of x[map[u, kappa], c] W[kappa, c, o]: ONE float32 fmaf
 * chain per output element from 0, float32 operands (no narrowing), a missing neighbour is a term left out, no floating-point atomic -- a
 * row's bits do not depend on what it is batched with.  x [n_in, Cin] with row stride ldx, W [K, Cin, Cout], map [n_out, K] (a value >=
 * n_in counts as -1).  out[u, o] = relu?(fmaf(y, scale[o], shift[o]) + residual[u, o]) at row stride ldo: scale null = no scaling (shift
 * alone is a bias), shift, residual (row stride ldr) nullable, relu 0 / 1.  x, residual and out may point into column windows of wider
 * buffers (the network's concatenations cost no copy); out overlaps neither x nor residual.  Cin = 1 takes a kernel of its own. */
int roreg_sparse_conv(const float *x, int ldx, int Cin, int n_in, const int32_t *map, int n_out, int K, const float *W, int Cout,
                      const float *scale, const float *shift, const float *residual, int ldr, int relu, float *out, int ldo, void *stream);
/* v6j.  out[u] = x[u] / sqrt(sum_c x[u, c]^2), x and out [n, C] dense: the squares added by fmaf in ascending c; no epsilon (the reference's
 * normalize_feature has none). */
int roreg_sparse_l2norm(const float *x, int n, int C, float *out, void *stream);

/* ---- v6l: assembly of a cloud's group feature on the device (csrc/group_feature.hip; addition, ROREG_ABI_VERSION stays 6) -------------------
 * The reference's testset.py:170-181: every rotated keypoint takes the backbone feature of its nearest down-sampled point.  One launch per
 * batch of R rotations run through the network as one sparse tensor:
 *     out[n, f, g0 + r] = feats[cuts[r] + nn[r, n], f]            r < R, n < N, f < F;  no other element of out is touched
 * feats float32 [M,F] (dense rows), cuts int32 [R + 1] (the items' segment starts among feats' rows), nn int64 [R,N] (item-local rows:
 * roreg_nn_search's output, stacked), out [N,F,60] float32 (out_bf16 = 0) or bfloat16 (out_bf16 = 1: round to nearest even, the bits of a
 * float32 -> bfloat16 cast), all on the device.  1 <= F <= 32, 1 <= R, 0 <= g0, g0 + R <= 60.
 * info int32 [1], zeroed by the caller: set to 1 if an nn entry is outside [0, cuts[r + 1] - cuts[r]) or its row is outside feats.  Such a row
 * is not read (its elements are stored as 0); the caller reads info back and refuses the result.  No arithmetic, no atomics, no host
 * synchronisation. */
int roreg_group_feature_assemble(const float *feats, int M, int F, const int32_t *cuts, const int64_t *nn, int R, int N, int g0, void *out,
                                 int out_bf16, int32_t *info, void *stream);

/* ---- v6m: spatial-compatibility hypotheses (csrc/sc2.hip; additions, ROREG_ABI_VERSION stays 6) ----------------------------------------------
 * No reference counterpart.  Semantics (tests/_sc2_oracle.py restates them in numpy), per pair with P = keys0[matches[:,0]], Q = keys1[matches[:,1]]:
 *   a_ij = sqrt((dx dx + dy dy) + dz dz) of P_i - P_j, b_ij of Q_i - Q_j (float64, this order, no FMA);  C_ij = [i != j and |a_ij - b_ij| <= tau];
 *   deg_i = sum_j C_ij;  seeds = the S = min(M, max_seeds) rows of greatest degree, ties to the lower index, in that order;
 *   N2[s, j] = C[s, j] sum_k C[s, k] C[k, j];  set(s) = s, then at most K - 1 of the j with C[s, j] = 1 by greater N2, ties to the lower j;
 *   row h of Trans [3,4] = the Kabsch fit P ~ R Q + t over set(seeds[h]) with det R = +1 (the sign on the smallest singular direction), or, for a
 *   set of fewer than 3 members, R = I and t = P_s - Q_s.  No random numbers; every float64 sum has a fixed order.
 * One pair of roreg_sc2_hypotheses_batch (device pointers; 64 bytes).  The offsets are the caller's running sums over the tasks before this one:
 * koff of M, boff of M ceil(M / 64), hoff of S, noff of S M. */
#define ROREG_SC2_MAX_M 8192       /* correspondences per pair */
#define ROREG_SC2_SEED_TILE 64     /* the second-order kernel's tile: seed rows ... */
#define ROREG_SC2_COL_TILE 64      /* ... x columns */
typedef struct {
    const double *keys0, *keys1;   /* the two clouds' keypoints [*,3] */
    const int64_t *matches;        /* [M,2] interleaved (row in cloud 0, row in cloud 1) */
    int32_t M, S;                  /* correspondences (<= ROREG_SC2_MAX_M), seeds = min(M, max_seeds) */
    int64_t koff, boff, hoff, noff;
} roreg_sc2_task;
/* v6m, HOST function: bytes of workspace for tasks with these totals (sum of M, of M ceil(M / 64), of S M); offsets (optional, [5]): where the
 * regions start -- P f64 [total_M,3], Q f64 [total_M,3], bit rows u64 [total_words], deg int32 [total_M], N2 uint16 [total_SM] -- each followed by
 * at least 64 bytes that no kernel writes.  0 if a total is negative. */
size_t roreg_sc2_workspace(long long total_M, long long total_words, long long total_SM, size_t *offsets);
/* v6m.  Six launches whatever n_tasks (<= 65535), no host synchronisation.  max_M / max_S: the greatest M / S of the table; 3 <= K <= 64.
 * Trans_out f64 [total_S,3,4], seeds_out int32 [total_S], cons_out int32 [total_S,K] or null (the sets' members in order, -1 padded). */
int roreg_sc2_hypotheses_batch(const roreg_sc2_task *tasks_dev, int n_tasks, long long total_M, long long total_words, long long total_SM,
                               int max_M, int max_S, double tau, int K, double *Trans_out, int32_t *seeds_out, int32_t *cons_out,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6n: FPFH descriptors of a dense cloud (csrc/fpfh.hip, csrc/fpfh_math.h; additions, ROREG_ABI_VERSION stays 6) -------------------------------
 * No reference counterpart (the reference's descriptors are learned).  Semantics (tests/_fpfh_oracle.py restates them in numpy; DESIGN.md
 * section 4.23), coordinates float32 widened to float64, every operation float64 in the order of csrc/fpfh_math.h, no FMA:
 *   orientation: n_i <- -n_i iff (n0 (c0 - x0) + n1 (c1 - x1)) + n2 (c2 - x2) < 0; a zero row (invalid normal) stays zero;
 *   pair (i, j) contributes iff j != i, both normals are valid, 0 < d2 = |x_j - x_i|^2 <= radius^2 and the pair has a Darboux frame
 *   (fpfh_math::pair_feature); its three bins (fpfh_math::bin_angle, bin_linear) are counted once each: counts int32 [n,33], m = pairs counted;
 *   S_i = count_i (100 / m_i); W_i = sum_j S_j / d2_ij over j != i, 0 < d2 <= radius^2, m_j > 0; per third g of the 33 bins s_g = sum W_i[b],
 *   F_i[b] = (s_g > 0 ? (100 W_i[b]) / s_g : 0) + S_i[b]; out = (float)F_i; row i is valid iff m_i > 0, an invalid row is 33 zeros.
 * `grid` is a cloud's grid (roreg_icp_grid_build, built for any radius; the FPFH radius walks the fewest cells) and n its number of points: a
 * kernel that finds another n in the grid's descriptor writes nothing.  Every table is in ORIGINAL row order.  n == 0: no launch.  n <= 2^30.
 * v6n, HOST functions: bytes of workspace of roreg_fpfh_spfh / roreg_fpfh_features for n points (0 if n is out of range). */
size_t roreg_fpfh_spfh_workspace(int n);
size_t roreg_fpfh_features_workspace(int n);
/* v6n.  normals, out: f64 [n,4] (roreg_icp_normals' table; column 3 is copied), 32-byte aligned; viewpoint: three doubles in HOST memory. */
int roreg_fpfh_orient(const void *grid, int n, const double *normals, const double *viewpoint, double *out, void *stream);
/* v6n.  oriented: roreg_fpfh_orient's out.  counts_out int32 [n,33], m_out int32 [n].  Two launches: the normals into cell order, the walk. */
int roreg_fpfh_spfh(const void *grid, int n, const double *oriented, double radius, int32_t *counts_out, int32_t *m_out, void *workspace,
                    size_t workspace_bytes, void *stream);
/* v6n.  counts, m: roreg_fpfh_spfh's outputs.  out f32 [n,33], valid_out uint8 [n].  Two launches: S and m into cell order, the walk (its float64
 * sums run over the neighbours in ascending cell, ascending original row inside a cell). */
int roreg_fpfh_features(const void *grid, int n, const int32_t *counts, const int32_t *m, double radius, float *out, uint8_t *valid_out,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6o: mutual nearest neighbours of FPFH descriptors on the matrix cores (csrc/fpfh_match.hip; additions, ROREG_ABI_VERSION stays 6) -------
 * No reference counterpart.  Per task, with S = desc0[rows0] (m0 rows) and T = desc1[rows1] (m1 rows), width 33: nn01 / dist01 are
 * roreg_nn_search_ex(.., F = 33, squared = 0)'s answer for every row of S over T, nn10 its answer for every row of T over S, bit for bit (the
 * literal float32 formula decides among the candidates an approximate distance matrix leaves: DESIGN.md section 4.24), and the mutual pairs
 * (rows0[i], rows1[nn01[i]]) with nn10[nn01[i]] == i are written in increasing i, their number to counts_out, as roreg_mutual_matches does.
 * PRECONDITION: every selected row is finite, its squared norm 0 or in [2^-60, 2^100] (roreg_fpfh_features writes nothing else).  Rows the
 * lists do not select are never read.
 * One task (device pointers; 80 bytes).  rows0 / rows1: int64 row lists or NULL (= 0..m-1).  The offsets are the caller's running sums over the
 * tasks before this one: r0 / r1 = this task's first rows in the workspace, each side padded to ITS OWN multiple of ROREG_FPFH_MATCH_TILE
 * (side 0 first: r1 = r0 + round_up(m0), the next task's r0 = r1 + round_up(m1)); o0 of m0, o1 of m1, om of min(m0, m1). */
#define ROREG_FPFH_MATCH_WIDTH 33          /* channels */
#define ROREG_FPFH_MATCH_TILE 128          /* edge of a tile of the distance matrix */
#define ROREG_FPFH_MATCH_MAX_ROWS 1048576  /* rows per side */
#define ROREG_FPFH_MATCH_DEBUG_MAX 512     /* a task with both sides at most this long fills its debug arrays */
typedef struct {
    const float *desc0, *desc1;
    const int64_t *rows0, *rows1;
    int32_t m0, m1;
    int64_t r0, r1, o0, o1, om;
} roreg_fpfh_match_task;
/* one task's debug arrays (40 bytes; any pointer may be NULL): a f32 [m0,m1] the approximate matrix, amin0 f32 [m0] / amin1 f32 [m1] its row
 * and column minima as pass A found them, cnt0 int32 [m0] / cnt1 int32 [m1] the candidates of every row / column (the caller zeroes them) */
typedef struct {
    float *a, *amin0, *amin1;
    int32_t *cnt0, *cnt1;
} roreg_fpfh_match_debug;
/* v6o, HOST function: bytes of workspace for tasks whose padded sides sum to total_rows; offsets (optional, [5]): where the regions start --
 * gathered rows f32 [total_rows,36], squared norms f32 [total_rows], minima keys u32 [total_rows], packed keys u64 [total_rows], the sides'
 * greatest squared norms u32 [n_tasks,2] -- each followed by at least 64 bytes that no kernel writes.  0 if an argument is negative. */
size_t roreg_fpfh_match_workspace(long long total_rows, int n_tasks, size_t *offsets);
/* v6o.  Five launches whatever n_tasks (<= 32767), no host synchronisation.  max_m0 / max_m1: the greatest m0 / m1 of the table (each at most
 * ROREG_FPFH_MATCH_MAX_ROWS).  nn01_out int64 [sum m0], dist01_out f32 [sum m0], nn10_out int64 [sum m1], match_out int64 [sum min(m0,m1),2],
 * counts_out int32 [n_tasks].  A task with an empty side writes a count of 0 and nothing else.  debug_dev: NULL, or one roreg_fpfh_match_debug
 * per task in device memory (read for tasks with both sides <= ROREG_FPFH_MATCH_DEBUG_MAX only). */
int roreg_fpfh_match_batch(const roreg_fpfh_match_task *tasks_dev, int n_tasks, int max_m0, int max_m1, long long total_rows,
                           int64_t *nn01_out, float *dist01_out, int64_t *nn10_out, int64_t *match_out, int32_t *counts_out,
                           const roreg_fpfh_match_debug *debug_dev, void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6q: k nearest neighbours within a radius, from a cloud's grid (csrc/grid_knn.hip, csrc/knn_list.h; addition, ROREG_ABI_VERSION stays 6) ------
 * No reference counterpart.  Semantics (tests/_grid_knn_oracle.py restates them in numpy).  `grid` is a cloud's grid
 * (roreg_icp_grid_build, built for any radius) and n its number of points: a kernel that finds another n in the grid's descriptor writes nothing,
 * a record whose row word is out of range is skipped.  k in 1..32, radius > 0 and finite.
 *   queries == NULL (then self_rows must be NULL and m == n): the queries are the cloud's own rows; row i excludes candidate row i; the outputs
 *   are in ORIGINAL row order.
 *   queries f32 [m,3]: m finite points, anywhere (outside the grid's box too); self_rows int32 [m] or NULL: the cloud row query q excludes
 *   (-1: none).
 * Coordinates are float32 values widened to float64.  For query x and cloud row j: dx = x_j.x - x.x, dy, dz likewise (exact),
 * d2 = (dx dx + dy dy) + dz dz, no FMA.  Row j is a candidate iff it is not the excluded row and d2 <= radius * radius (one float64 product, on
 * the host); the walk visits the cells a ball of radius (1 + 1e-9) meets, as roreg_icp_normals does.  A duplicated point (d2 == 0) is a candidate:
 * exclusion is by row, never by distance.  Candidates are ordered by (d2, j) ascending: among equal d2 the lower row first.
 *   count_out int32 [m]: the number of candidates, NOT capped at k;
 *   idx_out int32 [m,k], d2_out f64 [m,k]: the first f = min(k, count) candidates in that order, then -1 / +inf;
 *   mean_dist_out f64 [m] or NULL: (...((sqrt(d2_0) + sqrt(d2_1)) + sqrt(d2_2)) ...) / f in list order, +inf when f == 0.
 * Every output is a function of + - * / sqrt and comparisons in this order: the same bytes from any grid of the cloud.  m == 0: no launch.
 * n, m <= 2^30.  One launch, no workspace, no host synchronisation. */
int roreg_grid_knn(const void *grid, int n, int k, double radius, const float *queries, const int32_t *self_rows, int m, int32_t *idx_out,
                   double *d2_out, int32_t *count_out, double *mean_dist_out, void *stream);

/* ---- v6r: DBSCAN clustering of a dense cloud, from its grid (csrc/cluster.hip; additions, ROREG_ABI_VERSION stays 6) --------------------------------
 * No reference counterpart.  Semantics (tests/_cluster_oracle.py restates them in numpy).  `grid` is a cloud's grid
 * (roreg_icp_grid_build, built for any radius) and n its number of points: a kernel that finds another n in the grid's descriptor writes nothing.
 * eps > 0 and finite, min_points >= 1.
 *   Neighbourhood.  Coordinates are float32 values widened to float64; dx = x_j.x - x_i.x, dy, dz likewise (exact), d2 = (dx dx + dy dy) + dz dz,
 *     no FMA.  Rows i and j are neighbours iff d2 <= eps * eps (one float64 product, on the host); the walk visits the cells a ball of
 *     eps (1 + 1e-9) meets, as roreg_icp_normals and roreg_grid_knn do.
 *   Core rows.  count_i = the number of rows within eps of row i, ITSELF INCLUDED (a duplicated point counts); row i is core iff
 *     count_i >= min_points (Open3D's cluster_dbscan, sklearn's DBSCAN; min_points = 1 is PCL's EuclideanClusterExtraction).
 *   Clusters.  The connected components of the graph whose vertices are the core rows and whose edges join core rows that are neighbours.
 *   Border rows.  A non-core row with at least one core neighbour belongs to the cluster of the core neighbour that is first in (d2, row)
 *     order -- to one cluster only, and the same one on every run.
 *   Noise.  Every other row: label -1.
 *   Numbering.  Clusters are numbered 0..C-1 by ascending lowest core row.
 * Outputs, in ORIGINAL row order: labels int32 [n]; core uint8 [n] (1 / 0); n_clusters int32 [1] = C; sizes int32 [n]: entries 0..C-1 the
 * number of rows (core and border) of each cluster, the rest 0.  All outputs are integers defined by comparisons: the same bytes from any grid
 * of the cloud and on every run (union-find on the core graph whose hooks only ever lower a parent word with an integer atomicMin, so a
 * component's root is its lowest core row whatever order they land in; sizes by integer atomicAdd; no floating-point atomic; no lane waits for
 * another's write).  n == 0: no launch, nothing is written.  n <= 2^30.  Eight launches, no host synchronisation.
 *
 * v6r, HOST function: bytes of workspace for n rows (0 <= n <= 2^30; 0 otherwise). */
size_t roreg_cluster_workspace(int n);
/* v6r.  The workspace needs no clearing: the call writes every word before it reads it. */
int roreg_grid_dbscan(const void *grid, int n, double eps, int min_points, int32_t *labels, uint8_t *core, int32_t *n_clusters, int32_t *sizes,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- v6s: farthest-point sampling of dense clouds (csrc/sample.hip; additions, ROREG_ABI_VERSION stays 6) -----------------------------------------
 * No reference counterpart.  Semantics (tests/_fps_oracle.py restates them in numpy), per task:
 *   Inputs.  points f32 [n,3], 0 <= n <= 2^30; k >= 0; start in [0, n) (ignored when n == 0); stop2 >= 0, the SQUARE of a stop distance, 0 = none.
 *   Arithmetic.  Coordinates are float32 values widened to float64; d2(i, j) = (dx dx + dy dy) + dz dz, no FMA.
 *   Selection.  A row with a non-finite coordinate is dead: never selected, never used.  D[i] = +inf for every live row.  Step 0 selects
 *     `start`, or the lowest live row when start is dead.  Step s >= 1 selects the live row not yet taken of greatest D, among equal D the
 *     LOWEST ROW.  After every selection c, D[i] = min(D[i], d2(i, c)) for every live row.  A taken row is excluded as such, not by its D (a
 *     cloud of duplicates yields start, then the other rows in ascending order, each at D = 0).
 *   End.  At the first of: k rows selected; no live row left that is not taken; for s >= 1, the candidate's D < stop2 (strict: D == stop2 is
 *     still selected).
 *   Outputs.  rows int32 [k] in selection order, -1 behind `count`; dist2 f64 [k]: the D of each row at the moment it was selected
 *     (dist2[0] = +inf, non-increasing), 0 behind `count`; count int32 [1].  rows[:k'] of a k-call are the rows of a k'-call.  Every output is
 *     defined by comparisons of exactly rounded float64 values: the same bytes on every run and in whatever batch the task runs.
 *   n == 0 or k == 0: count = 0 and nothing else is written.
 * One workgroup of 1024 lanes per task, persistent over the task's steps; no workgroup waits for another.  The host chooses a task's tier from n:
 *   ROREG_FPS_TIER_LDS   n <= ROREG_FPS_LDS_MAX_N: D in registers, the coordinates staged once into LDS;
 *   ROREG_FPS_TIER_REG   n <= ROREG_FPS_REG_MAX_N: D in registers, the coordinates read again every step;
 *   ROREG_FPS_TIER_MEM   any n: D in the workspace, 8 n bytes at ws_off (roreg_fps_workspace).
 * A task whose tier cannot hold its n, whose tier is none of the three, or whose workspace region does not lie inside the workspace writes
 * count = 0 and nothing else.  A lower tier's task may run in a higher tier (the same bytes). */
#define ROREG_FPS_THREADS 1024
#define ROREG_FPS_LDS_MAX_N 13312  /* 13 rows per lane: 3 x 13312 floats = 159,744 bytes of the CU's 163,840 */
#define ROREG_FPS_REG_MAX_N 32768  /* 32 rows per lane: 64 of the 128 registers a lane of a 1024-lane workgroup has */
#define ROREG_FPS_TIER_LDS 0
#define ROREG_FPS_TIER_REG 1
#define ROREG_FPS_TIER_MEM 2
typedef struct {
    const float *points;           /* [n,3] */
    int32_t *rows;                 /* [k] */
    double *dist2;                 /* [k] */
    int32_t *count;                /* [1] */
    double stop2;
    int64_t ws_off;                /* byte offset of the task's D array in the workspace, a multiple of 8 (ROREG_FPS_TIER_MEM only) */
    int32_t n, k, start, tier;
} roreg_fps_task;                  /* 64 bytes */
/* v6s, HOST function: bytes of workspace a ROREG_FPS_TIER_MEM task of n rows takes (8 n rounded up to 256; 0 for n outside 0..2^30).  The
 * caller lays the tasks' regions out one behind the other. */
size_t roreg_fps_workspace(int n);
/* v6s.  One launch whatever n_tasks (<= 2^20), no host synchronisation.  tasks_dev: n_tasks records in device memory.  The workspace needs
 * no clearing: a task writes every word of its region before it reads it.  workspace may be NULL when workspace_bytes == 0. */
int roreg_fps_batch(const roreg_fps_task *tasks_dev, int n_tasks, void *workspace, size_t workspace_bytes, void *stream);
/* v6s, the per-step launch form: ONE cloud over many workgroups, for a cloud so large that one compute unit is the bottleneck.  The same
 * definition and the same bytes as a task of roreg_fps_batch.  k + 1 launches, no host synchronisation: launch j reduces the candidates that
 * the workgroups of launch j - 1 left, writes step j - 1's outputs and updates D; nothing waits on another workgroup.  Host arguments; start in
 * [0, n) and stop2 >= 0 are checked.  n == 0 or k == 0: count = 0 (a memset on the stream) and nothing else.
 * HOST function: bytes of workspace for a cloud of n rows (D and two candidate buffers; 0 for n outside 0..2^30). */
size_t roreg_fps_steps_workspace(int n);
/* v6s.  The workspace needs no clearing. */
int roreg_fps_steps(const float *points, int n, int k, int start, double stop2, int32_t *rows, double *dist2, int32_t *count, void *workspace,
                    size_t workspace_bytes, void *stream);

/* ---- v6t: RANSAC plane segmentation of dense clouds (csrc/plane.hip; additions, ROREG_ABI_VERSION stays 6) ---------------------------------------
 * No reference counterpart.  Semantics (tests/_plane_oracle.py restates them in numpy, twice; csrc/plane_math.h holds the scalar arithmetic;
 * DESIGN.md section 4.30):
 *   Inputs.  points f32 [n,3], 0 <= n <= 2^30; dist > 0 and finite; n_hyp = H in [1, ROREG_PLANE_MAX_HYP]; max_planes = K in
 *     [0, ROREG_PLANE_MAX_PLANES]; min_inliers >= 3; seed uint64.
 *   Arithmetic.  Coordinates are float32 values widened to float64; every product and sum in the order written below, no FMA.  A row with a
 *     non-finite coordinate is dead: never drawn, never counted, label -1.
 *   Rounds r = 0 .. K-1.  The live rows are the rows not dead and not yet labelled, in ascending row order; L is their number.  A round with
 *     L < 3 ends the segmentation.
 *   Draws (integers, counter based: a function of seed, r, h, j and L alone).  mix = the splitmix64 finaliser: x += 0x9E3779B97F4A7C15,
 *     x = (x ^ x >> 30) 0xBF58476D1CE4E5B9, x = (x ^ x >> 27) 0x94D049BB133111EB, x ^ x >> 31, all mod 2^64.  base = mix(seed ^ (r << 32)),
 *     w = mix(base + 3 h + j), index = ((w >> 32) L) >> 32: slot j = 0, 1, 2 of hypothesis h is live row number `index`.  Two equal indices
 *     make the hypothesis invalid.
 *   Plane of (a, b, c).  e1 = b - a, e2 = c - a, n = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), q = (nx nx + ny ny) + nz nz.
 *     Invalid if q is 0 or not finite.  The count of an invalid hypothesis is -1.
 *   Support.  For a live row p: s = (nx (px - ax) + ny (py - ay)) + nz (pz - az); p is an inlier iff s s <= (dist dist) q (inclusive; dist dist
 *     and its product with q are each computed once).  No square root, no division: every count is an exact integer function of the input.
 *   Winner.  The valid hypothesis of greatest count, among equal counts the LOWEST h.  No valid hypothesis, or a count below min_inliers: the
 *     segmentation ends and later rounds change nothing.  Otherwise the winner's inliers get label r and leave the live set.
 *   Outputs.  labels int32 [n] (-1: on no plane); n_planes int32 [1]; counts int32 [K], 0 behind n_planes; triples int32 [K,3] original rows,
 *     -1 behind n_planes; raw f64 [K,4] = (nx, ny, nz, -((nx ax + ny ay) + nz az)), unnormalised, 0 behind n_planes.  The same bytes as the
 *     oracle's on every run.
 *   Fit (reported; decides nothing).  fit f64 [K,4]: the least-squares plane through plane r's inliers, a unit normal and an offset, the normal
 *     signed like raw's (negated when its dot product with raw's is < 0), 0 behind n_planes.  Moments of (p - a) over the inliers are summed in
 *     float64 through one fixed slot per ROREG_PLANE_TILE live rows, the slots in ascending order (no float atomics); the normal is the
 *     eigenvector of the covariance's smallest eigenvalue (icp_math.h jacobi3); the offset is -(normal . centroid).  rms f64 [K]: the root mean
 *     square of the inliers' distances normal . (p - centroid), 0 behind n_planes.
 * The scoring kernel keeps ROREG_PLANE_TILE live points per workgroup of ROREG_PLANE_THREADS lanes in registers and walks the hypotheses in
 * chunks of ROREG_PLANE_HYP_CHUNK records in LDS. */
#define ROREG_PLANE_THREADS 256
#define ROREG_PLANE_TILE 1024
#define ROREG_PLANE_HYP_CHUNK 128
#define ROREG_PLANE_MAX_HYP 65536
#define ROREG_PLANE_MAX_PLANES 64
/* v6t, HOST function: bytes of workspace for n rows and n_hyp hypotheses (0 for n outside 0..2^30 or n_hyp outside 1..ROREG_PLANE_MAX_HYP). */
size_t roreg_plane_workspace(int n, int n_hyp);
/* v6t.  Every round is enqueued with no host synchronisation; whether a round runs is read by its launches from device words that earlier
 * launches wrote (n_planes[0] == r and the live count >= 3), so nothing waits on another workgroup.  The workspace needs no clearing and may be
 * NULL when n < 3 or max_planes == 0. */
int roreg_plane_segment(const float *points, int n, double dist, int n_hyp, int max_planes, int min_inliers, uint64_t seed, int32_t *labels,
                        int32_t *n_planes, int32_t *counts, int32_t *triples, double *raw, double *fit, double *rms, void *workspace,
                        size_t workspace_bytes, void *stream);
/* v6t.  The scoring pass alone over caller-given triples int32 [n_hyp,3] of original rows, every non-dead row live: counts_out int32 [n_hyp].
 * A triple with a repeated row, a row outside [0, n), a dead row or a degenerate plane gives -1.  0 <= n_hyp <= ROREG_PLANE_MAX_HYP. */
int roreg_plane_score(const float *points, int n, const int32_t *triples, int n_hyp, double dist, int32_t *counts_out, void *stream);

/* Optional kernel timing for bench.py's measured rooflines (no reference counterpart: the reference has no profiler hooks).
 * While enabled, the library brackets selected launches with HIP events recorded ON THE LAUNCH STREAM; roreg_profile_read synchronises
 * on them and returns the summed duration and the number of brackets of a slot:
 *   0 = the two mm_tile_kernel passes of roreg_mutual_match_batch (the descriptor distance matrix on the matrix cores),
 *   1 = ransac_score_batch_kernel of roreg_ransac_batch, 2 = des2r_batch_kernel of roreg_lt_prepare_batch, 3 = roreg_ft_nonlin,
 *   4 = the `iters` Sinkhorn iterations of roreg_sinkhorn_batch (one fused pass over every pair's coupling matrix + column merge each),
 *   5 = roreg_topk_dot (slice search + merge), 6 = the nearest-neighbour search launches of roreg_icp_batch (v6c), roreg_icp_plane_batch and roreg_icp_gicp_batch,
 *   7 = the second pass of a normal-based method: icp_plane_kernel of roreg_icp_plane_batch (v6d), icp_gicp_kernel of roreg_icp_gicp_batch (v6i),
 *       and their weighted forms of roreg_icp_plane_robust_batch / roreg_icp_gicp_robust_batch (v6p; slot 6 covers their searches too),
 *   8 = the solve launches (pg_solve_kernel, one per round) of roreg_pg_optimize_batch (v6h),
 *   9 / 10 = pass A / pass B (fm_tile_kernel) of roreg_fpfh_match_batch (v6o).
 * roreg_profile_enable(1) clears earlier records; (0) stops recording. */
int roreg_profile_enable(int on);
int roreg_profile_read(int slot, double *total_ms, int *launches);

#ifdef __cplusplus
}
#endif
#endif /* ROREG_HIP_H */
