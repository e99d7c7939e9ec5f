"""The C-ABI of libroreg_hip.so as data: ctypes prototypes (name -> (restype, argtypes), mirroring include/roreg_hip.h declaration by
declaration -- tests/test_host_logic.py checks the two against each other and against the exported symbols) and the numpy layouts of the task
structs the batched entry points take.  roreg_amd/hip.py binds them."""
import ctypes
from ctypes import c_int, c_void_p, c_size_t, c_double, c_float, c_char_p, c_uint64

import numpy as np

ABI_VERSION = 6          # == ROREG_ABI_VERSION of include/roreg_hip.h; hip.lib() refuses a library that reports another one

_P = c_void_p
PROTOTYPES = {
    'roreg_abi_version': (c_int, []),
    'roreg_last_error': (c_char_p, []),
    'roreg_set_group_tables': (c_int, [_P, _P, _P]),
    'roreg_group_conv_packed_size': (c_size_t, [c_int, c_int, c_int]),
    'roreg_group_conv_pack_weights': (c_int, [_P, c_int, c_int, c_int, _P]),
    'roreg_group_conv_workspace_size': (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'roreg_group_conv': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    'roreg_group_conv_split': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'roreg_group_conv_f16x2': (c_int, [_P, _P, c_int, _P, _P, _P, c_float, c_float, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'roreg_group_conv_f16x2_packed': (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'roreg_dense_f16x2': (c_int, [_P, _P, c_int, _P, _P, _P, c_float, c_float, _P, _P, c_int, _P, _P, c_int, c_int, c_int, _P]),
    'roreg_dense_split': (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, c_int, c_int, c_int, _P]),
    'roreg_gf_finalize': (c_int, [_P, _P, c_int, _P, c_int, _P]),
    'roreg_det_score': (c_int, [_P, _P, c_int, _P]),
    'roreg_inv_descriptor': (c_int, [_P, c_int, _P, c_int, _P]),
    'roreg_nn_search': (c_int, [_P, _P, c_int, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    'roreg_nn_search_ex': (c_int, [_P, _P, c_int, _P, _P, c_int, c_int, c_int, _P, _P, _P, _P]),
    'roreg_pdist': (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P]),
    'roreg_knn_search_workspace': (c_size_t, [c_int, c_int]),
    'roreg_knn_search': (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    'roreg_knn_search_ex': (c_int, [_P, c_int, _P, c_int, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    'roreg_knn_search_seg_workspace': (c_size_t, [ctypes.c_longlong, c_int, c_int, c_int]),
    'roreg_knn_search_seg': (c_int, [_P, _P, _P, _P, c_int, ctypes.c_longlong, c_int, c_int, c_int, c_int, _P, _P, c_size_t, _P]),
    'roreg_mutual_matches': (c_int, [_P, _P, c_int, c_int, _P, _P, _P, _P, _P]),
    'roreg_mutual_match_batch_workspace': (c_size_t, [c_int, c_int]),
    'roreg_mutual_match_batch': (c_int, [_P, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    'roreg_des2r': (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P]),
    'roreg_set_des2r_tables': (c_int, [c_int, _P, _P, _P, _P]),
    'roreg_group_corr_irrep': (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P]),
    'roreg_group_corr_mfma': (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P]),
    'roreg_des2r_irrep': (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, _P, _P]),
    'roreg_des2r_recheck_count': (c_int, [c_int, _P]),
    'roreg_feat_coefs': (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P]),
    'roreg_et_gather': (c_int, [_P, _P, _P, _P, c_int, _P, _P, _P, c_int, _P, _P]),
    'roreg_quat_to_trans': (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _P, _P]),
    'roreg_ransac_score': (c_int, [_P, _P, _P, c_int, c_int, _P, _P, c_int, c_double, _P, _P, _P, _P]),
    'roreg_refine': (c_int, [_P, _P, _P, c_int, c_int, _P, c_int, _P, _P, _P, c_double, _P, _P, _P]),
    'roreg_lt_prepare_batch': (c_int, [_P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P]),
    'roreg_lt_finish_batch': (c_int, [_P, c_int, c_int, _P, _P, _P, _P]),
    'roreg_role_max': (c_int, [_P, _P, c_int, _P, _P, _P, c_int, _P]),
    'roreg_row_bound_roles': (c_int, [_P, c_int, _P, _P, _P, _P, c_int, _P]),
    'roreg_inv_descriptor_roles': (c_int, [_P, c_int, _P, _P, _P, _P, c_int, _P]),
    'roreg_lt_prepare_rows': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P]),
    'roreg_ransac_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong, c_int]),
    'roreg_ransac_batch': (c_int, [_P, c_int, ctypes.c_longlong, c_int, c_int, c_double, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_refine_batch': (c_int, [_P, _P, c_int, ctypes.c_longlong, _P, ctypes.c_double, c_int, _P, _P, _P, _P]),
    'roreg_yohoc_draw': (c_int, [_P, ctypes.c_longlong, _P, _P, c_int, c_int, _P, _P, _P, _P]),
    'roreg_gather_rows_batch': (c_int, [_P, c_int, c_int, c_int, _P]),
    'roreg_gather_rows_f64': (c_int, [_P, _P, c_int, c_int, _P, _P]),
    'roreg_group_corr': (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, _P]),
    'roreg_topk_dot_workspace_size': (c_size_t, [c_int, c_int, c_int]),
    'roreg_topk_dot': (c_int, [_P, c_int, _P, c_int, c_int, _P, _P, _P, c_size_t, _P, _P, c_int, c_int, c_int, _P]),
    'roreg_context_colmax': (c_int, [_P, c_int, _P, c_int, c_int, _P, _P, _P]),
    'roreg_sinkhorn_batch_workspace_size': (c_size_t, [c_int, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong]),
    'roreg_sinkhorn_batch_consts': (c_int, [_P, _P, c_int, _P]),
    'roreg_sinkhorn_batch': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_sinkhorn_batch2_workspace_size': (c_size_t, [c_int, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong]),
    'roreg_sinkhorn_batch2': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, c_int, _P]),
    'roreg_sinkhorn_batch3_workspace_size': (c_size_t, [c_int, c_int, c_int, ctypes.c_longlong, ctypes.c_longlong, c_int, c_int]),
    'roreg_sinkhorn_batch3': (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_float, c_int, _P, _P, _P, _P, _P, c_size_t, c_int, _P, _P]),
    'roreg_write_files': (c_int, [_P, _P, _P, _P, _P, c_int, c_int]),
    'roreg_yohoc_draw_many': (c_int, [_P, c_int, _P, _P, c_int, c_int, _P, _P, _P, c_int]),
    'roreg_mlp_head_workspace': (c_size_t, [c_int, c_int, c_int]),
    'roreg_mlp_head': (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P, _P, _P, _P, _P, c_int, c_int, c_float, _P, _P, _P]),
    'roreg_sinkhorn_early_exit': (c_int, [c_int]),
    'roreg_sinkhorn_iteration_stats': (c_int, [_P, _P, c_int, _P]),
    'roreg_linear': (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P]),
    'roreg_linear_mfma': (c_int, [_P, c_int, c_int, _P, _P, c_int, _P, _P]),
    'roreg_linear_path': (c_int, [c_int]),
    'roreg_linear_cat3': (c_int, [_P, _P, _P, _P, c_int, c_int, _P, _P, c_int, _P, _P]),
    'roreg_gemm_persistent': (c_int, [c_int]),
    'roreg_gemm_thin': (c_int, [c_int]),
    'roreg_gf_finish_route': (c_int, [c_int]),
    'roreg_irrep_gemm_f16x2_rows': (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    'roreg_gf_finish': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    'roreg_instnorm_stats': (c_int, [_P, c_int, c_int, c_float, _P, _P, _P, c_int, c_int, _P]),
    'roreg_mlp_tail': (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    'roreg_mlp_tail_mfma': (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    'roreg_knn_attention': (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    'roreg_rm_elementwise': (c_int, [c_int, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    'roreg_sinkhorn_workspace_size': (c_size_t, [c_int, c_int]),
    'roreg_sinkhorn': (c_int, [_P, c_int, _P, c_int, c_float, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_grid_size': (c_size_t, [_P, _P, c_int, c_double, _P, _P]),
    'roreg_icp_grid_build': (c_int, [_P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, c_int, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_normals': (c_int, [_P, c_double, c_int, _P, _P]),
    'roreg_icp_plane_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_plane_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, c_int, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_gicp_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_gicp_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, c_int, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_plane_robust_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_plane_robust_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, c_int, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_gicp_robust_batch_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_gicp_robust_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, c_int, c_double, c_double, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_icp_eval_workspace': (c_size_t, [c_int, ctypes.c_longlong]),
    'roreg_icp_eval_batch': (c_int, [_P, c_int, _P, c_int, ctypes.c_longlong, c_double, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_voxel_workspace': (c_size_t, [c_int]),
    'roreg_voxel_downsample': (c_int, [_P, c_int, c_double, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_pg_workspace': (c_size_t, [_P, c_int]),
    'roreg_pg_optimize_batch': (c_int, [_P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_sparse_map_workspace': (c_size_t, [c_int]),
    'roreg_sparse_stride_map': (c_int, [_P, c_int, c_int, _P, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_sparse_kernel_map': (c_int, [_P, c_int, _P, c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    'roreg_sparse_conv': (c_int, [_P, c_int, c_int, c_int, _P, c_int, c_int, _P, c_int, _P, _P, _P, c_int, c_int, _P, c_int, _P]),
    'roreg_sparse_l2norm': (c_int, [_P, c_int, c_int, _P, _P]),
    'roreg_group_feature_assemble': (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, c_int, _P, c_int, _P, _P]),
    'roreg_sc2_workspace': (c_size_t, [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, _P]),
    'roreg_sc2_hypotheses_batch': (c_int, [_P, c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_longlong, c_int, c_int, c_double, c_int, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_fpfh_spfh_workspace': (c_size_t, [c_int]),
    'roreg_fpfh_features_workspace': (c_size_t, [c_int]),
    'roreg_fpfh_orient': (c_int, [_P, c_int, _P, _P, _P, _P]),
    'roreg_fpfh_spfh': (c_int, [_P, c_int, _P, c_double, _P, _P, _P, c_size_t, _P]),
    'roreg_fpfh_features': (c_int, [_P, c_int, _P, _P, c_double, _P, _P, _P, c_size_t, _P]),
    'roreg_fpfh_match_workspace': (c_size_t, [ctypes.c_longlong, c_int, _P]),
    'roreg_fpfh_match_batch': (c_int, [_P, c_int, c_int, c_int, ctypes.c_longlong, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_grid_knn': (c_int, [_P, c_int, c_int, c_double, _P, _P, c_int, _P, _P, _P, _P, _P]),
    'roreg_cluster_workspace': (c_size_t, [c_int]),
    'roreg_grid_dbscan': (c_int, [_P, c_int, c_double, c_int, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_fps_workspace': (c_size_t, [c_int]),
    'roreg_fps_batch': (c_int, [_P, c_int, _P, c_size_t, _P]),
    'roreg_fps_steps_workspace': (c_size_t, [c_int]),
    'roreg_fps_steps': (c_int, [_P, c_int, c_int, c_int, c_double, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_plane_workspace': (c_size_t, [c_int, c_int]),
    'roreg_plane_segment': (c_int, [_P, c_int, c_double, c_int, c_int, c_int, c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    'roreg_plane_score': (c_int, [_P, c_int, _P, c_int, c_double, _P, _P]),
    'roreg_profile_enable': (c_int, [c_int]),
    'roreg_profile_read': (c_int, [c_int, _P, _P]),
    'roreg_set_fourier_tables': (c_int, [_P]),
    'roreg_mt_shuffle_prefix': (c_int, [_P, c_int, _P, c_int, c_int, _P, c_int]),
    'roreg_mt_stream_shuffle_prefix': (c_int, [_P, _P, _P, c_int, c_int, _P]),
    'roreg_irrep_gemm_tiles': (c_size_t, [c_int, c_int, _P]),
    'roreg_irrep_gemm_tiles_m': (c_size_t, [c_int, c_int, c_int, _P]),
    'roreg_irrep_gemm': (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, c_int, _P]),
    'roreg_irrep_gemm_split': (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P, c_int, _P]),
    'roreg_irrep_gemm_f16x2': (c_int, [_P, _P, _P, _P, _P, c_int, _P, _P, _P, c_int, c_int, c_int, _P, c_int, c_int, c_int, _P]),
    'roreg_row_bound': (c_int, [_P, c_int, _P, _P, _P, c_int, c_int, _P]),
    'roreg_ft_nonlin': (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, c_int, c_int, _P]),
    'roreg_ft_nonlin_packed': (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, c_int, _P]),
    'roreg_ft_nonlin_gathered': (c_int, [_P, _P, c_int, _P, _P, _P, c_int, _P, c_int, _P]),
}


_RANSAC_TASK = np.dtype([('keys0', np.uint64), ('keys1', np.uint64), ('matches', np.uint64), ('w', np.uint64), ('Trans', np.uint64),
                         ('hyp_rows', np.uint64), ('M', np.int32), ('H', np.int32), ('koff', np.int64)])

_MATCH_TASK = np.dtype([('desc0', np.uint64), ('desc1', np.uint64), ('rows0', np.uint64), ('rows1', np.uint64), ('m0', np.int32), ('m1', np.int32)])

_GATHER_TASK = np.dtype([('src', np.uint64), ('rows', np.uint64), ('dst', np.uint64), ('n', np.int32), ('pad', np.int32)])

_LT_TASK = np.dtype([('before0', np.uint64), ('before1', np.uint64), ('after0', np.uint64), ('after1', np.uint64), ('keys0', np.uint64),
                     ('keys1', np.uint64), ('matches', np.uint64), ('sel', np.uint64), ('n', np.int32), ('pad', np.int32), ('off', np.int64),
                     ('coef0', np.uint64), ('coef1', np.uint64)])

# v6c (dense ICP): the 64-byte grid descriptor roreg_icp_grid_size fills and one pair of roreg_icp_batch
_ICP_GRID_DESC = np.dtype([('origin', np.float64, 3), ('edge', np.float64), ('dims', np.int32, 3), ('n', np.int32), ('cells', np.int64),
                           ('reserved', np.int64)])

_ICP_TASK = np.dtype([('tgt_grid', np.uint64), ('src_grid', np.uint64), ('T0', np.uint64), ('n_src', np.int32), ('slot0', np.int32)])

# v6d (point-to-plane ICP): one pair of roreg_icp_plane_batch
_ICP_PLANE_TASK = np.dtype([('tgt_grid', np.uint64), ('src_grid', np.uint64), ('tgt_normals', np.uint64), ('T0', np.uint64), ('n_src', np.int32),
                            ('slot0', np.int32)])

# v6i (plane-to-plane ICP): one pair of roreg_icp_gicp_batch
_ICP_GICP_TASK = np.dtype([('tgt_grid', np.uint64), ('src_grid', np.uint64), ('tgt_normals', np.uint64), ('src_normals', np.uint64), ('T0', np.uint64),
                           ('epsilon', np.float64), ('n_src', np.int32), ('slot0', np.int32)])

# v6p (robust losses): the plane and gicp records followed by the loss's scale and kind (roreg_icp_loss)
_ICP_LOSS = {'huber': 1, 'cauchy': 2, 'gm': 3, 'tukey': 4}
_ICP_PLANE_ROBUST_TASK = np.dtype(_ICP_PLANE_TASK.descr + [('scale', np.float64), ('loss', np.int32), ('reserved', np.int32)])
_ICP_GICP_ROBUST_TASK = np.dtype(_ICP_GICP_TASK.descr + [('scale', np.float64), ('loss', np.int32), ('reserved', np.int32)])
assert _ICP_PLANE_ROBUST_TASK.itemsize == 56 and _ICP_GICP_ROBUST_TASK.itemsize == 72

# v6h (pose-graph optimisation): one graph of roreg_pg_optimize_batch
_PG_GRAPH = np.dtype([('node0', np.int32), ('n_nodes', np.int32), ('edge0', np.int32), ('n_edges', np.int32), ('act0', np.int32), ('n_act', np.int32),
                      ('anchor', np.int32), ('reserved0', np.int32), ('h0', np.int64), ('tau', np.float64), ('lambda0', np.float64),
                      ('tol_t', np.float64), ('tol_rot', np.float64), ('tol_cost', np.float64), ('reserved1', np.float64)])

# v6m (spatial-compatibility hypotheses): one pair of roreg_sc2_hypotheses_batch
_SC2_TASK = np.dtype([('keys0', np.uint64), ('keys1', np.uint64), ('matches', np.uint64), ('M', np.int32), ('S', np.int32), ('koff', np.int64),
                      ('boff', np.int64), ('hoff', np.int64), ('noff', np.int64)])

# v6o (FPFH matcher): one task of roreg_fpfh_match_batch and its debug arrays
_FPFH_MATCH_TASK = np.dtype([('desc0', np.uint64), ('desc1', np.uint64), ('rows0', np.uint64), ('rows1', np.uint64), ('m0', np.int32), ('m1', np.int32),
                             ('r0', np.int64), ('r1', np.int64), ('o0', np.int64), ('o1', np.int64), ('om', np.int64)])
_FPFH_MATCH_DEBUG = np.dtype([('a', np.uint64), ('amin0', np.uint64), ('amin1', np.uint64), ('cnt0', np.uint64), ('cnt1', np.uint64)])

# v6s (farthest-point sampling): one cloud of roreg_fps_batch
_FPS_TASK = np.dtype([('points', np.uint64), ('rows', np.uint64), ('dist2', np.uint64), ('count', np.uint64), ('stop2', np.float64), ('ws_off', np.int64),
                      ('n', np.int32), ('k', np.int32), ('start', np.int32), ('tier', np.int32)])
assert _FPS_TASK.itemsize == 64
