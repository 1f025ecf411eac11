"""The pointer-alignment contract of include/vslam_amd.h ("Alignment of device pointers"), as data.

One row per pointer argument of every entry point: (entry point, argument, requirement).  The requirement is the number of
bytes the address must be a multiple of (VSLAM_ERR_INVALID otherwise, vslam_last_error names the argument, nothing is queued),
ANY = 0 for a device pointer that is accepted at any address (the kernels behind it use byte accesses, memcpy-style loads or a
dispatch arm made for a misaligned base), or HOST for a pointer that is not device memory at all (handles, host arrays,
out-parameters, host structs).  A member of a host struct that holds a device pointer is written `struct->member`.

A kind of array has one requirement wherever it appears, the widest access any entry point makes through it, because the
output of one entry point is the input of the next: descriptors, k-NN rows, homogeneous points 16 (uint4 / int4 / float4);
keypoints, index pairs, queries and f64 arrays 8 (float2 / int2 / double); other int32 / float arrays 4, their element's own
alignment; image planes, colours, the inlier mask and the rBRIEF pattern any address.

tests/test_alignment_contract.py holds this table to the header (no argument without a row, no row without an argument);
tests/test_gpu_alignment.py generates its cases from it.
"""
HOST = "host"
ANY = 0

_BY_ENTRY = {
    "vslam_ctx_create": {"out": HOST},
    "vslam_ctx_destroy": {"ctx": HOST},
    "vslam_ctx_make_current": {"ctx": HOST},
    "vslam_ctx_set_stream": {"ctx": HOST, "hip_stream": HOST},
    "vslam_ctx_synchronize": {"ctx": HOST},
    "vslam_ctx_wait": {"ctx": HOST},
    "vslam_last_error": {"ctx": HOST},
    "vslam_corner_stats": {"ctx": HOST, "h_stats": HOST},
    "vslam_ctx_workspace_bytes": {"ctx": HOST, "bytes_out": HOST},
    "vslam_ctx_workspace_fill": {"ctx": HOST},
    "vslam_ctx_workspace_slots": {"ctx": HOST, "buf": HOST, "needed": HOST},
    "vslam_ctx_set_option": {"ctx": HOST},
    "vslam_dev_alloc": {"ctx": HOST, "d_out": HOST},
    "vslam_dev_free": {"ctx": HOST, "d_ptr": ANY},
    "vslam_copy_h2d": {"ctx": HOST, "d_dst": ANY, "h_src": HOST},
    "vslam_copy_d2h": {"ctx": HOST, "h_dst": HOST, "d_src": ANY},
    "vslam_host_alloc": {"ctx": HOST, "h_out": HOST},
    "vslam_host_free": {"ctx": HOST, "h_ptr": HOST},
    "vslam_upload_async": {"ctx": HOST, "d_dst": ANY, "h_src": HOST},
    "vslam_upload_fence": {"ctx": HOST},
    "vslam_upload_wait": {"ctx": HOST},
    "vslam_download_async": {"ctx": HOST, "h_dst": HOST, "d_src": ANY},
    "vslam_prof_enable": {"ctx": HOST},
    "vslam_prof_reset": {"ctx": HOST},
    "vslam_prof_count": {"ctx": HOST},
    "vslam_prof_get": {"ctx": HOST, "name": HOST, "total_ms": HOST, "launches": HOST},
    "vslam_debug_stream_copy": {"ctx": HOST, "d_src": 16, "d_dst": 16},
    "vslam_debug_valu_calib": {"ctx": HOST},
    "vslam_match_knn2_ratio": {"ctx": HOST, "d_desc1": 16, "d_n1": 4, "d_desc2": 16, "d_n2": 4, "d_pairs": 8, "d_m": 4, "d_knn": 16},
    "vslam_ransac_sets": {"ctx": HOST, "d_seeds": 4, "d_m": 4, "d_sets": 4, "d_draw_scratch": 4},
    "vslam_ransac_fundamental": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_pairs": 8, "d_m": 4, "d_sets": 4, "d_F": 4, "d_mask": ANY, "d_best": 4,
        "d_matches": 8, "d_hypF": 4, "d_hyp_count": 4, "d_hyp_sum": 4},
    "vslam_ransac_solve": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_pairs": 8, "d_m": 4, "d_sets": 4, "d_hypF": 4},
    "vslam_ransac_evaluate": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_pairs": 8, "d_m": 4, "d_hypF": 4, "d_F": 4, "d_mask": ANY, "d_best": 4,
        "d_matches": 8, "d_hyp_count": 4, "d_hyp_sum": 4},
    "vslam_refit_fundamental": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_matches": 8, "d_best": 4, "d_F_in": 4, "d_F_out": 4, "d_stats": 8},
    "vslam_refine_pairs": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_matches": 8, "d_best": 4, "h_K": HOST, "d_R": 4, "d_t": 4, "d_c2": 4,
        "d_points4d": 16, "d_stats": 8},
    "vslam_kdtree_build": {"ctx": HOST, "d_xy": 8, "d_n": 4, "d_nodes": 4},
    "vslam_kdtree_radius": {"ctx": HOST, "d_nodes": 4, "d_xy": 8, "d_n": 4, "d_queries": 8, "d_nq": 4, "d_hits": 4, "d_counts": 4},
    "vslam_kdtree_nearest": {"ctx": HOST, "d_nodes": 4, "d_xy": 8, "d_n": 4, "d_queries": 8, "d_nq": 4, "d_best_idx": 4},
    "vslam_kdtree_cell_table": {"ctx": HOST, "d_nodes": 4, "d_xy": 8, "d_n": 4, "d_table": 4, "d_ok": 4},
    "vslam_extract_features": {"ctx": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_xy": 8, "d_desc": 16, "d_nodes": 4, "d_n": 4,
        "d_n_detected": 4},
    "vslam_extract_features_grid": {"ctx": HOST, "d_bgr": ANY, "d_pattern": ANY, "d_xy": 8, "d_desc": 16, "d_angle_octave": 4, "d_n": 4},
    "vslam_bgr2gray": {"ctx": HOST, "d_bgr": ANY, "d_gray": ANY},
    "vslam_min_eigen": {"ctx": HOST, "d_gray": ANY, "d_eig": 4},
    "vslam_good_features": {"ctx": HOST, "d_gray": ANY, "d_xy": 8, "d_n": 4},
    "vslam_gaussian7": {"ctx": HOST, "d_gray": ANY, "d_out": ANY},
    "vslam_orb_describe": {"ctx": HOST, "d_blurred": ANY, "d_xy_in": 8, "d_n_in": 4, "d_pattern": ANY, "d_xy_out": 8, "d_desc": 16, "d_n_out":
        4},
    "vslam_extract_Rt": {"ctx": HOST, "d_F": 4, "d_best": 4, "h_K": HOST, "d_R": 4, "d_t": 4, "d_c2": 4},
    "vslam_triangulate": {"ctx": HOST, "d_xy1": 8, "d_xy2": 8, "d_matches": 8, "d_best": 4, "h_K": HOST, "d_c2": 4, "d_points4d": 16},
    "vslam_triangulate_points": {"ctx": HOST, "d_p1": 8, "d_p2": 8, "h_c1": HOST, "h_c2": HOST, "d_points4d": 16},
    "vslam_reprojection_filter": {"ctx": HOST, "d_points4d": 16, "d_xy1": 8, "d_xy2": 8, "d_matches": 8, "d_best": 4, "h_K": HOST, "d_c2": 4,
        "d_map_point_ids": 4, "d_inlier_idx": 4, "d_n_inliers": 4, "d_error": 8},
    "vslam_associate_map_points": {"ctx": HOST, "d_map_points": 16, "d_n_map": 4, "d_c2": 4, "d_nodes": 4, "d_xy": 8, "d_desc": 16, "d_n": 4,
        "d_obs_offsets": 4, "d_obs_desc": 16, "d_map_point_ids": 4, "d_claim": 4},
    "vslam_map_create": {"ctx": HOST, "out": HOST},
    "vslam_map_destroy": {"map": HOST},
    "vslam_map_reset": {"ctx": HOST, "map": HOST},
    "vslam_map_step": {"ctx": HOST, "map": HOST, "d_xy_last": 8, "d_desc_last": 16, "d_n_last": 4, "d_xy_cur": 8, "d_desc_cur": 16,
        "d_nodes_cur": 4, "d_n_cur": 4, "d_matches": 8, "d_best": 4, "d_F": 4, "d_bgr_cur": ANY, "h_K": HOST},
    "vslam_map_view": {"map": HOST, "out": HOST},
    "vslam_map_observations": {"ctx": HOST, "map": HOST, "d_offsets": 4, "d_frame_ids": 4, "d_point_ids": 4},
    "vslam_track_sequences": {"ctx": HOST, "map": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "h_K": HOST, "d_xy":
        8, "d_desc": 16, "d_nodes": 4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4},
    "vslam_view_default": {"out": HOST},
    "vslam_view_look_at": {"eye": HOST, "target": HOST, "up": HOST, "mv_out": HOST},
    "vslam_render_points": {"ctx": HOST, "d_points": 16, "d_colors": ANY, "d_sizes": 4, "d_pose": 4, "h_view": HOST, "d_bgr_out": ANY,
        "d_depth_out": 4},
    "vslam_map_render": {"ctx": HOST, "map": HOST, "h_view": HOST, "d_bgr_out": ANY, "d_depth_out": 4},
    "vslam_world_create": {"ctx": HOST, "out": HOST},
    "vslam_world_destroy": {"world": HOST},
    "vslam_world_reset": {"ctx": HOST, "world": HOST},
    "vslam_world_step": {"ctx": HOST, "world": HOST, "d_matches": 8, "d_best": 4, "d_points4d": 16, "d_R": 4, "d_t": 4, "d_n_last": 4,
        "d_n_cur": 4},
    "vslam_world_lift": {"ctx": HOST, "world": HOST, "d_points": 16, "d_lo": 4, "d_hi": 4, "d_out": 16},
    "vslam_world_view": {"world": HOST, "out": HOST},
    "vslam_map_attach_world": {"map": HOST, "world": HOST},
    "vslam_world_render": {"ctx": HOST, "world": HOST, "map": HOST, "h_view": HOST, "d_bgr_out": ANY, "d_depth_out": 4},
    "vslam_match_features": {"ctx": HOST, "d_xy1": 8, "d_desc1": 16, "d_n1": 4, "d_xy2": 8, "d_desc2": 16, "d_n2": 4, "d_seeds": 4, "d_matches": 8,
        "d_best": 4, "d_F": 4, "d_prelim_m": 4},
    "vslam_frontend_pairs": {"ctx": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4},
    "vslam_frontend_pairs_pose": {"ctx": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4, "h_K": HOST, "d_map_point_ids": 4, "pose": HOST, "pose->d_R": 4,
        "pose->d_t": 4, "pose->d_c2": 4, "pose->d_points4d": 16, "pose->d_inlier_idx": 4, "pose->d_n_inliers": 4,
        "pose->d_error": 8},
    "vslam_pack_records": {"ctx": HOST, "d_F": 4, "d_best": 4, "d_matches": 8, "d_records": 4},
    "vslam_frontend_sequence": {"ctx": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4},
    "vslam_pipeline_create": {"out": HOST},
    "vslam_pipeline_destroy": {"p": HOST},
    "vslam_pipeline_size": {"p": HOST},
    "vslam_pipeline_ctx": {"p": HOST},
    "vslam_pipeline_last_error": {"p": HOST},
    "vslam_pipeline_set_option": {"p": HOST},
    "vslam_pipeline_acquire": {"p": HOST, "ctx_out": HOST, "ticket_out": HOST},
    "vslam_pipeline_commit": {"p": HOST},
    "vslam_pipeline_submit_pairs": {"p": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4, "d_records": 4, "ticket_out": HOST},
    "vslam_pipeline_submit_pairs_pose": {"p": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4, "h_K": HOST, "d_map_point_ids": 4, "pose": HOST, "pose->d_R": 4,
        "pose->d_t": 4, "pose->d_c2": 4, "pose->d_points4d": 16, "pose->d_inlier_idx": 4, "pose->d_n_inliers": 4,
        "pose->d_error": 8, "d_records": 4, "ticket_out": HOST},
    "vslam_pipeline_submit_sequence": {"p": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "d_seeds": 4, "d_xy": 8, "d_desc": 16, "d_nodes":
        4, "d_n": 4, "d_matches": 8, "d_best": 4, "d_F": 4, "d_records": 4, "ticket_out": HOST},
    "vslam_pipeline_poll": {"p": HOST},
    "vslam_pipeline_wait": {"p": HOST},
    "vslam_pipeline_drain": {"p": HOST},
    "vslam_pipeline_batches_redone": {"p": HOST},
    "vslam_shard_range": {"lo": HOST, "hi": HOST},
    "vslam_multi_create": {"devices": HOST, "out": HOST},
    "vslam_multi_destroy": {"m": HOST},
    "vslam_multi_size": {"m": HOST},
    "vslam_multi_ctx": {"m": HOST},
    "vslam_multi_last_error": {"m": HOST},
    "vslam_multi_frontend_pairs": {"m": HOST, "h_bgr_last": HOST, "h_bgr_cur": HOST, "params": HOST, "params->d_pattern": ANY, "h_pattern": HOST,
        "h_records": HOST, "h_n_keypoints": HOST},
    "vslam_multi_frontend_pairs_resident": {"m": HOST, "d_bgr": ANY, "params": HOST, "params->d_pattern": ANY, "h_pattern": HOST, "h_records": HOST,
        "h_n_keypoints": HOST},
    "vslam_comm_unique_id": {"id_out": HOST},
    "vslam_comm_create": {"ctx": HOST, "id": HOST, "out": HOST},
    "vslam_comm_destroy": {"comm": HOST},
    "vslam_gather_records": {"ctx": HOST, "comm": HOST, "d_records": 4, "d_all": 4},
    "vslam_comm_info": {"comm": HOST, "world_out": HOST, "rank_out": HOST},
    "vslam_gather_records_v": {"ctx": HOST, "comm": HOST, "d_records": 4, "h_words": HOST, "d_all": 4},
}

# (entry point, argument, required bytes | ANY | HOST)
CONTRACT = [(entry, arg, req) for entry, args in _BY_ENTRY.items() for arg, req in args.items()]


def requirement(entry, arg):
    return _BY_ENTRY[entry][arg]
