"""ctypes binding of libmpe_hip.so (include/mpe.h).

The HIP library is the product: there is no CPU fallback.  Importing this module works
anywhere (so that host-side logic can be tested without a GPU); *using* it without the
built library raises immediately.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libmpe_hip.so')
if os.environ.get('MPE_LIB_VARIANT'):      # diagnostics: an experiment build beside the product library (csrc/Makefile `exp`)
    LIB_PATH = os.path.join(_HERE, 'libmpe_hip_%s.so' % os.environ['MPE_LIB_VARIANT'])

# HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  The engine's pipelines keep 3-4 streams busy
# (parse / copy / matching / 3D) beside whatever the application has; two of them on one queue serialise (pipeline.py:
# _make_json_streams has the measurement), so a process that streams JSON or pipelines its copies should run with
# GPU_MAX_HW_QUEUES=8 -- set before HIP initialises.  A library does not rewrite its host's environment on import: since round 5
# this is OPT-IN (MPE_SET_HW_QUEUES=1 makes the import set it when it is unset); bench.py sets the variable itself.
if os.environ.get('MPE_SET_HW_QUEUES', '0') == '1':
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

MPE_MAX_CAMERAS = 32
MPE_MAX_JOINTS = 32
MPE_ERR_UNSUPPORTED = -6

c_f32p = C.POINTER(C.c_float)
c_f64p = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int32)
c_u32p = C.POINTER(C.c_uint32)
c_u8p = C.POINTER(C.c_uint8)


class MpeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libmpe_hip error %d: %s' % (code, msg))
        self.code = code


class mpe_config(C.Structure):
    _fields_ = [
        ('n_cameras', C.c_int32), ('n_joints', C.c_int32), ('image_width', C.c_int32),
        ('image_height', C.c_int32), ('numbers_per_joint', C.c_int32), ('min_views', C.c_int32),
        ('median_axis', C.c_int32), ('used_joint_mask', C.c_uint32), ('threshold', C.c_float),
        ('median_window', C.c_double), ('max_frames', C.c_int32), ('max_heads', C.c_int32),
        ('max_edge_nodes', C.c_int32), ('max_heads_per_frame', C.c_int32),
        ('max_persons_per_frame', C.c_int32),
        ('Kinv', c_f32p), ('K', c_f32p), ('T_i', c_f32p), ('P', c_f64p), ('dist', c_f64p),
    ]


class mpe_batch(C.Structure):
    _fields_ = [
        ('n_frames', C.c_int32), ('n_heads', C.c_int32), ('n_edge_nodes', C.c_int32),
        ('d_frame_head_off', C.c_void_p), ('d_frame_en_off', C.c_void_p), ('d_slot_cam', C.c_void_p),
        ('d_slot_n', C.c_void_p), ('d_head_cam', C.c_void_p), ('d_joint_mask', C.c_void_p),
        ('d_tri_mask', C.c_void_p), ('d_xy', C.c_void_p), ('d_vp', C.c_void_p),
        ('d_en_pair', C.c_void_p),      # optional explicit edge-node list (process_training topology); NULL = implicit
        ('generation', C.c_uint64),     # changes whenever the arrays are rewritten in place (packing.next_generation; mpe.h: mpe_mlp3d_batch)
    ]


class mpe_packed_arrays(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('n_heads', C.c_int32), ('n_edge_nodes', C.c_int32),
                ('n_cameras', C.c_int32), ('n_joints', C.c_int32),
                ('frame_head_off', c_i32p), ('frame_en_off', c_i32p), ('slot_cam', c_i32p), ('slot_n', c_i32p),
                ('head_cam', c_i32p), ('skeleton_index', c_i32p), ('joint_mask', c_u32p), ('tri_mask', c_u32p),
                ('xy', c_f64p), ('vp', c_f32p)]


class mpe_pack_dst(C.Structure):
    _fields_ = [('max_frames', C.c_int32), ('max_heads', C.c_int32),
                ('frame_head_off', C.c_void_p), ('frame_en_off', C.c_void_p), ('slot_cam', C.c_void_p), ('slot_n', C.c_void_p),
                ('head_cam', C.c_void_p), ('skeleton_index', C.c_void_p), ('joint_mask', C.c_void_p), ('tri_mask', C.c_void_p),
                ('xy', C.c_void_p), ('vp', C.c_void_p)]


class mpe_eval_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('gcap', C.c_int32),
                ('pose_f64', C.c_int32), ('joint_flags', C.c_int32), ('used_joint_mask', C.c_uint32),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_gt_xyz', C.c_void_p),
                ('d_gt_joint', C.c_void_p), ('d_gt_valid', C.c_void_p), ('d_n_gt_in', C.c_void_p), ('d_skip', C.c_void_p),
                ('d_table', C.c_void_p), ('d_assign', C.c_void_p), ('d_err', C.c_void_p), ('d_invalid', C.c_void_p),
                ('d_n_gt', C.c_void_p), ('d_n_res', C.c_void_p), ('d_status', C.c_void_p)]


class mpe_track_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('used_joint_mask', C.c_uint32), ('gate', C.c_double),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p),
                ('d_track_id', C.c_void_p), ('d_link_cost', C.c_void_p), ('d_link_gap', C.c_void_p), ('d_issued', C.c_void_p)]


class mpe_smooth_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('fill', C.c_int32), ('joint_mask', C.c_uint32), ('lambda_', C.c_double),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p),
                ('d_poses_out', C.c_void_p), ('d_flags_out', C.c_void_p), ('d_vel', C.c_void_p), ('d_n_samples', C.c_void_p)]


class mpe_skel_config(C.Structure):
    _fields_ = [('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32), ('tid_cap', C.c_int32), ('n_bones', C.c_int32),
                ('reserved', C.c_int32), ('bin_width', C.c_double), ('bones', c_i32p)]


class mpe_skel_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('iters', C.c_int32), ('joint_mask', C.c_uint32), ('reserved', C.c_int32),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p),
                ('d_poses_out', C.c_void_p), ('d_err', C.c_void_p), ('d_n_bones', C.c_void_p)]


class mpe_relink_config(C.Structure):
    _fields_ = [('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32), ('tid_cap', C.c_int32), ('n_bones', C.c_int32),
                ('max_frames', C.c_int32), ('min_gap', C.c_int32), ('max_gap', C.c_int32), ('min_samples', C.c_int32), ('min_bones', C.c_int32),
                ('used_joint_mask', C.c_uint32), ('joint_mask', C.c_uint32), ('gate_m', C.c_double), ('max_bone_m', C.c_double),
                ('reach_m', C.c_double), ('reach_per_frame_m', C.c_double), ('bones', c_i32p)]


class mpe_relink_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('reserved', C.c_int32),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p),
                ('d_ids', C.c_void_p), ('d_link_cost', C.c_void_p), ('d_link_gap', C.c_void_p)]


class mpe_body_refine_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('sweeps', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float),
                ('bone_weight', C.c_double), ('huber_px', C.c_double),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p),
                ('d_persons', C.c_void_p), ('d_frame', C.c_void_p), ('d_poses_out', C.c_void_p), ('d_status', C.c_void_p),
                ('d_n_views', C.c_void_p), ('d_cost', C.c_void_p), ('d_err', C.c_void_p), ('d_n_bones', C.c_void_p)]


class mpe_track_score_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('gcap', C.c_int32), ('joint_flags', C.c_int32), ('threshold_mm', C.c_double),
                ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p), ('d_assign', C.c_void_p),
                ('d_err', C.c_void_p), ('d_invalid', C.c_void_p), ('d_n_res', C.c_void_p), ('d_n_gt', C.c_void_p), ('d_gt_id', C.c_void_p),
                ('d_gt_valid', C.c_void_p), ('d_skip', C.c_void_p), ('d_frame_counts', C.c_void_p), ('d_match_tid', C.c_void_p),
                ('d_status', C.c_void_p)]


class mpe_track_score_totals(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ('frames', 'n_gt', 'n_pred', 'tp', 'fp', 'fn', 'idsw', 'frag', 'ignored', 'over_ids',
                                         'idtp', 'n_ids', 'n_tracks', 'mt', 'pt', 'ml')] + \
               [(k, C.c_double) for k in ('err_sum', 'mota', 'motp_mm', 'idp', 'idr', 'idf1')] + [('status', C.c_int32), ('reserved', C.c_int32)]


class mpe_reproject_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p),
                ('d_res', C.c_void_p)]


class mpe_posecov_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float), ('huber_px', C.c_double),
                ('sigma_px', C.c_double), ('gate_m', C.c_double),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p),
                ('d_cov', C.c_void_p), ('d_sigma', C.c_void_p), ('d_status', C.c_void_p), ('d_n_views', C.c_void_p),
                ('d_flags_out', C.c_void_p)]


class mpe_refine_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float), ('max_iters', C.c_int32),
                ('step_tol', C.c_double), ('huber_px', C.c_double),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p),
                ('d_poses_out', C.c_void_p), ('d_status', C.c_void_p), ('d_cost0', C.c_void_p), ('d_cost1', C.c_void_p),
                ('d_iters', C.c_void_p), ('d_n_views', C.c_void_p)]


class mpe_regroup_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float), ('min_joints', C.c_int32),
                ('gate_px', C.c_double), ('clip_px', C.c_double), ('flags', C.c_uint32), ('reserved', C.c_int32),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p),
                ('d_persons_out', C.c_void_p), ('d_change', C.c_void_p), ('d_n_views', C.c_void_p), ('d_cost', C.c_void_p),
                ('d_counts', C.c_void_p), ('d_status', C.c_void_p)]


class mpe_consolidate_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float), ('min_joints', C.c_int32),
                ('merge_m', C.c_double), ('found_m', C.c_double), ('clip_m', C.c_double), ('found_min_views', C.c_int32),
                ('fcap', C.c_int32), ('flags', C.c_uint32), ('reserved', C.c_int32),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p),
                ('d_persons_out', C.c_void_p), ('d_n_persons_out', C.c_void_p), ('d_change', C.c_void_p), ('d_n_views', C.c_void_p),
                ('d_dist', C.c_void_p), ('d_pair', C.c_void_p), ('d_free', C.c_void_p), ('d_counts', C.c_void_p),
                ('d_status', C.c_void_p)]


class mpe_calib_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('threshold', C.c_float), ('reserved', C.c_int32),
                ('huber_px', C.c_double),
                ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p)]


class mpe_calib_step_args(C.Structure):
    _fields_ = [('rot_tol', C.c_double), ('trans_tol', C.c_double), ('min_obs', C.c_int64), ('hold_mask', C.c_uint32),
                ('reserved', C.c_int32)]


class mpe_calib_cam_report(C.Structure):
    _fields_ = [('status', C.c_int32), ('passes', C.c_int32), ('n_obs', C.c_int64), ('n_skipped', C.c_int64),
                ('cost_start', C.c_double), ('cost', C.c_double), ('lambda_', C.c_double), ('last_rot', C.c_double),
                ('last_trans', C.c_double), ('delta', C.c_double * 6)]


class mpe_calib_report(C.Structure):
    _fields_ = [('n_cameras', C.c_int32), ('all_done', C.c_int32), ('cam', mpe_calib_cam_report * MPE_MAX_CAMERAS)]


class mpe_camfit_step_args(C.Structure):
    _fields_ = [('rot_tol', C.c_double), ('trans_tol', C.c_double), ('pix_tol', C.c_double), ('lens_tol', C.c_double),
                ('min_obs', C.c_int64), ('hold_mask', C.c_uint32), ('free_mask', C.c_uint32)]


class mpe_camfit_cam_report(C.Structure):
    _fields_ = [('status', C.c_int32), ('passes', C.c_int32), ('n_obs', C.c_int64), ('n_skipped', C.c_int64),
                ('cost_start', C.c_double), ('cost', C.c_double), ('lambda_', C.c_double), ('last_rot', C.c_double),
                ('last_trans', C.c_double), ('last_pix', C.c_double), ('last_lens', C.c_double), ('delta', C.c_double * 13)]


class mpe_camfit_report(C.Structure):
    _fields_ = [('n_cameras', C.c_int32), ('all_done', C.c_int32), ('cam', mpe_camfit_cam_report * MPE_MAX_CAMERAS)]


class mpe_lag_config(C.Structure):
    _fields_ = [('pcap', C.c_int32), ('n_joints', C.c_int32), ('window', C.c_int32), ('sub', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('max_frames', C.c_int32), ('reserved', C.c_int32)]


class mpe_lag_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('frame_start', C.c_int32), ('n_table', C.c_int32), ('joint_mask', C.c_uint32),
                ('threshold', C.c_float), ('reserved', C.c_int32), ('huber_px', C.c_double),
                ('d_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p),
                ('d_tid', C.c_void_p)]


class mpe_lag_cam_report(C.Structure):
    _fields_ = [('status', C.c_int32), ('k_best', C.c_int32), ('lag_grid', C.c_double), ('lag_refined', C.c_double),
                ('cost_best', C.c_double), ('cost_zero', C.c_double), ('n_obs', C.c_int64), ('n_support', C.c_int64),
                ('n_unsupported', C.c_int64)]


class mpe_lag_report(C.Structure):
    _fields_ = [('n_cameras', C.c_int32), ('n_grid', C.c_int32), ('cam', mpe_lag_cam_report * MPE_MAX_CAMERAS)]


class mpe_refine_timed_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('frame_start', C.c_int32), ('n_table', C.c_int32), ('joint_mask', C.c_uint32),
                ('threshold', C.c_float), ('max_iters', C.c_int32), ('step_tol', C.c_double), ('huber_px', C.c_double),
                ('lag', C.c_double * MPE_MAX_CAMERAS),
                ('d_persons', C.c_void_p), ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p),
                ('d_tid', C.c_void_p),
                ('d_poses_out', C.c_void_p), ('d_status', C.c_void_p), ('d_cost0', C.c_void_p), ('d_cost1', C.c_void_p),
                ('d_iters', C.c_void_p), ('d_n_views', C.c_void_p), ('d_n_timed', C.c_void_p)]


class mpe_geom_args(C.Structure):
    _fields_ = [('sigma_m', C.c_double), ('clip_m', C.c_double), ('min_joints', C.c_int32), ('joint_mask', C.c_uint32),
                ('min_conf', C.c_float), ('d_scores', C.c_void_p), ('d_n_votes', C.c_void_p), ('d_mean', C.c_void_p)]


class mpe_residual_stats_args(C.Structure):
    _fields_ = [('n_buffers', C.c_int32), ('n_joints', C.c_int32), ('d_res', C.POINTER(C.c_void_p)), ('n_groups', C.POINTER(C.c_int64)),
                ('d_count', C.c_void_p), ('d_nonfinite', C.c_void_p), ('d_sum', C.c_void_p), ('d_mid', C.c_void_p)]


class mpe_partition_labels_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('hcap', C.c_int32), ('d_persons', C.c_void_p), ('d_n_persons', C.c_void_p),
                ('d_labels', C.c_void_p), ('d_count', C.c_void_p), ('d_status', C.c_void_p)]


class mpe_group_bodies_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('scap', C.c_int32), ('kcap', C.c_int32), ('d_xyz', C.c_void_p), ('d_mask', C.c_void_p),
                ('d_nkeys', C.c_void_p), ('d_order', C.c_void_p), ('d_m1', C.c_void_p), ('d_n', C.c_void_p), ('d_skip_in', C.c_void_p),
                ('d_labels', C.c_void_p), ('d_n_groups', C.c_void_p), ('d_skip', C.c_void_p), ('d_status', C.c_void_p)]


class mpe_partition_scores_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('ld_true', C.c_int32), ('ld_pred', C.c_int32), ('d_labels_true', C.c_void_p),
                ('d_labels_pred', C.c_void_p), ('d_count', C.c_void_p), ('d_count_true', C.c_void_p), ('d_skip', C.c_void_p),
                ('d_scores', C.c_void_p), ('d_status', C.c_void_p)]


class mpe_json_bodies_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('n_entries', C.c_int32), ('scap', C.c_int32), ('d_text', C.c_void_p), ('d_entries', C.c_void_p),
                ('d_frame_entry_off', C.c_void_p), ('d_xyz', C.c_void_p), ('d_mask', C.c_void_p), ('d_nkeys', C.c_void_p),
                ('d_order', C.c_void_p), ('d_m1', C.c_void_p), ('d_n', C.c_void_p), ('d_entry_count', C.c_void_p),
                ('d_body_cam', C.c_void_p), ('d_status', C.c_void_p), ('d_scratch', C.c_void_p), ('scratch_bytes', C.c_size_t)]


class mpe_gt_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('scap', C.c_int32), ('gcap', C.c_int32), ('n_joints', C.c_int32), ('n_files', C.c_int32),
                ('d_entries', C.c_void_p), ('d_frame_entry_off', C.c_void_p), ('d_entry_count', C.c_void_p), ('d_xyz', C.c_void_p),
                ('d_mask', C.c_void_p), ('d_m1', C.c_void_p), ('d_T_d', C.c_void_p), ('d_file_of_frame', C.c_void_p), ('T_i1', c_f32p),
                ('d_gt_xyz', C.c_void_p), ('d_gt_joint', C.c_void_p), ('d_gt_valid', C.c_void_p), ('d_n_gt_in', C.c_void_p)]


class mpe_json_write_args(C.Structure):
    _fields_ = [('n_frames', C.c_int32), ('pcap', C.c_int32), ('n_joints', C.c_int32), ('pose_f64', C.c_int32),
                ('joint_flags', C.c_int32), ('joint_mask', C.c_uint32), ('frame_start', C.c_int64), ('scale', C.c_double),
                ('d_poses', C.c_void_p), ('d_flags', C.c_void_p), ('d_n_persons', C.c_void_p), ('d_track_id', C.c_void_p),
                ('d_text', C.c_void_p), ('text_cap', C.c_uint64), ('d_frame_off', C.c_void_p), ('d_bodies_extent', C.c_void_p),
                ('d_rows_written', C.c_void_p), ('d_status', C.c_void_p), ('d_total', C.c_void_p), ('d_scratch', C.c_void_p),
                ('scratch_bytes', C.c_size_t)]


# key slots of mpe_json_parse_bodies_device: joint key "j" -> slot j (0..30), "-1" -> slot 31
MPE_GT_KEY_SLOTS, MPE_GT_M1_SLOT = 32, 31

# per-frame status bits and compiled caps of mpe_partition_labels / mpe_group_bodies / mpe_partition_scores
MPE_PART_SKIPPED, MPE_PART_OVER_CAP = 1, 2
MPE_PART_MAX_SAMPLES, MPE_PART_MAX_SKELETONS, MPE_PART_MAX_KEYS = 256, 1024, 32

# compiled caps of mpe_track_create
MPE_TRACK_MAX_PERSONS, MPE_TRACK_MAX_GAP = 128, 15

# the window cap of mpe_smooth_create and the output flag of a joint that mpe_smooth_batch filled in
MPE_SMOOTH_MAX_WINDOW, MPE_SMOOTH_FILLED = 15, 2

# the caps of mpe_skel_create / mpe_skel_fit_batch and the sticky status bit of mpe_skel_observe_batch
MPE_SKEL_BINS, MPE_SKEL_MAX_BONES, MPE_SKEL_MAX_ITERS, MPE_SKEL_OVER_IDS, MPE_SKEL_MAX_HIST_BYTES = 512, 32, 64, 1, 256 << 20

# the caps of mpe_relink_create and the sticky status bit of mpe_relink_batch
MPE_RELINK_MAX_TID_CAP, MPE_RELINK_MAX_GAP, MPE_RELINK_OVER_IDS = 4096, 1 << 30, 1

# per-joint status bits of mpe_body_refine_batch
MPE_BODY_REFINE_FREE, MPE_BODY_REFINE_MOVED, MPE_BODY_REFINE_BAD_START, MPE_BODY_REFINE_ONE_VIEW, MPE_BODY_REFINE_BAD_FRAME = 1, 2, 4, 8, 16

# the sticky status bit of mpe_track_score_batch and the cap on gid_cap * tid_cap of mpe_track_score_create
MPE_TRACK_SCORE_OVER_IDS, MPE_TRACK_SCORE_MAX_TABLE = 1, 1 << 22

# per-joint status bits and the iteration cap of mpe_refine_batch
MPE_REFINE_SOLVED, MPE_REFINE_MOVED, MPE_REFINE_CONVERGED, MPE_REFINE_FEW_VIEWS, MPE_REFINE_BAD_START = 1, 2, 4, 8, 16
MPE_REFINE_MAX_ITERS = 64

# per-joint status bits of mpe_posecov_batch
MPE_POSECOV_COMPUTED, MPE_POSECOV_FEW_VIEWS, MPE_POSECOV_BAD_POSE, MPE_POSECOV_SINGULAR, MPE_POSECOV_GATED = 1, 8, 16, 32, 64

# per-frame status bits, the pass flags and the row cap of mpe_regroup_batch
MPE_REGROUP_BAD_ROWS, MPE_REGROUP_OVER_CAP = 1, 2
MPE_REGROUP_RELEASE, MPE_REGROUP_ATTACH = 1, 2
MPE_REGROUP_MAX_PERSONS = 128
# per-frame status bits, the pass flags and the caps of mpe_consolidate_batch
MPE_CONSOLIDATE_BAD_ROWS, MPE_CONSOLIDATE_OVER_CAP, MPE_CONSOLIDATE_FREE_OVER_CAP, MPE_CONSOLIDATE_ROWS_FULL = 1, 2, 4, 8
MPE_CONSOLIDATE_MERGE, MPE_CONSOLIDATE_FOUND = 1, 2
MPE_CONSOLIDATE_MAX_FREE = 64
MPE_CONSOLIDATE_RAY_DOUBLES = 3520

# per-camera status bits of mpe_calib_step and the sums a camera accumulates
MPE_CALIB_HELD, MPE_CALIB_FEW_OBS, MPE_CALIB_CONVERGED, MPE_CALIB_STALLED, MPE_CALIB_ACCEPTED, MPE_CALIB_REJECTED = 1, 2, 4, 8, 16, 32
MPE_CALIB_SUMS = 28

# the groups of unknowns of mpe_camfit_step (free_mask), by name, and the sums a camera accumulates
MPE_CAMFIT_POSE, MPE_CAMFIT_FOCAL, MPE_CAMFIT_CENTRE, MPE_CAMFIT_K1, MPE_CAMFIT_K2, MPE_CAMFIT_K3 = 1, 2, 4, 8, 16, 32
MPE_CAMFIT_GROUPS = {'pose': 1, 'focal': 2, 'centre': 4, 'k1': 8, 'k2': 16, 'k3': 32}
MPE_CAMFIT_UNKNOWNS = 13
MPE_CAMFIT_SUMS = 105

# per-camera status bits of mpe_lag_estimate and the caps of mpe_lag_create
MPE_LAG_FEW_OBS, MPE_LAG_EDGE, MPE_LAG_FLAT = 1, 2, 4
MPE_LAG_MAX_WINDOW, MPE_LAG_MAX_SUB = 8, 8
# mpe_refine_timed_batch: the status bits are mpe_refine_batch's, and a lag is within this many frames either way
MPE_REFINE_TIMED_MAX_LAG = MPE_LAG_MAX_WINDOW

# per-frame status bit and the total's capacity bit of mpe_json_write_poses; the bytes of a conversion slot, the longest
# line that is put together on chip, and the row cap
MPE_WRITE_NONFINITE, MPE_WRITE_CAPACITY = 1, 2
MPE_JSON_WRITE_SLOT_BYTES, MPE_JSON_WRITE_STAGE_BYTES, MPE_JSON_WRITE_MAX_PERSONS = 32, 16384, 1024

# per-frame status bits of mpe_eval_batch
MPE_EVAL_SKIPPED, MPE_EVAL_OVER_CAP, MPE_EVAL_OVER_BUDGET, MPE_EVAL_NO_ASSIGNMENT = 1, 2, 4, 8


# name -> (restype, argtypes); must list every symbol include/mpe.h declares
SYMBOLS = {
    'mpe_create': (C.c_int, [C.POINTER(mpe_config), C.POINTER(C.c_void_p)]),
    'mpe_destroy': (None, [C.c_void_p]),
    'mpe_last_error': (C.c_char_p, [C.c_void_p]),
    'mpe_version': (C.c_char_p, []),
    'mpe_set_gat_params': (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float]),
    'mpe_set_gat_layer': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    c_f32p, c_f32p, c_f32p, c_f32p, c_f32p, c_f32p]),
    'mpe_set_mlp_params': (C.c_int, [C.c_void_p, C.c_int32, C.c_float]),
    'mpe_set_mlp_layer': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, c_f32p, c_f32p]),
    'mpe_set_precision': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    'mpe_match_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_mlp3d_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    'mpe_triangulate_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint32]),
    'mpe_upload_linear': (C.c_int, [C.c_void_p, c_f32p, c_f32p, C.c_int32, C.c_int32,
                                    C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)]),
    'mpe_free_device': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_linear': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                             C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                             C.c_float]),
    'mpe_head_features': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p]),
    'mpe_dense_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_int32]),
    'mpe_gat_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_void_p]),
    'mpe_set_gat_output': (C.c_int, [C.c_void_p, C.c_int32]),
    'mpe_gat_layer': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_int32, C.c_void_p, C.c_int32,
                                C.c_void_p, C.c_int32, C.c_int32]),
    'mpe_edge_softmax_aggregate': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_int32, C.c_void_p,
                                             C.c_int32, C.c_void_p, C.c_int32]),
    'mpe_sync_status': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_status_queue': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_status_wait': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_set_threshold': (C.c_int, [C.c_void_p, C.c_float]),
    'mpe_cluster_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p,
                                    C.c_void_p]),
    'mpe_mlp_input_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, C.c_void_p]),
    'mpe_mlp_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    'mpe_eval_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_eval_args)]),
    'mpe_track_create': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'mpe_track_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_track_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_track_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_track_args)]),
    'mpe_track_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_smooth_create': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'mpe_smooth_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_smooth_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_smooth_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_smooth_args)]),
    'mpe_smooth_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_skel_create': (C.c_int, [C.c_void_p, C.POINTER(mpe_skel_config), C.POINTER(C.c_void_p)]),
    'mpe_skel_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_skel_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_skel_observe_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_skel_args)]),
    'mpe_skel_update': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    'mpe_skel_set_lengths': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_skel_get_lengths': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_skel_fit_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_skel_args)]),
    'mpe_skel_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_body_refine_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_body_refine_args)]),
    'mpe_relink_create': (C.c_int, [C.c_void_p, C.POINTER(mpe_relink_config), C.POINTER(C.c_void_p)]),
    'mpe_relink_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_relink_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_relink_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_relink_args)]),
    'mpe_relink_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_relink_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_track_score_create': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'mpe_track_score_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_track_score_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_track_score_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_track_score_args)]),
    'mpe_track_score_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_track_score_result': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_track_score_totals)]),
    'mpe_track_score_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_reproject_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_reproject_args)]),
    'mpe_refine_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_refine_args)]),
    'mpe_posecov_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_posecov_args)]),
    'mpe_regroup_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_regroup_args)]),
    'mpe_consolidate_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_consolidate_args)]),
    'mpe_calib_create': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    'mpe_calib_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_calib_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_calib_set_extrinsics': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f64p]),
    'mpe_calib_get_extrinsics': (C.c_int, [C.c_void_p, C.c_void_p, c_f64p, c_f64p]),
    'mpe_calib_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_calib_args)]),
    'mpe_calib_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mpe_calib_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_calib_step_args), C.POINTER(mpe_calib_report)]),
    'mpe_calib_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_camfit_create': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    'mpe_camfit_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_camfit_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_camfit_set_cameras': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f64p, c_f32p, c_f64p]),
    'mpe_camfit_get_cameras': (C.c_int, [C.c_void_p, C.c_void_p, c_f64p, c_f32p, c_f64p, c_f64p, c_f32p, c_f64p]),
    'mpe_camfit_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_calib_args)]),
    'mpe_camfit_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'mpe_camfit_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_camfit_step_args), C.POINTER(mpe_camfit_report)]),
    'mpe_camfit_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_lag_create': (C.c_int, [C.c_void_p, C.POINTER(mpe_lag_config), C.POINTER(C.c_void_p)]),
    'mpe_lag_reset': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'mpe_lag_destroy': (C.c_int, [C.c_void_p, C.c_void_p]),
    'mpe_lag_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_lag_args)]),
    'mpe_lag_launches': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'mpe_lag_read': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, c_f64p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                               C.POINTER(C.c_int64)]),
    'mpe_lag_estimate': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(mpe_lag_report)]),
    'mpe_refine_timed_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_refine_timed_args)]),
    'mpe_geom_scores_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_geom_args)]),
    'mpe_geom_match_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_geom_args), C.c_void_p, C.c_void_p]),
    'mpe_residual_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_residual_stats_args)]),
    'mpe_partition_labels': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_batch), C.POINTER(mpe_partition_labels_args)]),
    'mpe_group_bodies': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_group_bodies_args)]),
    'mpe_set_log_table': (C.c_int, [C.c_void_p, c_f64p, C.c_int32]),
    'mpe_partition_scores': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_partition_scores_args)]),
    'mpe_dlt_pairs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    'mpe_pack_json': (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    'mpe_packed_view': (C.c_int, [C.c_void_p, C.POINTER(mpe_packed_arrays)]),
    'mpe_pack_json_into': (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_int32, C.POINTER(mpe_pack_dst), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'mpe_pack_views_into': (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                      C.POINTER(mpe_pack_dst), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    'mpe_json_index_create': (C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    'mpe_json_index_free': (None, [C.c_void_p]),
    'mpe_pack_indexed_into': (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.POINTER(mpe_pack_dst), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    'mpe_json_stage_window': (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    'mpe_json_scratch_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'mpe_json_parse_device': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.POINTER(mpe_batch), C.c_void_p, C.c_void_p]),
    'mpe_json_stage_gt_window': (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_void_p, C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), C.POINTER(C.c_size_t)]),
    'mpe_json_bodies_scratch_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'mpe_json_parse_bodies_device': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_json_bodies_args)]),
    'mpe_gt_from_bodies': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_gt_args)]),
    'mpe_json_write_poses': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(mpe_json_write_args)]),
    'mpe_json_write_bound': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'mpe_json_write_scratch_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'mpe_json_write_launches': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    # n is an int64_t in the header: passed as the 64-bit size type, which carries the same bits (a negative n included)
    'mpe_format_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    'mpe_packed_free': (None, [C.c_void_p]),
    'mpe_pack_last_error': (C.c_char_p, []),
    'mpe_profile_enable': (C.c_int, [C.c_void_p, C.c_int32]),
    'mpe_profile_read': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    'mpe_profile_read_split': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'mpe_profile_read_bf16': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'mpe_l0_attention_launches': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
}

_lib = None


def hip_runtimes_mapped():
    """Real paths of every libamdhip64 mapped into this process (Linux: /proc/self/maps)."""
    paths = set()
    try:
        with open('/proc/self/maps') as fh:
            for line in fh:
                if 'libamdhip64' in line:
                    paths.add(os.path.realpath(line.split()[-1]))
    except OSError:
        pass
    return sorted(paths)


def load():
    """Return the loaded library; raise if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError('%s is missing: build it with `python __graft_entry__.py` or '
                          '`make -C 3d_multi_pose_estimator_amd/csrc` (hipcc, gfx950). '
                          'There is no CPU fallback.' % LIB_PATH)
    # torch first, if it is there: libmpe_hip.so needs libamdhip64, and a process that already has the system's copy loaded
    # when torch later brings its own talks to two HIP runtimes at once (device tensors of one, kernels of the other)
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    rts = hip_runtimes_mapped()
    if len(rts) > 1:
        # device memory of one runtime, kernels of the other: every later call would fail with an opaque MPE_ERR_HIP (-4)
        raise ImportError('two HIP runtimes are mapped into this process (%s): something loaded a libamdhip64 before torch '
                          'brought its own.  Import torch (or this package) BEFORE anything that dlopens the system HIP '
                          'runtime, e.g. before ctypes.CDLL(%r).' % (', '.join(rts), LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(ctx, rc):
    if rc != 0:
        msg = load().mpe_last_error(ctx)
        raise MpeError(rc, msg.decode() if msg else '?')
