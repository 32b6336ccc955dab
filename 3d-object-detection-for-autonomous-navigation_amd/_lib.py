"""ctypes binding of the C-ABI in include/pp_hip.h (libpp_hip.so, built in-tree by hipcc).

There is no CPU fallback: if the shared library is missing or cannot be
loaded, `lib()` raises, and every compute entry point needs a gfx950 device
(`pp_create` fails without one).  `build()` only needs hipcc (it cross-compiles
for gfx950 on a machine without a GPU).
"""
import ctypes
import os
import shutil
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, "csrc")
_INCLUDE = os.path.join(os.path.dirname(_PKG), "include", "pp_hip.h")
# PP_HIP_LIB: load (and build into) another library file -- A/B builds with extra compiler flags, e.g.
#   PP_HIP_LIB=libpp_hip_g.so PP_HIPCC_EXTRA="-g" python -c "import pp_amd; pp_amd._lib.build()"
SO_PATH = os.path.join(_PKG, os.environ.get("PP_HIP_LIB", "libpp_hip.so"))
_VARIANT = os.path.splitext(os.path.basename(SO_PATH))[0]
SOURCES = ["pp_api.hip", "api_ingest.hip", "api_crop.hip", "api_eval.hip", "api_nms.hip", "api_project.hip", "api_class_nms.hip", "api_metrics.hip", "api_publish.hip", "api_train.hip", "api_dataprep.hip", "voxelize.hip", "pfn.hip", "anchor_mask.hip", "backbone.hip", "postprocess.hip",
           "rotate_iou.hip", "rotate_nms.hip", "box_project.hip", "loss.hip", "metrics.hip", "optim.hip", "grad_clip.hip", "train.hip", "targets.hip", "augment.hip", "gt_sample.hip", "ingest.hip",
           "gt_database.hip", "eval_stats.hip", "frustum_crop.hip", "weight_publish.hip", "soft_nms.hip",
           "api_sweeps.hip", "sweeps.hip",
           "api_costmap.hip", "costmap.hip",
           "api_occupancy.hip", "occupancy.hip",
           "api_inflate.hip", "inflate.hip",
           "api_navfn.hip", "navfn.hip",
           "api_local_plan.hip", "local_plan.hip", "local_movers.hip",
           "api_scan_match.hip", "scan_match.hip",
           "api_frontier.hip", "frontier.hip",
           "api_object_mask.hip", "object_mask.hip",
           "api_ground.hip", "ground.hip",
           "api_track.hip", "track.hip"]
# -fno-slp-vectorize: keeps f32 FMAs as v_fma_f32; the SLP vectoriser's v_pk_fma_f32 is slow on a SIMD
# that is also issuing MFMAs (MI355X_MICROARCH.md, "price of one filler beside MFMAs")
HIPCC_FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off",
               "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"]

EXPORTS = [
    "pp_abi_version", "pp_create", "pp_destroy", "pp_last_error", "pp_set_weight", "pp_finalize_weights",
    "pp_set_anchors", "pp_points_to_voxel", "pp_anchor_mask", "pp_forward_voxels", "pp_predict",
    "pp_upload_points", "pp_upload_points_async", "pp_host_alloc", "pp_host_free", "pp_upload_points_device",
    "pp_current_batch", "pp_set_calib", "pp_detect_async", "pp_sync",
    "pp_get_detections", "pp_set_gemm_precision", "pp_get_gemm_precision", "pp_set_cache_budget", "pp_detect", "pp_fetch_intermediates", "pp_set_profiling", "pp_get_kernel_times",
    "pp_timer_start", "pp_timer_stop", "pp_device_info", "pp_device_copy_bench", "pp_device_mem_free", "pp_bench_layer", "pp_layer_count", "pp_layer_tag", "pp_plan_layer_name",
    "pp_rotate_iou_eval", "pp_d3_box_overlap", "pp_head_loss", "pp_adamw_step_device",
    "pp_train_layout", "pp_train_layout_entry", "pp_train_step", "pp_train_step_async", "pp_train_step_wait",
    "pp_train_graph_stats", "pp_stream", "pp_train_fetch_decisions",
    "pp_assign_targets", "pp_train_step_gt_async", "pp_train_step_gt",
    "pp_augment", "pp_train_step_aug_async", "pp_train_step_aug", "pp_augment_selected",
    "pp_train_set_frozen", "pp_adamw_step_segments_device",
    "pp_gtdb_load", "pp_gt_sample", "pp_gt_sample_info", "pp_train_step_sample_async", "pp_train_step_sample",
    "pp_ingest_pointcloud2", "pp_ingest_pointcloud2_async", "pp_ingest_info",
    "pp_ingest_depth", "pp_ingest_depth_async",
    "pp_ingest_rig_depth", "pp_ingest_rig_depth_async", "pp_ingest_rig_pointcloud2", "pp_ingest_rig_pointcloud2_async",
    "pp_ingest_rig_info",
    "pp_ingest_pointcloud2_fields", "pp_ingest_pointcloud2_fields_async",
    "pp_ingest_rig_pointcloud2_fields", "pp_ingest_rig_pointcloud2_fields_async",
    "pp_gtdb_build", "pp_gtdb_count",
    "pp_eval_match", "pp_eval_pr",
    "pp_frustum_crop", "pp_frustum_crop_async", "pp_frustum_crop_info",
    "pp_set_sweeps", "pp_get_sweeps", "pp_sweeps_accumulate", "pp_sweeps_accumulate_async", "pp_sweeps_info", "pp_sweeps_reset",
    "pp_set_track_pose", "pp_get_tracks_fixed",
    "pp_set_costmap", "pp_get_costmap_config", "pp_costmap_async", "pp_get_costmaps", "pp_costmap_info",
    "pp_set_occupancy", "pp_get_occupancy_config", "pp_occupancy_update_async", "pp_get_occupancy", "pp_occupancy_info",
    "pp_occupancy_reset",
    "pp_set_inflation", "pp_get_inflation_config", "pp_inflate_async", "pp_get_inflated", "pp_inflation_info",
    "pp_inflate_grids",
    "pp_set_navfn", "pp_get_navfn_config", "pp_navfn_async", "pp_get_navfn", "pp_navfn_info", "pp_navfn_grids",
    "pp_set_local_plan", "pp_get_local_plan_config", "pp_local_plan_async", "pp_get_local_plan", "pp_local_plan_grids",
    "pp_set_local_movers", "pp_get_local_movers_config", "pp_local_plan_movers_async", "pp_get_local_movers",
    "pp_local_plan_grids_movers",
    "pp_set_scan_match", "pp_get_scan_match_config", "pp_scan_match_async", "pp_get_scan_match", "pp_scan_match_grids",
    "pp_set_frontier", "pp_get_frontier_config", "pp_frontier_async", "pp_get_frontiers", "pp_frontier_grids",
    "pp_set_local_footprint", "pp_get_local_footprint_config", "pp_get_local_footprint", "pp_local_plan_grids_footprint",
    "pp_set_object_mask", "pp_get_object_mask_config", "pp_object_mask_async", "pp_object_mask_shape", "pp_get_object_mask",
    "pp_occupancy_masked", "pp_object_mask_points",
    "pp_set_ground", "pp_get_ground_config", "pp_ground_async", "pp_ground_used", "pp_ground_shape", "pp_get_ground", "pp_ground_points",
    "pp_set_nms_mode", "pp_get_nms_mode", "pp_rotate_nms",
    "pp_set_projection", "pp_get_projection", "pp_get_bboxes", "pp_box3d_to_bbox",
    "pp_set_class_nms", "pp_get_class_nms", "pp_get_detection_rows",
    "pp_head_metrics", "pp_set_train_metrics", "pp_get_train_metrics_enabled", "pp_get_train_metrics",
    "pp_grad_clip_workspace_bytes", "pp_grad_norm_device", "pp_adamw_step_clipped_device",
    "pp_publish_train_weights", "pp_publish_info",
    "pp_set_soft_nms", "pp_get_soft_nms", "pp_soft_nms",
    "pp_set_tracking", "pp_get_tracking", "pp_set_track_dt", "pp_get_tracks", "pp_track_update", "pp_track_reset",
    "pp_track_info",
]


class PPConfig(ctypes.Structure):
    _fields_ = [
        ("pc_range", ctypes.c_double * 6),
        ("voxel_size", ctypes.c_double * 3),
        ("max_points", ctypes.c_int32),
        ("max_voxels", ctypes.c_int32),
        ("num_point_features", ctypes.c_int32),
        ("pfn_filters", ctypes.c_int32),
        ("layer_nums", ctypes.c_int32 * 3),
        ("layer_strides", ctypes.c_int32 * 3),
        ("num_filters", ctypes.c_int32 * 3),
        ("upsample_strides", ctypes.c_int32 * 3),
        ("num_upsample_filters", ctypes.c_int32 * 3),
        ("num_anchor_per_loc", ctypes.c_int32),
        ("num_class", ctypes.c_int32),
        ("nms_pre_max_size", ctypes.c_int32),
        ("nms_post_max_size", ctypes.c_int32),
        ("nms_score_threshold", ctypes.c_float),
        ("nms_iou_threshold", ctypes.c_float),
        ("anchor_area_threshold", ctypes.c_float),
        ("max_batch", ctypes.c_int32),
        ("max_points_per_frame", ctypes.c_int32),
        ("use_direction_classifier", ctypes.c_int32),
        ("with_distance", ctypes.c_int32),
    ]


class PPLossConfig(ctypes.Structure):
    _fields_ = [
        ("alpha", ctypes.c_float),
        ("gamma", ctypes.c_float),
        ("sigma", ctypes.c_float),
        ("code_weight", ctypes.c_float * 7),
        ("pos_class_weight", ctypes.c_float),
        ("neg_class_weight", ctypes.c_float),
        ("classification_weight", ctypes.c_float),
        ("localization_weight", ctypes.c_float),
        ("direction_loss_weight", ctypes.c_float),
        ("norm_by_num_positives", ctypes.c_int32),
        ("encode_rad_error_by_sin", ctypes.c_int32),
        ("use_direction_classifier", ctypes.c_int32),
    ]


class PPLayerPlanDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "cin", "cout", "n_total", "stride", "k", "in_h", "in_w", "out_h", "out_w",
                                              "head_mode", "has_wt16", "has_head_wt16", "sparse_input")]


class PPTargetConfig(ctypes.Structure):
    _fields_ = [
        ("matched_threshold", ctypes.c_float),
        ("unmatched_threshold", ctypes.c_float),
        ("reserved", ctypes.c_int32 * 2),
    ]


class PPAugmentConfig(ctypes.Structure):
    _fields_ = [
        ("num_try", ctypes.c_int32),
        ("global_rot_per_object", ctypes.c_int32),
    ]


class PPGradClipConfig(ctypes.Structure):
    _fields_ = [
        ("mode", ctypes.c_int32),
        ("clip", ctypes.c_float),
        ("skip_nonfinite", ctypes.c_int32),
    ]


class PPPublishStats(ctypes.Structure):
    _fields_ = [
        ("publishes", ctypes.c_int64),
        ("reallocations", ctypes.c_int64),
        ("graph_invalidations", ctypes.c_int64),
        ("f32_fallback_layers", ctypes.c_int64),
    ]


class PPGtSampleConfig(ctypes.Structure):
    _fields_ = [
        ("max_point_collision", ctypes.c_int32),
        ("min_point_collision", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class PPGtsCand(ctypes.Structure):
    _fields_ = [
        ("object", ctypes.c_int32),
        ("group", ctypes.c_int32),
        ("low", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPPc2Layout(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("point_step", ctypes.c_int32),
        ("row_step", ctypes.c_int32),
        ("x_offset", ctypes.c_int32),
        ("y_offset", ctypes.c_int32),
        ("z_offset", ctypes.c_int32),
        ("datatype", ctypes.c_int32),
        ("is_bigendian", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPIngestConfig(ctypes.Structure):
    _fields_ = [
        ("first", ctypes.c_int32),
        ("decimate", ctypes.c_int32),
        ("r", ctypes.c_double * 9),
        ("r2", ctypes.c_double * 9),
        ("lift", ctypes.c_double * 3),
    ]


class PPPc2Feature(ctypes.Structure):
    _fields_ = [
        ("offset", ctypes.c_int32),
        ("datatype", ctypes.c_int32),
        ("scale", ctypes.c_double),
        ("bias", ctypes.c_double),
    ]


class PPDepthLayout(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("row_step", ctypes.c_int32),
        ("encoding", ctypes.c_int32),
        ("is_bigendian", ctypes.c_int32),
        ("fx", ctypes.c_float),
        ("fy", ctypes.c_float),
        ("ppx", ctypes.c_float),
        ("ppy", ctypes.c_float),
        ("depth_scale", ctypes.c_float),
        ("z_min", ctypes.c_float),
        ("z_max", ctypes.c_float),
    ]


PP_DEPTH_U16, PP_DEPTH_F32 = 0, 1      # pp_depth_layout.encoding
PP_RIG_MAX_SOURCES = 16      # sources per frame of a pp_ingest_rig_* call
PP_CROP_BACK = 1      # pp_frustum_crop* flags: bit 0
PP_SWEEP_MAX = 8      # past sweeps per stream (pp_set_sweeps)
PP_METRICS_COUNTS = 32      # int64 values of pp_head_metrics / pp_get_train_metrics
PP_CLASS_NMS_JOINT, PP_CLASS_NMS_PER_CLASS = 0, 1      # enum pp_class_nms
PP_NMS_STANDUP, PP_NMS_ROTATED, PP_NMS_SOFT = 0, 1, 2      # enum pp_nms_mode
PP_SOFT_NMS_HARD, PP_SOFT_NMS_LINEAR, PP_SOFT_NMS_GAUSSIAN = 0, 1, 2      # enum pp_soft_nms_method
PP_SNMS_MAX_BOXES = 4096      # most boxes that enter pp_soft_nms after pre_max_size
PP_TRACK_MAX = 64      # tracks per stream (pp_set_tracking)
PP_TRACK_MASK_ROWS = 128      # detection rows per frame the tracking step takes
PP_COSTMAP_MAX_STEPS = 8      # predicted footprints per track (pp_set_costmap)
PP_COSTMAP_MAX_CELLS = 262144      # width * height of a costmap
PP_OCC_MAX_CELLS = 1048576      # width * height of an occupancy window (pp_set_occupancy)
PP_INFLATE_MAX_RADIUS = 64      # cells: ceil(inflation_radius / resolution) at most (pp_set_inflation)
PP_INFLATE_COSTMAP, PP_INFLATE_OCCUPANCY = 0, 1      # `source` of the pp_*inflat* calls, and of the pp_*navfn* calls behind them
PP_NAVFN_UNREACHED = 0xFFFFFFFF # the potential of a cell no chain of moves joins to the goal (pp_get_navfn)
PP_NAVFN_MAX_PATH = 4096        # cells: pp_navfn_config.max_path at most
PP_LOCAL_SUB = 1024             # sub-cells per cell: the unit of a pose's X and Y (pp_local_plan_async)
PP_LOCAL_HEADINGS = 4096        # heading ticks per revolution
PP_LOCAL_MAX_SAMPLES = 16384    # pp_local_plan_config.nv * nw at most
PP_LOCAL_MAX_STEPS = 256        # pp_local_plan_config.steps at most
PP_LOCAL_MAX_LOOKAHEAD = 16384  # sub-cells: pp_local_plan_config.lookahead at most
PP_LOCAL_RESULT = 8             # int32 words per grid of pp_get_local_plan's result
PP_LOCAL_MAX_MOVERS = 64        # movers per grid (pp_local_plan_movers_async: a track slot each)
PP_LOCAL_MAX_MOVER_SPEED = 16384    # sub-cells per step: |mvx|, |mvy| at most
PP_LOCAL_MAX_MOVER_RADIUS = 32767   # sub-cells: r_soft at most
PP_LOCAL_MOVER_INFO = 4         # int32 words per grid of pp_get_local_movers' info
PP_LOCAL_MAX_PROBES = 256       # probes of a footprint (pp_set_local_footprint)
PP_LOCAL_MAX_PROBE = 32767      # sub-cells: |fx|, |fy| of a probe at most
PP_LOCAL_FOOT_INFO = 4          # int32 words per grid of pp_get_local_footprint's info
PP_SCAN_MAX_CANDIDATES = 65536  # pp_scan_match_config: (2 nx + 1)(2 ny + 1)(2 nt + 1) at most
PP_SCAN_RESULT = 8              # int32 words per stream of pp_get_scan_match's result
PP_OBJMASK_MAX_FOOTPRINTS = 128  # footprints of a frame's object mask (pp_set_object_mask)
PP_OBJMASK_INFO = 4              # int32 words per frame of pp_get_object_mask's info
PP_OBJMASK_OCCUPANCY, PP_OBJMASK_SCAN_MATCH, PP_OBJMASK_COSTMAP = 1, 2, 4     # bits of pp_object_mask_config.consumers
PP_GROUND_MAX_HYP = 512         # hypotheses of a frame's ground fit at most (pp_set_ground)
PP_GROUND_INFO = 12             # int32 words per frame of pp_get_ground's info
PP_GROUND_SUMS = 9              # int64 sums per frame of its refit
PP_GROUND_OCCUPANCY, PP_GROUND_SCAN_MATCH, PP_GROUND_COSTMAP = 1, 2, 4        # bits of pp_ground_config.consumers
PP_SCAN_NO_MAP, PP_SCAN_OUTSIDE, PP_SCAN_FEW_CELLS, PP_SCAN_LOW_SCORE, PP_SCAN_EDGE = 1, 2, 4, 8, 16      # its status bits
PP_FRONTIER_MAX = 64            # frontiers pp_get_frontiers returns per grid at most
PP_FRONTIER_INFO = 6            # int32 words per grid of its info: frontier_cells, clusters, small, unreached, kept, returned
PP_FRONTIER_NONE = 0xFFFFFFFF   # the label of a cell that is no frontier cell
PP_CLIP_NONE, PP_CLIP_VALUE, PP_CLIP_NORM, PP_CLIP_GLOBAL_NORM = 0, 1, 2, 3      # enum pp_grad_clip_mode


class PPDetection(ctypes.Structure):
    _fields_ = [
        ("box3d_camera", ctypes.c_double * 7),
        ("box3d_lidar", ctypes.c_float * 7),
        ("score", ctypes.c_float),
        ("label", ctypes.c_int32),
        ("dir_label", ctypes.c_int32),
        ("anchor_index", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPTrackConfig(ctypes.Structure):
    _fields_ = [
        ("gate", ctypes.c_double),
        ("q_acc", ctypes.c_double),
        ("r_pos", ctypes.c_double),
        ("p0_pos", ctypes.c_double),
        ("p0_vel", ctypes.c_double),
        ("size_alpha", ctypes.c_double),
        ("birth_score", ctypes.c_double),
        ("period", ctypes.c_double),
        ("max_misses", ctypes.c_int32),
        ("min_hits", ctypes.c_int32),
        ("class_aware", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPSweepConfig(ctypes.Structure):
    _fields_ = [
        ("max_age", ctypes.c_double),
        ("history", ctypes.c_int32),
        ("capacity", ctypes.c_int32),
        ("history_decimate", ctypes.c_int32),
        ("time_feature", ctypes.c_int32),
    ]


class PPCostmapConfig(ctypes.Structure):
    _fields_ = [
        ("x_min", ctypes.c_double),
        ("y_min", ctypes.c_double),
        ("resolution", ctypes.c_double),
        ("z_min", ctypes.c_double),
        ("z_max", ctypes.c_double),
        ("pad", ctypes.c_double),
        ("min_score", ctypes.c_double),
        ("horizon_dt", ctypes.c_double),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("min_points", ctypes.c_int32),
        ("objects", ctypes.c_int32),
        ("confirmed_only", ctypes.c_int32),
        ("horizon_steps", ctypes.c_int32),
        ("point_cost", ctypes.c_int32),
        ("object_cost", ctypes.c_int32),
        ("predict_cost", ctypes.c_int32 * PP_COSTMAP_MAX_STEPS),
    ]


class PPOccupancyConfig(ctypes.Structure):
    _fields_ = [
        ("resolution", ctypes.c_double),
        ("z_min", ctypes.c_double),
        ("z_max", ctypes.c_double),
        ("max_range", ctypes.c_double),
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("l_hit", ctypes.c_int32),
        ("l_miss", ctypes.c_int32),
        ("l_min", ctypes.c_int32),
        ("l_max", ctypes.c_int32),
    ]


class PPInflationConfig(ctypes.Structure):
    _fields_ = [
        ("resolution", ctypes.c_double),
        ("inscribed_radius", ctypes.c_double),
        ("inflation_radius", ctypes.c_double),
        ("cost_scaling_factor", ctypes.c_double),
        ("lethal_threshold", ctypes.c_int32),
        ("unknown_min_cost", ctypes.c_int32),
    ]


class PPNavfnConfig(ctypes.Structure):
    _fields_ = [
        ("lethal_cost", ctypes.c_int32),
        ("neutral_cost", ctypes.c_int32),
        ("cost_factor", ctypes.c_int32),
        ("allow_unknown", ctypes.c_int32),
        ("unknown_cost", ctypes.c_int32),
        ("connectivity", ctypes.c_int32),
        ("max_path", ctypes.c_int32),
        ("queued_rounds", ctypes.c_int32),
    ]


class PPLocalPlanConfig(ctypes.Structure):
    _fields_ = [
        ("nv", ctypes.c_int32),
        ("nw", ctypes.c_int32),
        ("steps", ctypes.c_int32),
        ("lookahead", ctypes.c_int32),
        ("pot_weight", ctypes.c_int32),
        ("occ_weight", ctypes.c_int32),
        ("speed_weight", ctypes.c_int32),
        ("turn_weight", ctypes.c_int32),
    ]


class PPLocalMoverConfig(ctypes.Structure):
    _fields_ = [
        ("pad_hard", ctypes.c_double),
        ("pad_soft", ctypes.c_double),
        ("horizon", ctypes.c_int32),
        ("mover_weight", ctypes.c_int32),
        ("confirmed_only", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPLocalFootprintConfig(ctypes.Structure):
    _fields_ = [
        ("foot_lethal", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 3),
    ]


class PPScanMatchConfig(ctypes.Structure):
    _fields_ = [
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
        ("nt", ctypes.c_int32),
        ("xy_step", ctypes.c_int32),
        ("theta_step", ctypes.c_int32),
        ("min_cells", ctypes.c_int32),
        ("min_mean", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPObjectMaskConfig(ctypes.Structure):
    _fields_ = [
        ("min_score", ctypes.c_double),
        ("min_speed", ctypes.c_double),
        ("pad", ctypes.c_double),
        ("objects", ctypes.c_int32),
        ("confirmed_only", ctypes.c_int32),
        ("consumers", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PPGroundConfig(ctypes.Structure):
    _fields_ = [(n, ctypes.c_double) for n in ("max_range", "cand_z_max", "max_slope", "h_min", "h_max", "inlier_dist", "ground_dist",
                                               "overhead_max", "fallback_c")] + [
        ("seed", ctypes.c_uint64),
        ("hypotheses", ctypes.c_int32),
        ("min_inliers", ctypes.c_int32),
        ("refine", ctypes.c_int32),
        ("consumers", ctypes.c_int32),
    ]


class PPFrontierConfig(ctypes.Structure):
    _fields_ = [
        ("free_max", ctypes.c_int32),
        ("connectivity", ctypes.c_int32),
        ("min_size", ctypes.c_int32),
        ("max_frontiers", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("use_field", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 2),
    ]


class PPTrack(ctypes.Structure):
    _fields_ = [
        ("state", ctypes.c_double * 6),
        ("size", ctypes.c_double * 3),
        ("yaw", ctypes.c_double),
        ("score", ctypes.c_float),
        ("id", ctypes.c_int32),
        ("label", ctypes.c_int32),
        ("hits", ctypes.c_int32),
        ("misses", ctypes.c_int32),
        ("confirmed", ctypes.c_int32),
        ("det_row", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: cannot build libpp_hip.so")


_OBJ = os.path.join(_CSRC, "_obj" if _VARIANT == "libpp_hip" else "_obj_" + _VARIANT)
_EXTRA = os.environ.get("PP_HIPCC_EXTRA", "").split()


def _deps():
    """Every header of csrc/ (and the C-ABI header): a change to any of them rebuilds every translation unit."""
    return sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith(".h")) + [_INCLUDE]


def needs_build():
    if not os.path.exists(SO_PATH):
        return True
    t = os.path.getmtime(SO_PATH)
    deps = [os.path.join(_CSRC, s) for s in SOURCES] + _deps()
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_one(src, verbose):
    """One translation unit -> csrc/_obj/<name>.o (skipped when the object is newer than its inputs)."""
    obj = os.path.join(_OBJ, os.path.splitext(src)[0] + ".o")
    path = os.path.join(_CSRC, src)
    if os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in [path] + _deps()):
        return obj
    tmp = f"{obj}.{os.getpid()}.tmp"
    cmd = [_hipcc()] + [f for f in HIPCC_FLAGS if f != "-shared"] + _EXTRA + ["-c", "-o", tmp, path]
    if verbose:
        print(" ".join(cmd), flush=True)
    try:
        subprocess.check_call(cmd)
        os.replace(tmp, obj)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return obj


def build(force=False, verbose=False):
    """Compiles every HIP source for gfx950 (one object per translation unit, in parallel) and links
    <package>/libpp_hip.so."""
    if not force and not needs_build():
        return SO_PATH
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(_OBJ, exist_ok=True)
    if force:
        for f in os.listdir(_OBJ):
            os.remove(os.path.join(_OBJ, f))
    with ThreadPoolExecutor(max_workers=min(6, len(SOURCES))) as ex:
        objs = list(ex.map(lambda s: _compile_one(s, verbose), SOURCES))
    tmp = f"{SO_PATH}.{os.getpid()}.tmp.so"      # atomic: a concurrent loader never sees a half-written library
    cmd = [_hipcc(), "--offload-arch=gfx950", "-fPIC", "-shared", "-o", tmp] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    try:
        subprocess.check_call(cmd)
        os.replace(tmp, SO_PATH)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return SO_PATH


_lib = None


def _one_hip_runtime():
    """One HIP runtime per process, whatever the import order.  libpp_hip.so needs `libamdhip64.so.7`; the torch
    wheel bundles its own copy (same SONAME) that libtorch_hip.so asks for as plain `libamdhip64.so`.  torch imported
    first: its copy is mapped, the SONAME matches, libpp_hip.so binds to it.  libpp_hip.so first: the loader knows the
    system copy only as `libamdhip64.so.7`, a later `import torch` maps the bundled one beside it, and the runtime
    that initialises second finds no device (hipErrorNoDevice: "no ROCm-capable device is detected").  Loading the
    system library once under the plain name as well makes the later request resolve to the same mapping."""
    try:
        with open("/proc/self/maps") as f:
            if any("libamdhip64" in line for line in f):
                return
    except OSError:
        pass
    try:
        ctypes.CDLL("libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    except OSError:
        pass            # not on the default search path: libpp_hip.so's own RUNPATH still finds its runtime


def lib():
    """Loads libpp_hip.so (raises if absent -- the HIP path is the only path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for this path.")
    _one_hip_runtime()
    L = ctypes.CDLL(SO_PATH)
    vp, i32, i64, f32p = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    L.pp_abi_version.restype = ctypes.c_int
    L.pp_create.argtypes = [ctypes.POINTER(PPConfig), ctypes.c_int, ctypes.POINTER(vp)]
    L.pp_destroy.argtypes = [vp]
    L.pp_last_error.argtypes = [vp]
    L.pp_last_error.restype = ctypes.c_char_p
    L.pp_set_weight.argtypes = [vp, ctypes.c_char_p, f32p, ctypes.POINTER(i64), i32]
    L.pp_finalize_weights.argtypes = [vp]
    L.pp_set_anchors.argtypes = [vp, f32p, vp, i64]
    L.pp_points_to_voxel.argtypes = [vp, f32p, i64, f32p, vp, vp, ctypes.POINTER(i32)]
    L.pp_anchor_mask.argtypes = [vp, vp, i64, i32, vp]
    L.pp_forward_voxels.argtypes = [vp, f32p, vp, vp, i64, i32, f32p, f32p, f32p, f32p, f32p]
    L.pp_predict.argtypes = [vp, f32p, f32p, f32p, vp, f32p, f32p, i32, vp, vp]
    L.pp_upload_points.argtypes = [vp, f32p, vp, i32]
    L.pp_upload_points_async.argtypes = [vp, vp, vp, i32]
    L.pp_host_alloc.argtypes = [i64, ctypes.POINTER(vp)]
    L.pp_host_free.argtypes = [vp]
    L.pp_upload_points_device.argtypes = [vp, vp, vp, i32, vp]
    L.pp_current_batch.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pp_set_calib.argtypes = [vp, f32p, f32p, i32]
    L.pp_detect_async.argtypes = [vp]
    L.pp_sync.argtypes = [vp]
    L.pp_get_detections.argtypes = [vp, vp, vp]
    L.pp_set_gemm_precision.argtypes = [vp, i32]
    L.pp_get_gemm_precision.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_set_cache_budget.argtypes = [vp, i32]
    L.pp_detect.argtypes = [vp, f32p, vp, i32, f32p, f32p, vp, vp]
    L.pp_fetch_intermediates.argtypes = [vp, vp, vp, vp, vp, f32p, f32p, f32p, f32p]
    L.pp_set_profiling.argtypes = [vp, i32]
    L.pp_get_kernel_times.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float),
                                      ctypes.POINTER(i32)]
    L.pp_timer_start.argtypes = [vp]
    L.pp_timer_stop.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    L.pp_device_info.argtypes = [vp, ctypes.c_char_p, i32, ctypes.POINTER(i32), ctypes.POINTER(i64)]
    L.pp_device_copy_bench.argtypes = [vp, i64, i32, ctypes.POINTER(ctypes.c_float)]
    L.pp_device_mem_free.argtypes = [vp, ctypes.POINTER(i64)]
    L.pp_bench_layer.argtypes = [vp, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_float)]
    L.pp_layer_count.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_layer_tag.argtypes = [vp, i32]
    L.pp_layer_tag.restype = ctypes.c_char_p
    L.pp_plan_layer_name.argtypes = [ctypes.POINTER(PPLayerPlanDesc), i32, i32, ctypes.c_char_p, i32]
    L.pp_rotate_iou_eval.argtypes = [ctypes.c_int, f32p, i64, f32p, i64, i32, f32p]
    L.pp_d3_box_overlap.argtypes = [ctypes.c_int, vp, i64, vp, i64, i32, vp]
    L.pp_head_loss.argtypes = [vp, vp, f32p, i32, ctypes.POINTER(PPLossConfig), f32p, f32p]
    L.pp_train_layout.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i64), ctypes.POINTER(i64)]
    L.pp_train_layout_entry.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(i64), ctypes.POINTER(i64),
                                        ctypes.POINTER(i32)]
    L.pp_train_step.argtypes = [vp, vp, vp, vp, vp, f32p, i32, ctypes.POINTER(PPLossConfig), f32p]
    L.pp_train_step_async.argtypes = [vp, vp, vp, vp, vp, f32p, i32, ctypes.POINTER(PPLossConfig)]
    L.pp_train_step_wait.argtypes = [vp, f32p]
    L.pp_stream.argtypes = [vp, ctypes.POINTER(vp)]
    L.pp_train_graph_stats.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pp_train_fetch_decisions.argtypes = [vp, i32, vp, i64, ctypes.POINTER(i64)]
    L.pp_assign_targets.argtypes = [vp, f32p, vp, vp, i32, vp, ctypes.POINTER(PPTargetConfig), vp, f32p, vp, f32p]
    L.pp_train_step_gt_async.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                         ctypes.POINTER(PPTargetConfig)]
    L.pp_train_step_gt.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                   ctypes.POINTER(PPTargetConfig), f32p]
    L.pp_augment.argtypes = [vp, f32p, vp, vp, vp, i32, ctypes.POINTER(PPAugmentConfig), vp, vp, f32p, f32p, vp, vp]
    L.pp_train_step_aug_async.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                          ctypes.POINTER(PPTargetConfig), vp, ctypes.POINTER(PPAugmentConfig), vp, vp]
    L.pp_train_step_aug.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                    ctypes.POINTER(PPTargetConfig), vp, ctypes.POINTER(PPAugmentConfig), vp, vp, f32p]
    L.pp_augment_selected.argtypes = [vp, vp, i64, ctypes.POINTER(i64)]
    L.pp_adamw_step_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, i64, ctypes.c_float, ctypes.c_float,
                                       ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.pp_train_set_frozen.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), i32]
    L.pp_adamw_step_segments_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, vp, i32, ctypes.c_float,
                                                ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.pp_gtdb_load.argtypes = [vp, f32p, vp, vp, vp, i64]
    L.pp_gt_sample.argtypes = [vp, f32p, vp, vp, vp, i32, ctypes.POINTER(PPGtSampleConfig), vp, vp, f32p, i64, vp, f32p,
                               vp, vp, vp]
    L.pp_gt_sample_info.argtypes = [vp, vp, vp, vp, i32]
    L.pp_train_step_sample_async.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                             ctypes.POINTER(PPTargetConfig), vp, ctypes.POINTER(PPGtSampleConfig), vp, vp,
                                             ctypes.POINTER(PPAugmentConfig), vp, vp]
    L.pp_train_step_sample.argtypes = [vp, vp, vp, vp, f32p, vp, vp, i32, ctypes.POINTER(PPLossConfig),
                                       ctypes.POINTER(PPTargetConfig), vp, ctypes.POINTER(PPGtSampleConfig), vp, vp,
                                       ctypes.POINTER(PPAugmentConfig), vp, vp, f32p]
    L.pp_ingest_pointcloud2.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig), f32p, i64]
    L.pp_ingest_pointcloud2_async.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig)]
    L.pp_ingest_info.argtypes = [vp, vp, vp, i32]
    L.pp_ingest_depth.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig), f32p, i64]
    L.pp_ingest_depth_async.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig)]
    for name in ("pp_ingest_rig_depth", "pp_ingest_rig_pointcloud2"):      # (cfgs: an array of PPIngestConfig)
        getattr(L, name).argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, f32p, i64]
        getattr(L, name + "_async").argtypes = [vp, vp, vp, vp, vp, vp, i32, i32]
    L.pp_ingest_rig_info.argtypes = [vp, vp, vp, i32]
    # (features: an array of PPPc2Feature, [frames or sources][nfeat])
    L.pp_ingest_pointcloud2_fields.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig), vp, i32, f32p, i64]
    L.pp_ingest_pointcloud2_fields_async.argtypes = [vp, vp, vp, vp, i32, ctypes.POINTER(PPIngestConfig), vp, i32]
    L.pp_ingest_rig_pointcloud2_fields.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, f32p, i64]
    L.pp_ingest_rig_pointcloud2_fields_async.argtypes = [vp, vp, vp, vp, vp, vp, i32, i32, vp, i32]
    L.pp_gtdb_build.argtypes = [vp, vp, vp, i32, vp, vp, f32p, i64]
    L.pp_gtdb_count.argtypes = [vp, vp, vp, i32, vp]
    L.pp_eval_match.argtypes = [ctypes.c_int, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp]
    L.pp_eval_pr.argtypes = [ctypes.c_int, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp,
                             vp, vp]
    L.pp_frustum_crop.argtypes = [vp, vp, i32, i32, vp, f32p, i64]
    L.pp_frustum_crop_async.argtypes = [vp, vp, i32, i32]
    L.pp_frustum_crop_info.argtypes = [vp, vp, i32]
    L.pp_set_sweeps.argtypes = [vp, ctypes.POINTER(PPSweepConfig)]
    L.pp_get_sweeps.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPSweepConfig)]
    L.pp_sweeps_accumulate.argtypes = [vp, vp, vp, i32, vp, f32p, i64]
    L.pp_sweeps_accumulate_async.argtypes = [vp, vp, vp, i32]
    L.pp_sweeps_info.argtypes = [vp, vp, vp, vp, vp, i32]
    L.pp_sweeps_reset.argtypes = [vp, i32]
    L.pp_set_local_footprint.argtypes = [vp, i32, ctypes.POINTER(PPLocalFootprintConfig), vp, i32]
    L.pp_get_local_footprint_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPLocalFootprintConfig), vp, ctypes.POINTER(i32)]
    L.pp_get_local_footprint.argtypes = [vp, i32, vp, i32]
    L.pp_local_plan_grids_footprint.argtypes = [ctypes.c_int, vp, vp, i32, i32, i32, ctypes.POINTER(PPNavfnConfig),
                                                ctypes.POINTER(PPLocalPlanConfig), vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, i32,
                                                vp, vp, vp, vp, vp, vp]
    L.pp_set_nms_mode.argtypes = [vp, i32]
    L.pp_get_nms_mode.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_rotate_nms.argtypes = [ctypes.c_int, f32p, i64, ctypes.c_float, i32, i32, vp, ctypes.POINTER(i64)]
    L.pp_set_soft_nms.argtypes = [vp, i32, ctypes.c_float, ctypes.c_float]
    L.pp_get_soft_nms.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    L.pp_soft_nms.argtypes = [ctypes.c_int, f32p, i64, i32, ctypes.c_float, ctypes.c_float, ctypes.c_float, i32, i32, vp, vp,
                              ctypes.POINTER(i64)]
    L.pp_set_tracking.argtypes = [vp, ctypes.POINTER(PPTrackConfig)]
    L.pp_get_tracking.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPTrackConfig)]
    L.pp_set_track_dt.argtypes = [vp, vp, i32]
    L.pp_get_tracks.argtypes = [vp, vp, vp, vp]
    L.pp_track_update.argtypes = [vp, vp, vp, i32, i32, vp]
    L.pp_track_reset.argtypes = [vp, i32]
    L.pp_track_info.argtypes = [vp, vp, vp, vp]
    L.pp_set_track_pose.argtypes = [vp, vp, i32]
    L.pp_get_tracks_fixed.argtypes = [vp, vp, vp]
    L.pp_set_costmap.argtypes = [vp, ctypes.POINTER(PPCostmapConfig)]
    L.pp_get_costmap_config.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPCostmapConfig)]
    L.pp_costmap_async.argtypes = [vp]
    L.pp_get_costmaps.argtypes = [vp, vp, vp, i32]
    L.pp_costmap_info.argtypes = [vp, vp, vp, i32]
    L.pp_set_occupancy.argtypes = [vp, ctypes.POINTER(PPOccupancyConfig), vp, i32]
    L.pp_get_occupancy_config.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPOccupancyConfig)]
    L.pp_occupancy_update_async.argtypes = [vp, vp, i32]
    L.pp_get_occupancy.argtypes = [vp, vp, vp, vp, i32]
    L.pp_occupancy_info.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
    L.pp_occupancy_reset.argtypes = [vp, i32]
    L.pp_set_inflation.argtypes = [vp, i32, ctypes.POINTER(PPInflationConfig), vp, i32]
    L.pp_get_inflation_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPInflationConfig)]
    L.pp_inflate_async.argtypes = [vp, i32]
    L.pp_get_inflated.argtypes = [vp, i32, vp, vp, i32]
    L.pp_inflation_info.argtypes = [vp, i32, vp, vp, i32]
    L.pp_inflate_grids.argtypes = [ctypes.c_int, vp, i32, i32, i32, ctypes.POINTER(PPInflationConfig), vp, i32, vp, vp, vp]
    L.pp_set_navfn.argtypes = [vp, i32, ctypes.POINTER(PPNavfnConfig)]
    L.pp_get_navfn_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPNavfnConfig)]
    L.pp_navfn_async.argtypes = [vp, i32, vp, vp, i32]
    L.pp_get_navfn.argtypes = [vp, i32, vp, vp, vp, i32]
    L.pp_navfn_info.argtypes = [vp, i32, vp, vp, vp, vp, i32]
    L.pp_navfn_grids.argtypes = [ctypes.c_int, vp, i32, i32, i32, ctypes.POINTER(PPNavfnConfig), vp, vp, vp, vp, vp, vp]
    L.pp_set_local_plan.argtypes = [vp, i32, ctypes.POINTER(PPLocalPlanConfig), vp, i32]
    L.pp_get_local_plan_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPLocalPlanConfig)]
    L.pp_local_plan_async.argtypes = [vp, i32, vp, vp, i32]
    L.pp_get_local_plan.argtypes = [vp, i32, vp, vp, vp, vp, i32]
    L.pp_local_plan_grids.argtypes = [ctypes.c_int, vp, vp, i32, i32, i32, ctypes.POINTER(PPNavfnConfig),
                                      ctypes.POINTER(PPLocalPlanConfig), vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.pp_set_local_movers.argtypes = [vp, i32, ctypes.POINTER(PPLocalMoverConfig)]
    L.pp_get_local_movers_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPLocalMoverConfig)]
    L.pp_local_plan_movers_async.argtypes = [vp, i32, vp, vp, vp, i32]
    L.pp_get_local_movers.argtypes = [vp, i32, vp, vp, i32]
    L.pp_local_plan_grids_movers.argtypes = [ctypes.c_int, vp, vp, i32, i32, i32, ctypes.POINTER(PPNavfnConfig),
                                             ctypes.POINTER(PPLocalPlanConfig), vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.pp_set_scan_match.argtypes = [vp, ctypes.POINTER(PPScanMatchConfig), vp, i32]
    L.pp_get_scan_match_config.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPScanMatchConfig)]
    L.pp_scan_match_async.argtypes = [vp, vp, i32]
    L.pp_get_scan_match.argtypes = [vp, vp, vp, i32]
    L.pp_scan_match_grids.argtypes = [ctypes.c_int, vp, vp, i32, i32, i32, vp, vp, i32, vp, vp, vp,
                                      ctypes.POINTER(PPOccupancyConfig), ctypes.POINTER(PPScanMatchConfig), vp, i32, vp, vp]
    L.pp_set_frontier.argtypes = [vp, i32, ctypes.POINTER(PPFrontierConfig)]
    L.pp_get_frontier_config.argtypes = [vp, i32, ctypes.POINTER(i32), ctypes.POINTER(PPFrontierConfig)]
    L.pp_frontier_async.argtypes = [vp, i32, vp, i32]
    L.pp_get_frontiers.argtypes = [vp, i32, vp, vp, vp, i32]
    L.pp_frontier_grids.argtypes = [ctypes.c_int, vp, vp, i32, i32, i32, ctypes.POINTER(PPFrontierConfig), vp, vp, vp, vp]
    L.pp_set_projection.argtypes = [vp, vp, i32]
    L.pp_get_projection.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_get_bboxes.argtypes = [vp, vp]
    L.pp_box3d_to_bbox.argtypes = [ctypes.c_int, vp, vp, i32, vp, vp]
    L.pp_set_class_nms.argtypes = [vp, i32]
    L.pp_get_class_nms.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_get_detection_rows.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_head_metrics.argtypes = [vp, vp, i32, f32p, vp]
    L.pp_set_train_metrics.argtypes = [vp, i32]
    L.pp_get_train_metrics_enabled.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_get_train_metrics.argtypes = [vp, vp]
    L.pp_grad_clip_workspace_bytes.argtypes = [i64, i32, i32, ctypes.POINTER(i64)]
    L.pp_grad_norm_device.argtypes = [ctypes.c_int, vp, vp, i64, vp, i32, vp, i32, vp]
    L.pp_set_object_mask.argtypes = [vp, ctypes.POINTER(PPObjectMaskConfig)]
    L.pp_get_object_mask_config.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPObjectMaskConfig)]
    L.pp_object_mask_async.argtypes = [vp, vp, vp, i32]
    L.pp_object_mask_shape.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pp_get_object_mask.argtypes = [vp, vp, vp, i32]
    L.pp_occupancy_masked.argtypes = [vp, vp, i32]
    L.pp_object_mask_points.argtypes = [ctypes.c_int, vp, vp, i32, i32, vp, vp, ctypes.c_double, vp, i32, vp]
    L.pp_set_ground.argtypes = [vp, ctypes.POINTER(PPGroundConfig)]
    L.pp_get_ground_config.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(PPGroundConfig)]
    L.pp_ground_async.argtypes = [vp, vp, i32]
    L.pp_ground_used.argtypes = [vp, ctypes.POINTER(i32)]
    L.pp_ground_shape.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.pp_get_ground.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32]
    L.pp_ground_points.argtypes = [ctypes.c_int, vp, vp, i32, i32, ctypes.POINTER(PPGroundConfig), vp, vp, vp, vp, vp, i32, vp, vp]
    L.pp_adamw_step_clipped_device.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp, i64, vp, i32, vp, i32,
                                               ctypes.POINTER(PPGradClipConfig), vp, ctypes.c_float, ctypes.c_float,
                                               ctypes.c_float, ctypes.c_float, ctypes.c_float]
    L.pp_publish_train_weights.argtypes = [vp, vp, vp]
    L.pp_publish_info.argtypes = [vp, ctypes.POINTER(PPPublishStats)]
    for name in EXPORTS:
        fn = getattr(L, name)  # raises AttributeError if the symbol is not exported
        if name not in ("pp_last_error", "pp_layer_tag"):
            fn.restype = ctypes.c_int
    _lib = L
    return L
