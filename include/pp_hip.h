/* pp_hip.h -- C-ABI of the MI355X-native PointPillars inference path (libpp_hip.so).
 *
 * This is the drop-in boundary for the hot path of
 * krullgit/3D-Object-Detection-for-autonomous-navigation's `train.py evaluate`
 * (reference paths below are relative to that repository).  The reference has
 * no FFI for this path -- its callers are Python call sites
 * -- so each entry point names the Python interface it replaces; the binding a
 * maintainer adds on the reference side is the ctypes stub in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no framework types.  Every pointer is a
 *     HOST pointer unless its parameter is documented "device pointer".
 *   - integer status codes (PP_OK == 0); no exceptions cross the ABI; the text
 *     of the last failure is returned by pp_last_error().
 *   - one handle per GPU; a handle is not thread-safe; distinct handles are
 *     fully independent (own stream, own device workspaces sized at create
 *     for max_batch x max_points_per_frame).
 *   - every compute entry point runs on the GPU (gfx950).  There is no CPU
 *     fallback: without a device, pp_create fails.
 */
#ifndef PP_HIP_H
#define PP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: PP_ERR_NUMERIC, pp_set_gemm_precision / pp_get_gemm_precision, pp_set_cache_budget.  4: pp_train_fetch_decisions;
 * later additions within 4 (nothing before them changed): pp_target_config, pp_assign_targets, pp_train_step_gt_async,
 * pp_train_step_gt; then PP_AUG_MAX_TRY, pp_augment_config, pp_aug_frame, pp_augment, pp_train_step_aug_async,
 * pp_train_step_aug, pp_augment_selected; then pp_train_set_frozen, pp_adamw_step_segments_device; then PP_GTS_MAX_CAND,
 * PP_GTS_MAX_ROUNDS, pp_gt_sample_config, pp_gts_cand, pp_gtdb_load, pp_gt_sample, pp_gt_sample_info,
 * pp_train_step_sample_async, pp_train_step_sample; then pp_pc2_layout, pp_ingest_config, pp_ingest_pointcloud2,
 * pp_ingest_pointcloud2_async, pp_ingest_info; then pp_gtdb_build, pp_gtdb_count; then PP_CROP_BACK, pp_frustum_crop,
 * pp_frustum_crop_async, pp_frustum_crop_info; then pp_nms_mode, pp_set_nms_mode, pp_get_nms_mode, PP_RNMS_MAX_BOXES,
 * pp_rotate_nms; then pp_set_projection, pp_get_projection, pp_get_bboxes, pp_box3d_to_bbox; then pp_class_nms,
 * pp_set_class_nms, pp_get_class_nms, pp_get_detection_rows; then PP_METRICS_COUNTS, pp_head_metrics,
 * pp_set_train_metrics, pp_get_train_metrics_enabled, pp_get_train_metrics; then pp_grad_clip_mode, pp_grad_clip_config,
 * pp_grad_clip_workspace_bytes, pp_grad_norm_device, pp_adamw_step_clipped_device; then pp_publish_stats,
 * pp_publish_train_weights, pp_publish_info; then PP_NMS_SOFT, pp_soft_nms_method, pp_set_soft_nms, pp_get_soft_nms,
 * PP_SNMS_MAX_BOXES, pp_soft_nms.  Then PP_DEPTH_U16, PP_DEPTH_F32, pp_depth_layout, pp_ingest_depth,
 * pp_ingest_depth_async (declared behind pp_ingest_info, whose counts serve both feeds).  Then PP_RIG_MAX_SOURCES,
 * pp_ingest_rig_depth, pp_ingest_rig_depth_async, pp_ingest_rig_pointcloud2, pp_ingest_rig_pointcloud2_async,
 * pp_ingest_rig_info.  Then pp_pc2_feature, pp_ingest_pointcloud2_fields, pp_ingest_pointcloud2_fields_async,
 * pp_ingest_rig_pointcloud2_fields, pp_ingest_rig_pointcloud2_fields_async (declared behind pp_ingest_rig_info).  Then
 * PP_TRACK_MAX, pp_track_config, pp_track, pp_set_tracking, pp_get_tracking, pp_set_track_dt, pp_get_tracks,
 * pp_track_update, pp_track_reset, pp_track_info.  Then PP_SWEEP_MAX, pp_sweep_config, pp_set_sweeps, pp_get_sweeps,
 * pp_sweeps_accumulate, pp_sweeps_accumulate_async, pp_sweeps_info, pp_sweeps_reset (declared behind
 * pp_frustum_crop_info: the stage sits where the crop sits).  Then pp_set_track_pose, pp_get_tracks_fixed (declared
 * behind pp_track_info).  Then PP_COSTMAP_MAX_STEPS, PP_COSTMAP_MAX_CELLS, pp_costmap_config, pp_set_costmap,
 * pp_get_costmap_config, pp_costmap_async, pp_get_costmaps, pp_costmap_info (declared behind pp_get_tracks_fixed: the
 * stage reads what a pass and its tracking step leave on the device).  Then PP_OCC_MAX_CELLS, pp_occupancy_config,
 * pp_set_occupancy, pp_get_occupancy_config, pp_occupancy_update_async, pp_get_occupancy, pp_occupancy_info,
 * pp_occupancy_reset (declared behind pp_costmap_info).  Then pp_layer_plan_desc, pp_plan_layer_name (declared behind
 * pp_layer_tag).  Then PP_INFLATE_MAX_RADIUS, pp_inflation_config, PP_INFLATE_COSTMAP, PP_INFLATE_OCCUPANCY,
 * pp_set_inflation, pp_get_inflation_config, pp_inflate_async, pp_get_inflated, pp_inflation_info, pp_inflate_grids
 * (declared behind pp_occupancy_reset: the stage reads the grid either stage leaves on the device).  Then
 * PP_ERR_INTERNAL, PP_NAVFN_UNREACHED, PP_NAVFN_MAX_PATH, pp_navfn_config, pp_set_navfn, pp_get_navfn_config,
 * pp_navfn_async, pp_get_navfn, pp_navfn_info, pp_navfn_grids (declared behind pp_inflate_grids: the stage reads the
 * inflated grid where it lies).  Then PP_LOCAL_SUB, PP_LOCAL_HEADINGS, PP_LOCAL_MAX_SAMPLES, PP_LOCAL_MAX_STEPS,
 * PP_LOCAL_MAX_LOOKAHEAD, PP_LOCAL_RESULT, pp_local_plan_config, pp_set_local_plan, pp_get_local_plan_config,
 * pp_local_plan_async, pp_get_local_plan, pp_local_plan_grids (declared behind pp_navfn_grids: the stage reads the
 * inflated grid and the field where they lie).  Then PP_LOCAL_MAX_MOVERS, PP_LOCAL_MAX_MOVER_SPEED,
 * PP_LOCAL_MAX_MOVER_RADIUS, PP_LOCAL_MOVER_INFO, pp_local_mover_config, pp_set_local_movers, pp_get_local_movers_config,
 * pp_local_plan_movers_async, pp_get_local_movers, pp_local_plan_grids_movers (declared behind pp_local_plan_grids).  Then
 * PP_SCAN_MAX_CANDIDATES, PP_SCAN_RESULT, pp_scan_status, pp_scan_match_config, pp_set_scan_match,
 * pp_get_scan_match_config, pp_scan_match_async, pp_get_scan_match, pp_scan_match_grids (declared behind
 * pp_local_plan_grids_movers: the stage reads the occupancy maps' log-odds where they lie).  Then PP_FRONTIER_MAX,
 * PP_FRONTIER_INFO, PP_FRONTIER_NONE, pp_frontier_config, pp_set_frontier, pp_get_frontier_config, pp_frontier_async,
 * pp_get_frontiers, pp_frontier_grids (declared behind pp_scan_match_grids: the stage reads the inflated grid, and under
 * use_field the navigation function's field, where they lie).  Then PP_LOCAL_MAX_PROBES, PP_LOCAL_MAX_PROBE,
 * PP_LOCAL_FOOT_INFO, pp_local_footprint_config, pp_set_local_footprint, pp_get_local_footprint_config,
 * pp_get_local_footprint, pp_local_plan_grids_footprint (declared behind pp_local_plan_grids_movers: the footprint rides
 * in the local planner's rollout).  Then PP_OBJMASK_MAX_FOOTPRINTS, PP_OBJMASK_INFO, PP_OBJMASK_OCCUPANCY,
 * PP_OBJMASK_SCAN_MATCH, PP_OBJMASK_COSTMAP, pp_object_mask_config, pp_set_object_mask, pp_get_object_mask_config,
 * pp_object_mask_async, pp_object_mask_shape, pp_get_object_mask, pp_occupancy_masked, pp_object_mask_points (declared
 * behind pp_frontier_grids: the stage reads what a pass and its tracking step leave, and the three readers of the
 * resident rows read its bits).  Then PP_GROUND_MAX_HYP, PP_GROUND_INFO, PP_GROUND_OCCUPANCY, PP_GROUND_SCAN_MATCH,
 * PP_GROUND_COSTMAP, pp_ground_config, pp_set_ground, pp_get_ground_config, pp_ground_async, pp_ground_used, pp_ground_shape,
 * pp_get_ground, pp_ground_points (declared behind pp_object_mask_points: the same three readers read its two bit planes). */
#define PP_ABI_VERSION 4

enum pp_status {
    PP_OK = 0,
    PP_ERR_ARG = 1,    /* null / out-of-range argument */
    PP_ERR_STATE = 2,  /* call order: weights or anchors not set */
    PP_ERR_HIP = 3,    /* a HIP runtime call failed (see pp_last_error) */
    PP_ERR_SHAPE = 4,  /* tensor shape does not match the configuration */
    PP_ERR_UNSUPPORTED = 5,
    PP_ERR_NUMERIC = 6, /* non-finite head outputs: pp_get_detections / pp_detect / pp_predict never hand out NaN boxes */
    PP_ERR_INTERNAL = 7 /* a bound the library proves was passed all the same (pp_get_navfn: more rounds than cells) */
};

/* GEMM arithmetic of the backbone (pp_set_gemm_precision) */
enum pp_gemm_precision {
    PP_PREC_SPLIT_F16 = 0, /* default: fp32 results on the 16-bit matrix pipe, every operand as two float16 pieces.
                            * Needs |BN-folded weight| < 32768 (checked per layer at pp_finalize_weights: a layer that
                            * fails runs in PP_PREC_F32 by itself) and |activation| < 65504 (checked on the device:
                            * a frame whose activations leave the range ends in PP_ERR_NUMERIC) */
    PP_PREC_F32 = 1        /* every layer on the float32 matrix instruction (v_mfma_f32_32x32x2_f32): float32's range */
};

/* Suppression rule of the detector's post-process (pp_set_nms_mode) */
enum pp_nms_mode {
    PP_NMS_STANDUP = 0, /* default, the reference's predict(): the stand-up axis-aligned box of every decoded box, `+1` on
                         * widths measured in metres (iou_device) -- boxes within about 0.6 m of each other count as
                         * IoU > 0.5 */
    PP_NMS_ROTATED = 1, /* rotate_nms_kernel's rule (second/core/non_max_suppression/nms_gpu.py:419-452, shipped by the
                         * reference but never wired in): devRotateIoU of the decoded [x, y, w, l, r] */
    PP_NMS_SOFT = 2     /* soft_nms_jit's rule (second/core/non_max_suppression/nms_cpu.py:79-169, compiled by the reference
                         * but never called) on the stand-up boxes and their `+1` overlap: a neighbour of a selected box is
                         * not deleted, its score is decayed by the overlap (pp_set_soft_nms) and the caller's score cut
                         * decides */
};

/* How PP_NMS_SOFT and pp_soft_nms decay the score of a box that overlaps a selected one by `ov` (the reference's `method`
 * values; Nt is the IoU threshold) */
enum pp_soft_nms_method {
    PP_SOFT_NMS_HARD = 0,     /* ov > Nt ? 0 : 1 -- with a floor above 0 the greedy rule */
    PP_SOFT_NMS_LINEAR = 1,   /* ov > Nt ? 1 - ov : 1 */
    PP_SOFT_NMS_GAUSSIAN = 2  /* exp(-ov * ov / sigma) */
};

/* How the detector's post-process treats more than one class (pp_set_class_nms) */
enum pp_class_nms {
    PP_CLASS_NMS_JOINT = 0,     /* default, the reference's predict() (model/voxelnet.py:1172-1286): an anchor's score is
                                 * its largest class score, its label the argmax; one top-100 and one suppression pass
                                 * serve all classes together */
    PP_CLASS_NMS_PER_CLASS = 1  /* model.second.use_multi_class_nms, the branch the reference leaves as `pass`
                                 * (model/voxelnet.py:1170-1171): the same pass once per class on that class's score
                                 * alone -- threshold, top-100, suppression and both caps per class */
};

typedef struct pp_engine* pp_handle;

/* Mirrors the keys the reference's hot path reads from configs/train.yaml
 * (SURVEY.md section 5 "Config / flag system"; values of the shipped config in
 * SURVEY Appendix B). */
typedef struct pp_config {
    double pc_range[6];   /* model.second.voxel_generator.point_cloud_range: xmin ymin zmin xmax ymax zmax */
    double voxel_size[3]; /* ...voxel_size (float64, as load_data.py:2573-2574 builds them) */
    int32_t max_points;   /* ...max_number_of_points_per_voxel  (T) */
    int32_t max_voxels;   /* ...max_number_of_voxels */
    int32_t num_point_features; /* model.second.num_point_features (F: 3 or 4) */
    int32_t pfn_filters;  /* voxel_feature_extractor.num_filters (C) */
    int32_t layer_nums[3];            /* rpn.layer_nums */
    int32_t layer_strides[3];         /* rpn.layer_strides */
    int32_t num_filters[3];           /* rpn.num_filters */
    int32_t upsample_strides[3];      /* rpn.upsample_strides */
    int32_t num_upsample_filters[3];  /* rpn.num_upsample_filters */
    int32_t num_anchor_per_loc;       /* len(rotations) * len(sizes) */
    int32_t num_class;                /* model.second.num_class.  1 in the shipped config; > 1 is an extension the
                                         reference leaves as a TF stub (model/voxelnet.py:1183-1185): score = max,
                                         label = argmax over the class logits of an anchor; the fused head row must
                                         hold num_anchor_per_loc * (7 + num_class + 2) <= 32 columns */
    int32_t nms_pre_max_size;         /* model.second.nms_pre_max_size */
    int32_t nms_post_max_size;        /* model.second.nms_post_max_size */
    float nms_score_threshold;        /* model.second.nms_score_threshold */
    float nms_iou_threshold;          /* model.second.nms_iou_threshold */
    float anchor_area_threshold;      /* eval_input_reader.anchor_area_threshold */
    int32_t max_batch;                /* frames per call the workspaces are sized for */
    int32_t max_points_per_frame;     /* points per frame the workspaces are sized for */
    int32_t use_direction_classifier; /* model.second.use_direction_classifier (model/voxelnet.py:690,714,1093,1297):
                                         0 = no conv_dir_cls head, no direction flip */
    int32_t with_distance;            /* voxel_feature_extractor.with_distance (model/pointpillars.py:185-188): one more
                                         PFN input feature, the point's Euclidean norm */
} pp_config;

/* One detection, in NMS keep order (descending score), as VoxelNet.predict
 * assembles it (model/voxelnet.py:1281-1369). */
typedef struct pp_detection {
    double box3d_camera[7]; /* x y z l h w r, float64 as box_lidar_to_camera returns (eval_helper_functions.py:735-740) */
    float box3d_lidar[7];   /* x y z w l h r after the direction flip (model/voxelnet.py:1305-1310) */
    float score;            /* sigmoid(cls) (model/voxelnet.py:1150) */
    int32_t label;          /* label_preds: argmax over the class logits (0 when num_class == 1) */
    int32_t dir_label;      /* argmax of the direction head */
    int32_t anchor_index;   /* flat anchor index (y, x, rot) of the source anchor */
    int32_t reserved;
} pp_detection;

/* ---- lifetime -------------------------------------------------------- */

/* Replaces VoxelNet.__init__ (model/voxelnet.py:727-787) + the dataloader's
 * per-config constants.  Fails with PP_ERR_HIP when no gfx950 device `device`
 * is usable. */
int pp_create(const pp_config* cfg, int device, pp_handle* out);
int pp_destroy(pp_handle h);
/* Text of the last failure on `h` (or of the last pp_create failure when h is NULL). */
const char* pp_last_error(pp_handle h);
int pp_abi_version(void);

/* ---- weights: replaces net.load_weights (train.py:731-734) ------------ */

/* One named float32 tensor in the Keras layout (names / layouts listed in
 * INTEGRATION.md and <package>/weights.py).  The data is copied. */
int pp_set_weight(pp_handle h, const char* name, const float* data, const int64_t* shape, int32_t ndim);
/* Verifies that every tensor is present, folds BatchNorm (eps 1e-3) into the
 * following GEMM and uploads the kernel-side layouts. */
int pp_finalize_weights(pp_handle h);

/* Static anchors [A,7] (x y z w l h r) in the reference's (y, x, rot) order and
 * their clamped integral-image cells [A,4] (x0 y0 x1 y1), built once on the
 * host (replaces the per-frame generate_anchors / rbbox2d_to_near_bbox calls,
 * load_data.py:3029-3043). */
int pp_set_anchors(pp_handle h, const float* anchors, const int32_t* cells, int64_t num_anchors);

/* ---- stage entry points (parity checkpoints) -------------------------- */
/* These reuse the device buffers of the fused path: after any of them the handle holds no resident frames
 * and no fused-path results (pp_detect_async / pp_get_detections / pp_fetch_intermediates then return
 * PP_ERR_STATE until the next upload + detect). */

/* points_to_voxel(points, voxel_size, coors_range, max_points, True, max_voxels)
 * (load_data.py:695-771) for ONE frame of n points [n,F].  Outputs are sized
 * by the caller for max_voxels pillars: voxels [max_voxels,T,F] (only the
 * first *n_pillars rows are written, zero padded), coors [max_voxels,3] (z y x),
 * num_points [max_voxels]. */
int pp_points_to_voxel(pp_handle h, const float* points, int64_t n, float* voxels, int32_t* coors,
                       int32_t* num_points, int32_t* n_pillars);

/* The dataloader's anchors_mask for `batch` frames (load_data.py:3043-3072)
 * from batched pillar coordinates coors [P,4] (b z y x).  mask [batch,A] u8. */
int pp_anchor_mask(pp_handle h, const int32_t* coors, int64_t num_pillars, int32_t batch, uint8_t* mask);

/* VoxelNet.__call__(voxels, num_points, coors, batch_anchors) eval branch
 * (model/voxelnet.py:850-916): voxels [P,T,F], num_points [P], coors [P,4]
 * (b z y x, unique per frame as points_to_voxel produces them).  Outputs NHWC:
 * box_preds [batch,H',W',2*7], cls_preds [batch,H',W',2], dir_cls_preds
 * [batch,H',W',4].  Optional checkpoints (may be NULL): pillar_features [P,C]
 * (PillarFeatureNet output) and canvas [batch,ny,nx,C] (PointPillarsScatter
 * output, NHWC). */
int pp_forward_voxels(pp_handle h, const float* voxels, const int32_t* num_points, const int32_t* coors,
                      int64_t num_pillars, int32_t batch, float* box_preds, float* cls_preds,
                      float* dir_cls_preds, float* pillar_features, float* canvas);

/* VoxelNet.predict(example, preds_dict) (model/voxelnet.py:1060-1390) on the
 * head maps.  anchors_mask [batch,A] u8; rect, trv2c [batch,16] row-major 4x4.
 * dets [batch * nms_post_max_size] (pp_get_detection_rows rows per frame after
 * pp_set_class_nms); n_dets [batch] (0 == the reference's all-None dict). */
int pp_predict(pp_handle h, const float* box_preds, const float* cls_preds, const float* dir_cls_preds,
               const uint8_t* anchors_mask, const float* rect, const float* trv2c, int32_t batch,
               pp_detection* dets, int32_t* n_dets);

/* ---- fused path: raw points -> detections ----------------------------- */

/* Copies `batch` frames of raw points into the engine's device input buffer.
 * points: concatenated [sum n_b, F]; frame_offsets [batch+1] (row offsets). */
int pp_upload_points(pp_handle h, const float* points, const int32_t* frame_offsets, int32_t batch);
/* Same without waiting: `points_pinned` must be page-locked host memory (pp_host_alloc, or the caller's own
 * hipHostMalloc / hipHostRegister) and must stay unchanged until the copy has run (pp_sync after the
 * pp_detect_async that consumes these frames).  frame_offsets is copied before the call returns.
 * The handle's input is double-buffered and this copy runs on the handle's own copy stream into the buffer
 * the pass in flight is not reading, so the upload of batch k+1 proceeds beside the kernels of batch k:
 *     upload_async(k+1); sync + get_detections (batch k); detect_async (batch k+1); ...
 * pp_detect_async orders itself behind the copy.  This is the double-buffered feed of raw points that replaces
 * the per-frame host-to-device hand-over of train.py:748.
 * Batches of up to 4 frames (the latency case) are not copied at all: the call only fills a page-locked descriptor
 * and the next pass's first kernel reads offsets and points straight from `points_pinned` over the host link while
 * it writes the device copies the later kernels use -- no copy-engine transfer, no event chain (batch 1, upload
 * included: 0.29 -> 0.25 ms).  `points_pinned` must then be device-mapped page-locked memory (pp_host_alloc and
 * hipHostMalloc are; memory that is not falls back to the copy). */
int pp_upload_points_async(pp_handle h, const float* points_pinned, const int32_t* frame_offsets, int32_t batch);
/* Page-locked host memory for the staging buffers above (stateless; any thread). */
int pp_host_alloc(int64_t bytes, void** out);
int pp_host_free(void* p);
/* Same, from a DEVICE pointer `points_dev` (device-to-device copy on the engine's stream, no wait).
 * Ordering contract: `producer_stream` is the hipStream_t on which the work that writes `points_dev` was
 * queued (the engine's stream then waits for an event recorded there), or NULL when that work has already
 * completed (the caller synchronised).  `points_dev` must stay valid until the engine's stream has passed
 * the copy. */
int pp_upload_points_device(pp_handle h, const void* points_dev, const int32_t* frame_offsets, int32_t batch,
                            void* producer_stream);
/* Frames currently resident for pp_detect_async (`uploaded`) and frames of the last enqueued
 * pp_detect_async whose results pp_get_detections returns (`results`); 0 after a stage entry point reused
 * the buffers.  Either pointer may be NULL. */
int pp_current_batch(pp_handle h, int32_t* uploaded, int32_t* results);
/* Calibration for the uploaded frames: rect, trv2c [batch,16]. */
int pp_set_calib(pp_handle h, const float* rect, const float* trv2c, int32_t batch);

/* Enqueues the whole path (a1..a12 of SURVEY section 8a) for the frames resident in
 * the engine's input buffer on the engine's stream: voxelise -> PFN + scatter
 * -> anchor mask -> backbone + heads -> top-k / decode / NMS -> detections in
 * device memory, then an async copy into the engine's pinned result buffer.
 * Returns without waiting. */
int pp_detect_async(pp_handle h);
/* Waits for the engine's stream. */
int pp_sync(pp_handle h);
/* Copies the results of the last pp_detect_async (waits for the engine's stream first; immediate after
 * pp_sync).  dets [batch*nms_post_max_size], n_dets [batch].  PP_ERR_STATE when there are none.
 * PP_ERR_NUMERIC when a frame's head maps hold a non-finite value (pp_last_error names the frame): with
 * PP_PREC_SPLIT_F16 that is an activation beyond the float16 pieces' range -- the frames are still resident, so
 * pp_set_gemm_precision(h, PP_PREC_F32) + pp_detect_async + pp_get_detections re-runs them in float32; in PP_PREC_F32
 * the network itself overflowed (the reference, model/voxelnet.py:1060-1390, would return NaN boxes).  Nothing is
 * written to dets / n_dets in that case. */
int pp_get_detections(pp_handle h, pp_detection* dets, int32_t* n_dets);
/* Selects the backbone's GEMM arithmetic (enum pp_gemm_precision) for this handle; re-derives the device weights
 * (pp_finalize_weights' work) when they are loaded.  Waits for the handle's stream.  The default comes from the
 * environment (PP_GEMM_PREC=f32) or is PP_PREC_SPLIT_F16. */
int pp_set_gemm_precision(pp_handle h, int32_t precision);
int pp_get_gemm_precision(pp_handle h, int32_t* precision);
/* Selects the suppression rule (enum pp_nms_mode) of this handle's post-process: pp_predict and the fused path.  Takes
 * effect from the next pp_detect* / pp_predict; everything else of the post-process (candidates, top-100, decode, caps,
 * flip, camera transform, PP_ERR_NUMERIC) is the same in both modes, and with the default every output is what it was
 * before the mode existed.  PP_ERR_ARG for an unknown mode, PP_ERR_STATE while a training step is in flight (the rule
 * then stays as it was).  The rule is part of what a captured pass is keyed on: a change captures once more. */
int pp_set_nms_mode(pp_handle h, int32_t mode);
int pp_get_nms_mode(pp_handle h, int32_t* mode);
/* Parameters of PP_NMS_SOFT (they are kept, but read by no other mode): method (enum pp_soft_nms_method), sigma of the
 * Gaussian weight, and score_floor, the score under which a re-scored box is dropped.  Defaults: PP_SOFT_NMS_GAUSSIAN,
 * 0.5, 0.001 (soft_nms_jit's); Nt is nms_iou_threshold.  In that mode the first min(100, nms_pre_max_size) candidates go
 * through the rounds of pp_soft_nms (equal current scores: the earlier candidate, i.e. the lower anchor index, first), at
 * most nms_post_max_size selections are returned in selection order, and pp_detection.score is the decayed score;
 * everything else of the post-process is the same.  With PP_SOFT_NMS_HARD, a floor > 0 below every score and Nt =
 * nms_iou_threshold the mode returns the default mode's bytes.  Takes effect from the next pp_detect* / pp_predict.
 * PP_ERR_ARG for an unknown method, a sigma that is not finite or <= 0, a floor that is not finite or < 0 (the settings
 * then stay as they were); PP_ERR_STATE while a training step is in flight.  The three values are part of what a captured
 * pass is keyed on.  pp_set_nms_mode between PP_NMS_ROTATED and PP_NMS_SOFT is PP_ERR_UNSUPPORTED (soft re-scoring on the
 * rotated overlap is not built): go through PP_NMS_STANDUP. */
int pp_set_soft_nms(pp_handle h, int32_t method, float sigma, float score_floor);
int pp_get_soft_nms(pp_handle h, int32_t* method, float* sigma, float* score_floor);
/* Image boxes of the kept detections, computed at the end of this handle's post-process (pp_predict and the fused path):
 * box3d_to_bbox of second/core/box_np_ops.py:849-857 -- the eight corners of box3d_camera projected by the frame's P2,
 * min / max over them, float64 -- which the reference's predict() replaced by a constant (model/voxelnet.py:1336-1360).
 * p2 [batch,16]: the frames' 4 x 4 camera matrices, row-major; frame b of a pass uses matrix b, so a pass of more than
 * `batch` frames is refused (PP_ERR_STATE).  NULL switches the projection off (`batch` is then ignored); off is the
 * default, and then every output is what it was before the switch existed.  As the reference's project_to_image
 * appends zeros, not ones, as the homogeneous coordinate, only the left 3 x 3 of each matrix enters; nothing clips to the
 * image and nothing treats corners behind the camera (w' < 0 mirrors them, w' = 0 gives inf / NaN).  Takes effect from
 * the next pp_detect* / pp_predict; pp_detection and everything else of the post-process are the same either way.  The
 * matrices live in device memory written on the handle's stream (the call waits for it), so a replayed pass reads the
 * current ones; on / off is part of what a captured pass is keyed on.  An unchanged set is not uploaded again.
 * PP_ERR_ARG for a batch outside 1..max_batch, PP_ERR_STATE while a training step is in flight (the setting then stays
 * as it was). */
int pp_set_projection(pp_handle h, const double* p2, int32_t batch);
int pp_get_projection(pp_handle h, int32_t* on);
/* The image boxes of the last pass (pp_detect_async or pp_predict), bbox [batch*nms_post_max_size,4] float64 rows
 * (min u, min v, max u, max v), row b * nms_post_max_size + i beside detection i of frame b.  Waits for the handle's
 * stream first, and returns PP_ERR_NUMERIC where pp_get_detections would; PP_ERR_STATE when that pass ran with the
 * projection off or there are no results.  Rows at or beyond a frame's n_dets are not written. */
int pp_get_bboxes(pp_handle h, double* bbox);
/* Selects how this handle's post-process treats the classes (enum pp_class_nms): pp_predict and the fused path.  With
 * PP_CLASS_NMS_PER_CLASS every class c = 0 .. num_class-1 goes through the whole pass by itself: candidates are the masked
 * anchors whose class-c score passes nms_score_threshold, the top 100 of them by class-c score are decoded and suppressed
 * (the rule of pp_set_nms_mode) over the first nms_pre_max_size, at most nms_post_max_size are kept, and each kept box
 * gets label c.  A frame's detections are class 0's kept boxes in descending score, then class 1's, and so on; n_dets is
 * their total, at most num_class * nms_post_max_size, and the same anchor may appear under several classes.  The result
 * rows per frame follow the mode: see pp_get_detection_rows -- every buffer handed to pp_get_detections, pp_detect,
 * pp_predict and pp_get_bboxes has that many rows per frame.  PP_ERR_NUMERIC is raised as in the joint mode.  Takes effect
 * from the next pp_predict / pp_detect_async; results of a pass that ran in the other mode can no longer be fetched
 * (PP_ERR_STATE) until a new pass has run.  With the default every output is what it was before the mode existed.
 * PP_ERR_ARG for an unknown mode, PP_ERR_STATE while a training step is in flight (the mode then stays as it was).  The
 * mode is part of what a captured pass is keyed on: a change captures once more. */
int pp_set_class_nms(pp_handle h, int32_t mode);
int pp_get_class_nms(pp_handle h, int32_t* mode);
/* Rows per frame that pp_get_detections, pp_detect, pp_predict and pp_get_bboxes write in the handle's current mode:
 * nms_post_max_size with PP_CLASS_NMS_JOINT, num_class * nms_post_max_size with PP_CLASS_NMS_PER_CLASS. */
int pp_get_detection_rows(pp_handle h, int32_t* rows);
/* Last-level-cache budget of a pass, in MiB (default 256, 0 = off).  Layers whose input + output maps exceed it are run
 * over sub-ranges of the batch's frames, a block's consecutive separable layers sub-range by sub-range, so that a layer
 * reads what the layer before has just written while it still sits in the 256 MB cache (KITTI-shaped B = 32: -5 % per
 * pass; the shipped 80 x 64 grid fits as it is).  Results do not change.  Right for ONE handle in flight per GPU; a
 * caller that keeps several handles in flight (bench.py's feeder) sets 0: their working sets evict each other.
 * No reference counterpart (TensorFlow's executor owns that schedule).  Waits for the handle's stream. */
int pp_set_cache_budget(pp_handle h, int32_t megabytes);
/* Convenience: upload + calib + detect + sync + get (the evaluate loop body,
 * train.py:689-786 minus annotation formatting). */
int pp_detect(pp_handle h, const float* points, const int32_t* frame_offsets, int32_t batch,
              const float* rect, const float* trv2c, pp_detection* dets, int32_t* n_dets);

/* Debug / parity taps of the fused path (after pp_sync), any pointer may be
 * NULL: per-frame pillar counts [batch]; coors [batch*max_voxels,3];
 * num_points [batch*max_voxels]; anchors mask [batch,A]; head maps as in
 * pp_forward_voxels; canvas [batch,ny,nx,C]. */
int pp_fetch_intermediates(pp_handle h, int32_t* n_pillars, int32_t* coors, int32_t* num_points,
                           uint8_t* anchors_mask, float* box_preds, float* cls_preds,
                           float* dir_cls_preds, float* canvas);

/* ---- measurement ------------------------------------------------------ */

/* level 0: no events.  level 1: HIP events on the engine's stream around
 * every kernel launch of pp_detect_async (for bench.py's roofline leg). */
int pp_set_profiling(pp_handle h, int32_t level);
/* After pp_sync with profiling on: number of timed kernel launches of the last
 * pp_detect_async, their names and durations (ms).  Buffers sized by the
 * caller for `capacity` entries; names are static strings. */
int pp_get_kernel_times(pp_handle h, int32_t capacity, const char** names, float* ms, int32_t* count);
/* HIP-event stopwatch on the engine's stream. */
int pp_timer_start(pp_handle h);
int pp_timer_stop(pp_handle h, float* elapsed_ms); /* records, waits, returns the elapsed time */

/* Kernel-tuning aid: runs RPN layer `layer` (0-based, in launch order; the last one is
 * the heads) `reps` times on whatever the activation buffers hold for `batch` frames and
 * returns the average launch duration.  `ablate` must be 0 (PP_ERR_ARG otherwise); the
 * kernel is the one the pass would launch, chosen by the same environment switches. */
int pp_bench_layer(pp_handle h, int32_t layer, int32_t batch, int32_t reps, int32_t ablate, float* avg_ms);
/* Number of RPN layer launches per forward pass and the tag ("<kernel>:<layer>") of one. */
int pp_layer_count(pp_handle h, int32_t* count);
const char* pp_layer_tag(pp_handle h, int32_t layer);
/* The planner alone, for tests and tuning: which template instantiation the backbone would launch for one layer at
 * `batch` frames on a part with `compute_units` compute units (256 on the MI355X), written to `name` as a
 * NUL-terminated string.  It is the name of pp_layer_tag before the colon, except that k_sep_u and k_sep_p carry their
 * shared-window argument ("k_sep_u<64,1,3,1,0,0,1>", "k_sep_p<256,1>" / "k_sep_p<256>"), which the tags leave out.
 * Needs no handle and no device.  The process-start switches (PP_SEP_K4, PP_DECONV_K4, PP_SEP_KERNEL, PP_SEP_NT,
 * PP_GEMM_PREC) apply as they do to a pass: read once per process.  PP_ERR_ARG: NULL, batch or compute_units < 1, an
 * unknown kind, a name buffer that is too small (64 bytes hold every name). */
typedef struct pp_layer_plan_desc {
    int32_t kind;             /* 0 separable layer, 1 transposed convolution, 2 the heads as a layer of their own */
    int32_t cin, cout;        /* channels in / out (cout of one tap of a transposed convolution) */
    int32_t n_total;          /* cout (separable), k * k * cout (transposed convolution), 32 (heads) */
    int32_t stride;           /* separable layers: 1 or 2 */
    int32_t k;                /* transposed convolutions: kernel == stride */
    int32_t in_h, in_w;       /* input map */
    int32_t out_h, out_w;     /* output map (separable: strided; transposed convolution: in * k; heads: in) */
    int32_t head_mode;        /* transposed convolutions: 0 heads not fused, 1 the first fused branch, 2 a later one */
    int32_t has_wt16;         /* the layer's weights fit the float16 pieces (and the precision is PP_PREC_SPLIT_F16) */
    int32_t has_head_wt16;    /* so does its slice of the head weights */
    int32_t sparse_input;     /* the first layer of a sparse canvas */
} pp_layer_plan_desc;
int pp_plan_layer_name(const pp_layer_plan_desc* layer, int32_t batch, int32_t compute_units, char* name, int32_t name_capacity);

/* ---- AP-evaluator overlaps ------------------ */

/* Replaces rotate_iou_gpu_eval (second/core/non_max_suppression/nms_gpu.py:618-653; kernel
 * :579-615, device functions :180-415, :564-576).  boxes [n,5], query_boxes [k,5] float32 rows
 * (centre x, centre y, x size, y size, angle -- clockwise positive); out [n,k] float32 row-major:
 * rotated-rectangle intersection of (query k, box n) divided by: -1 the union, 0 the query's area,
 * 1 the box's area, 2 nothing (raw area).  Stateless; host pointers; `device` is the HIP device. */
int pp_rotate_iou_eval(int device, const float* boxes, int64_t n, const float* query_boxes, int64_t k,
                       int32_t criterion, float* out);
/* Replaces d3_box_overlap (second/utils/eval.py:159-163 with its kernel :132-156): camera-frame
 * boxes [n,7] / [k,7] float64 rows (x, y, z, l, h, w, ry); out [n,k] float64: BEV intersection
 * (float32, as above with criterion 2) x height overlap / {union | box volume | query volume | 1}. */
int pp_d3_box_overlap(int device, const double* boxes, int64_t n, const double* query_boxes, int64_t k,
                      int32_t criterion, double* out);

/* ---- rotated-box NMS ------------------------- */

#define PP_RNMS_MAX_BOXES 16384 /* most boxes that enter the suppression (after pre_max_size): the 64 x 64-bit mask takes
                                 * n * ceil(n / 64) * 8 bytes of device memory, 32 MB here */

/* Replaces rotate_nms_gpu (second/core/non_max_suppression/nms_gpu.py:455-490; kernel :419-452, device functions
 * :180-415, host sweep :111-128) with the caps of nms() around it (libraries/eval_helper_functions.py:463-492).
 * dets [n,6] float32 rows (centre x, centre y, x size, y size, angle, score).  pre_max_size <= 0: every box goes in,
 * otherwise the min(n, pre_max_size) best by score; boxes are walked by descending score (equal scores: lower index
 * first), a box is dropped when devRotateIoU(an earlier kept box, it) > iou_threshold (float32, strict: a NaN IoU --
 * two zero-area boxes -- suppresses nothing); at most post_max_size are kept (<= 0: no cap).  keep: room for
 * min(n, pre_max_size) (n without a cap) int32 indices into dets, written in walk order; *n_keep their number.  n = 0 is
 * PP_OK with *n_keep = 0.  PP_ERR_ARG for a non-finite score (checked on the host, nothing launched) or more than
 * PP_RNMS_MAX_BOXES boxes entering.  Stateless; host pointers; `device` is the HIP device.  The same input gives the same
 * bytes on every run. */
int pp_rotate_nms(int device, const float* dets, int64_t n, float iou_threshold, int32_t pre_max_size,
                  int32_t post_max_size, int32_t* keep, int64_t* n_keep);

/* ---- Soft-NMS -------------------------------- */

#define PP_SNMS_MAX_BOXES 4096 /* most boxes that enter the rounds (after pre_max_size): they stay in one workgroup's LDS */

/* Replaces soft_nms_jit (second/core/non_max_suppression/nms_cpu.py:79-169) with the caps of nms() around it
 * (libraries/eval_helper_functions.py:463-492).  dets [n,5] float32 rows (x1, y1, x2, y2, score).  pre_max_size <= 0: every
 * box goes in, otherwise the min(n, pre_max_size) best by score (equal scores: lower index first).  Each round selects the
 * alive box with the largest current score (equal scores: lower index first) -- that score is final -- and multiplies the
 * score of every other alive box whose `+1` overlap with it has positive width and height by the method's weight (enum
 * pp_soft_nms_method; float64 as numba types it, rounded to float32 once); a box re-scored to below score_floor is
 * dropped, a box that never overlaps a selected one is never dropped.  At most post_max_size rounds (<= 0: no cap).  keep
 * and scores: room for min(n, pre_max_size, post_max_size) entries (caps <= 0 not counted) -- int32 indices into dets in
 * selection order and the final scores, which are non-increasing; *n_keep their number.  n = 0 is PP_OK with *n_keep = 0.
 * PP_ERR_ARG for a non-finite score (checked on the host, nothing launched), an unknown method, a sigma that is not finite
 * or <= 0, a floor that is not finite or < 0, or more than PP_SNMS_MAX_BOXES boxes entering.  Stateless; host pointers;
 * `device` is the HIP device.  The same input gives the same bytes on every run. */
int pp_soft_nms(int device, const float* dets, int64_t n, int32_t method, float sigma, float iou_threshold,
                float score_floor, int32_t pre_max_size, int32_t post_max_size, int32_t* keep, float* scores,
                int64_t* n_keep);

/* ---- image boxes of camera-frame boxes ------- */

/* box3d_to_bbox (second/core/box_np_ops.py:849-857) of any boxes, without a handle: labels, database boxes.
 * boxes_camera [n,7] float64 rows (x, y, z, l, h, w, ry) of `frames` frames laid end to end, box_counts [frames] boxes
 * per frame (n is their sum), p2 [frames,16] the frames' matrices; bbox [n,4].  The arithmetic is the function the
 * detector's post-process calls (pp_set_projection): the same seven doubles give the same bits.  n = 0 or frames = 0 is
 * PP_OK with nothing written.  PP_ERR_ARG for a negative count.  Stateless; host pointers; `device` is the HIP device. */
int pp_box3d_to_bbox(int device, const double* boxes_camera, const int32_t* box_counts, int32_t frames, const double* p2,
                     double* bbox);

/* ---- AP-evaluator statistics ----------------- */

#define PP_EVAL_NTHRESH 41     /* recall sample points: thresholds per overlap tier */
#define PP_EVAL_MAX_BOXES 1024 /* most ground truths, and most detections, one frame may hold */

/* Replace the per-frame loops over compute_statistics_jit (second/utils/eval.py:166-287) of eval_class_v3
 * (:552-660, fused_compute_statistics :298-345) for all `ntiers` overlap tiers of one (class, difficulty).
 * Stateless; host pointers; `device` is the HIP device.  Frame f holds ground truths gt_off[f] .. gt_off[f+1],
 * detections dt_off[f] .. dt_off[f+1] and its overlaps at ov_off[f], packed [G][D] (ground truth major), float64;
 * every offset array has nframes + 1 entries and starts at 0.  ignored_gt / ignored_det: 0 counts, 1 neutral,
 * -1 another class (clean_data).  A frame with more than PP_EVAL_MAX_BOXES ground truths or detections is
 * PP_ERR_ARG.  No frames, or no boxes at all, is PP_OK with zeroed output.  kernel_ms (may be NULL) receives the
 * device time of the call's kernels.
 *
 * pp_eval_match: the pass with compute_fp = False.  matched [ntiers, gt_off[nframes]] int32: per tier and ground
 * truth the frame-local index of the detection counted as a true positive, or -1.
 * pp_eval_pr: the pass with compute_fp = True at thresholds [ntiers, PP_EVAL_NTHRESH] (nthresh[k] in use), summed
 * over the frames in a fixed order: pr [ntiers, PP_EVAL_NTHRESH, 4] float64 = tp, fp, fn, similarity sum; slots
 * past nthresh[k] are zero.  metric 0 takes the DontCare boxes (dc_off, dc_boxes [.,4]) off the false positives;
 * compute_aos adds (1 + cos(gt_alpha - dt_alpha)) / 2 per true positive. */
int pp_eval_match(int device, int32_t nframes, const int32_t* gt_off, const int32_t* dt_off, const int64_t* ov_off,
                  const double* overlaps, const double* scores, const int32_t* ignored_gt, const int32_t* ignored_det,
                  const double* min_overlaps, int32_t ntiers, int32_t* matched, float* kernel_ms);
int pp_eval_pr(int device, int32_t nframes, const int32_t* gt_off, const int32_t* dt_off, const int64_t* ov_off,
               const double* overlaps, const double* scores, const int32_t* ignored_gt, const int32_t* ignored_det,
               const double* min_overlaps, int32_t ntiers, const double* gt_alphas, const double* dt_alphas,
               const double* dt_boxes, const int32_t* dc_off, const double* dc_boxes, int32_t metric,
               int32_t compute_aos, const double* thresholds, const int32_t* nthresh, double* pr, float* kernel_ms);

/* ---- training loss at the head maps ---------- */

/* Mirrors model.second.loss / pos_class_weight / ... of configs/train.yaml:147-167. */
typedef struct pp_loss_config {
    float alpha;             /* weighted_sigmoid_focal.alpha (0.25); negative = no alpha weighting */
    float gamma;             /* weighted_sigmoid_focal.gamma (2.0) */
    float sigma;             /* weighted_smooth_l1.sigma (3.0) */
    float code_weight[7];    /* weighted_smooth_l1.code_weight */
    float pos_class_weight, neg_class_weight;
    float classification_weight, localization_weight, direction_loss_weight;
    int32_t norm_by_num_positives;     /* loss_norm_type == "NormByNumPositives" */
    int32_t encode_rad_error_by_sin;   /* model.second.encode_rad_error_by_sin */
    int32_t use_direction_classifier;
} pp_loss_config;

/* Replaces the loss half of VoxelNet.call in training mode (model/voxelnet.py:922-1049: prepare_loss_weights
 * :461-512, create_loss :74-155, sigmoid_focal_classification_loss :262-364, WeightedSmoothL1LocalizationLoss
 * :407-459, get_direction_target :38-46, weighted_softmax_classification_loss :180-235) on the head maps the
 * last forward pass of this handle left on the device (pp_detect / pp_detect_async + pp_sync /
 * pp_forward_voxels with the same `batch`).  labels [batch][A] int32 (>0 class, 0 background, -1 ignored),
 * reg_targets [batch][A][7] float32: the dataloader's `labels` / `reg_targets` (load_data.py:3096-3100).
 * losses[8] = {loss, loc_loss_reduced, cls_loss_reduced, dir_loss_reduced, cls_pos_loss, cls_neg_loss,
 * number of positive anchors, 0}.  head_grad (may be NULL): d loss / d head map, [batch][H'*W'][32] float32 in
 * the fused head-map layout [box napl*7 | cls napl | dir napl*2 | zero pad] -- what the backward pass of the
 * head GEMM consumes.  Host pointers; synchronous. */
int pp_head_loss(pp_handle h, const int32_t* labels, const float* reg_targets, int32_t batch,
                 const pp_loss_config* cfg, float* losses, float* head_grad);

/* Replaces optimizer.apply_gradients for one flat float32 parameter buffer (train.py:228-239, :301:
 * tfa.optimizers.AdamW over tf.keras Adam): var -= weight_decay * var; m, v moments; var -= lr_t * m /
 * (sqrt(v) + epsilon) with lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) computed by the caller (t = step + 1,
 * lr from the ExponentialDecay schedule).  DEVICE pointers (params, grads, m, v: n floats each, on `device`);
 * `stream` is a hipStream_t or NULL; asynchronous on that stream.  Stateless. */
int pp_adamw_step_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                         int64_t n, float lr_t, float beta1, float beta2, float epsilon, float weight_decay);

/* The same update over part of the buffers only (fine-tuning with frozen layers): `segments` is a HOST array of
 * n_segments (offset, size) pairs in floats; entries outside them -- params, m and v alike -- are neither read nor
 * written.  An updated entry is bit-identical to what pp_adamw_step_device computes for it. */
int pp_adamw_step_segments_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                                  const int64_t* segments, int32_t n_segments, float lr_t, float beta1, float beta2,
                                  float epsilon, float weight_decay);

/* Gradient clipping and the non-finite step guard in front of that update (the lines the reference's trainStep carries
 * commented out above optimizer.apply_gradients, train.py:293-294, plus TensorFlow's global-norm rule).  The rules, per
 * element g of the trainable segments, in float32 with one rounding per written operation; c = cfg->clip:
 *   PP_CLIP_NONE         g' = g          (monitor: the norms are taken, and the guard if it is on)
 *   PP_CLIP_VALUE        g' = min(max(g, -c), c); a NaN stays a NaN                        (tf.clip_by_value)
 *   PP_CLIP_NORM         g' = (g * c) / max(norm of g's group, c), TensorFlow's order      (tf.clip_by_norm, per group)
 *   PP_CLIP_GLOBAL_NORM  g' = g * scale, scale = c * min(1 / global norm, 1 / c); NaN when the norm is not finite
 *                                                                                          (tf.clip_by_global_norm)
 * g' exists in the update kernel's registers only: `grads` is never written.  A group is a set of segments (`groups`: a
 * HOST int32 per segment, values in [0, n_groups); NULL = one group, n_groups must then be 1); its norm is
 * (float)sqrt(sum of (double)g * (double)g), summed in an order fixed by the segment table alone (no floating-point
 * atomics: the same buffer gives the same bits on every run); the global sum adds the group sums in group order.
 * nonfinite = !isfinite(global sum): exactly when a trainable entry is NaN or Inf.  With skip_nonfinite != 0 and the flag
 * set the update leaves params, m and v untouched (decided on the device; the caller learns it from `skipped`).  It does
 * the same when the flag is clear but the float32 global norm is Inf (finite gradients with a norm beyond FLT_MAX:
 * PP_CLIP_GLOBAL_NORM would scale by NaN): skipped = skip_nonfinite && (nonfinite || !isfinite(global norm)).
 *
 * The statistics block, the first (4 + 2 * n_groups) 32-bit words of the workspace, written on the device:
 *   [0] float global norm   [1] float global scale (1 unless PP_CLIP_GLOBAL_NORM)   [2] int32 nonfinite   [3] int32 skipped
 *   [4 .. 4 + n_groups) float norm per group
 *   [4 + n_groups .. 4 + 2 n_groups) float scale per group: PP_CLIP_NORM c / max(norm, c) (what the rule above amounts
 *   to, up to its two roundings), PP_CLIP_GLOBAL_NORM the global scale, else 1
 * Launches: PP_CLIP_VALUE and PP_CLIP_NONE without the guard launch the update only (pp_adamw_step_clipped_device; no
 * workspace needed); every other combination runs the reduction first: one launch per 128 non-empty segments plus one
 * that finishes the statistics, then the update (one launch per 64 non-empty segments, as pp_adamw_step_segments_device). */
enum pp_grad_clip_mode { PP_CLIP_NONE = 0, PP_CLIP_VALUE = 1, PP_CLIP_NORM = 2, PP_CLIP_GLOBAL_NORM = 3 };

typedef struct pp_grad_clip_config {
    int32_t mode;            /* enum pp_grad_clip_mode */
    float clip;              /* c: > 0 and finite for a clipping mode; ignored for PP_CLIP_NONE */
    int32_t skip_nonfinite;  /* != 0: a step whose trainable gradient holds a NaN or Inf changes nothing */
} pp_grad_clip_config;

/* *bytes: the size of the device workspace (statistics block included) for buffers of n_floats floats, n_segments
 * segments and n_groups groups; the caller allocates it once, 8-byte aligned, and need not clear it.  PP_ERR_ARG for a
 * negative argument, n_groups < 1 or a NULL `bytes`. */
int pp_grad_clip_workspace_bytes(int64_t n_floats, int32_t n_segments, int32_t n_groups, int64_t* bytes);

/* The reduction alone (monitoring, tests): fills the statistics block with the norms, scales of 1, the nonfinite flag
 * and skipped = 0.  DEVICE pointers grads (n floats) and workspace (sized by pp_grad_clip_workspace_bytes(n, n_segments,
 * n_groups)); `segments` as in pp_adamw_step_segments_device; asynchronous on `stream`; stateless.  PP_ERR_ARG for a
 * segment outside [0, n), overlapping segments (more partial sums than the workspace holds), a group outside
 * [0, n_groups), or a null / misaligned workspace. */
int pp_grad_norm_device(int device, void* stream, const float* grads, int64_t n, const int64_t* segments,
                        int32_t n_segments, const int32_t* groups, int32_t n_groups, void* workspace);

/* pp_adamw_step_segments_device on the clipped gradient: the reduction if the mode or the guard needs it, then the
 * update; from g' on an updated entry is bit-identical to what pp_adamw_step_segments_device makes of a buffer that
 * holds g'.  Buffers of n floats.  PP_ERR_ARG as above, for an unknown mode, and for a clipping mode whose clip is <= 0 or
 * not finite; `workspace` may be NULL where no reduction runs. */
int pp_adamw_step_clipped_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                                 int64_t n, const int64_t* segments, int32_t n_segments, const int32_t* groups,
                                 int32_t n_groups, const pp_grad_clip_config* cfg, void* workspace, float lr_t,
                                 float beta1, float beta2, float epsilon, float weight_decay);

/* ---- training step ---------------------------- */

/* The trainable tensors live in ONE flat float32 device buffer owned by the caller (a second one of the same
 * order receives the gradients, a third, smaller one holds the BatchNorm moving statistics): what the AdamW kernel
 * above and the data-parallel all-reduce work on.  These two calls describe the order: entry i is the Keras tensor
 * `name` (layouts of <package>/weights.py: depthwise [3,3,Cin,1], pointwise [1,1,Cin,Cout], Conv2DTranspose
 * [k,k,Cout,Cin], Dense [Fa,C], heads [1,1,Cin,Cout] + bias), `size` floats at `offset` of the parameter buffer
 * (is_state 0) or of the state buffer (is_state 1: moving_mean / moving_variance).  `name` stays valid for the
 * life of the handle. */
int pp_train_layout(pp_handle h, int32_t* n_entries, int64_t* n_param_floats, int64_t* n_state_floats);
int pp_train_layout_entry(pp_handle h, int32_t i, const char** name, int64_t* offset, int64_t* size, int32_t* is_state);

/* Replaces one trainStep of train.py:265-304 up to (not including) optimizer.apply_gradients: VoxelNet.call in
 * training mode (model/voxelnet.py:850-1049: PillarFeatureNet, scatter, RPN with batch-statistics BatchNorm, the
 * losses) on the `batch` frames resident in the handle (pp_upload_points*; they are voxelised here), and the
 * gradient of `loss` with respect to every trainable tensor.  params_dev / grads_dev / state_dev: DEVICE pointers to
 * the flat buffers described by pp_train_layout (grads overwritten; the moving statistics in state_dev updated in
 * place as Keras does).  labels [batch][A] int32, reg_targets [batch][A][7] float32: HOST pointers, the dataloader's
 * targets (load_data.py:3096-3100).  losses[8] as pp_head_loss.  Runs on the handle's stream and returns when the
 * step has finished (the caller then all-reduces grads_dev and calls pp_adamw_step_device). */
int pp_train_step(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const int32_t* labels,
                  const float* reg_targets, int32_t batch, const pp_loss_config* cfg, float* losses);

/* The same step in two halves, for the loader's hand-over (the reference's tf.data pipeline prepares batch n + 1 while
 * trainStep n runs, train.py:228-304): _async enqueues the step on the handle's stream and returns; between the two
 * calls the caller may upload the NEXT batch (pp_upload_points_async: it goes into the handle's other input buffer on
 * the copy stream, beside the running kernels); _wait returns when the step has finished, with its losses.  labels /
 * reg_targets must stay unchanged until _wait returns.  pp_train_step = _async + _wait. */
int pp_train_step_async(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const int32_t* labels,
                        const float* reg_targets, int32_t batch, const pp_loss_config* cfg);
int pp_train_step_wait(pp_handle h, float* losses);

/* ---- training targets from ground-truth boxes (SURVEY section 8f, row f3 -- data half) -------------- */

/* Replaces the loader's target_assigner.assign -> create_target_np (load_data.py:3086-3101, :267-293, :331-532) with
 * anchors pruned by the frame's anchors_mask, no positive-fraction sampling (target_assigner.sample_positive_fraction
 * draws from numpy's global generator: that configuration stays on the host), norm_by_num_examples=False, box code
 * size 7.  Bit-exact with the float32 numpy code (the log columns of the regression targets: within 1 ulp). */
#define PP_MAX_GT_PER_FRAME 256

/* Mirrors model.second.target_assigner.anchor_generators.anchor_generator_stride's thresholds (compared in float32). */
typedef struct pp_target_config {
    float matched_threshold;     /* anchor_generator_stride.matched_threshold (0.5) */
    float unmatched_threshold;   /* ...unmatched_threshold (0.35) */
    int32_t reserved[2];         /* 0 */
} pp_target_config;

/* Targets for `batch` frames.  gt_boxes: [sum(gt_counts), 7] x y z w l h r, the frames' boxes back to back; gt_classes:
 * [sum(gt_counts)] (1..num_class) or NULL (all 1); gt_counts [batch], each 0..PP_MAX_GT_PER_FRAME.  anchors_mask:
 * [batch, A] uint8, or NULL = the masks of the frames resident in the handle (voxelised on the GPU; `batch` must be the
 * number of frames uploaded, else PP_ERR_STATE).  Outputs, [batch, A] each: labels (>0 class, 0 background, -1
 * ignored or masked out), reg_targets [batch, A, 7] (0 where label <= 0); optional (NULL = not wanted): gt_index = the
 * box of the anchor's best overlap (first maximum; index within the frame; -1 for a masked-out anchor or a frame
 * without boxes) and overlap = that overlap (-1 for a masked-out anchor).  PP_ERR_ARG for a non-finite box, a size
 * w / l / h <= 0, a class outside 1..num_class, a negative count or one above PP_MAX_GT_PER_FRAME.  Host pointers;
 * synchronous.  The handle's fused-path results are left alone. */
int pp_assign_targets(pp_handle h, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                      int32_t batch, const uint8_t* anchors_mask, const pp_target_config* tc, int32_t* labels,
                      float* reg_targets, int32_t* gt_index, float* overlap);
/* pp_train_step_async / pp_train_step with the targets assigned on the GPU from the boxes (arguments as
 * pp_assign_targets; the anchor masks of the resident frames): the boxes go up on the copy stream behind the first half
 * of the step, the assignment runs between the halves.  gt_boxes / gt_classes / gt_counts must stay unchanged until
 * pp_train_step_wait returns, which serves both entry points. */
int pp_train_step_gt_async(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                           const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                           const pp_target_config* tc);
int pp_train_step_gt(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                     const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                     const pp_target_config* tc, float* losses);

/* ---- training-time augmentation -------------------------------------------------------- */
/* prep_pointcloud's training branch after GT-database sampling (load_data.py:2751-2866): noise_per_object_v3_ (num_try
 * tries per box, the first collision-free one wins), dropping the invalid boxes, random_flip, global_rotation,
 * global_scaling_v2, global_translate, limit_period(yaw, 0.5, 2 pi), the point shuffle and
 * filter_gt_box_outside_range_by_center.  The random numbers come from the caller (<package>/augment.py draw: the
 * reference's numpy calls in its order); every decision is taken in float64, points are rounded to float32 once. */
#define PP_AUG_MAX_TRY 128

typedef struct pp_augment_config {
    int32_t num_try;                /* tries per box, 1..PP_AUG_MAX_TRY (the loader passes 100) */
    int32_t global_rot_per_object;  /* |global_random_rotation_range_per_object| >= 1e-3: noise_per_box_v2_'s rule */
} pp_augment_config;

/* One frame's global draws. */
typedef struct pp_aug_frame {
    double theta;   /* global_rotation's angle: points and centres turn by -theta, the yaw gains theta */
    double scale;   /* global_scaling_v2's factor (> 0) */
    double t[3];    /* global_translate's shift */
    int32_t flip;   /* random_flip: y = -y, yaw = -yaw */
    uint32_t seed;  /* key of the point shuffle (output point i = input point perm(seed, n)[i]) */
} pp_aug_frame;

/* Augments the RESIDENT frames in place (the next pp_train_step_gt* trains on them) and returns them with their boxes.
 * gt_boxes / gt_classes / gt_counts as pp_assign_targets; gt_valid [sum(gt_counts)] uint8 or NULL (all valid): invalid
 * boxes are obstacles for the others' tries and are dropped.  frames [batch]; box_draws [sum(gt_counts)][num_try][5]
 * float64 (loc x y z, rot, global rot) per box.  Outputs (host): points_out [sum n, F] (the resident offsets),
 * boxes_out [sum(gt_counts), 7] and classes_out [sum(gt_counts)] of which the first sum(counts_out) rows are written,
 * counts_out [batch] (boxes kept per frame).  PP_ERR_ARG for what pp_assign_targets refuses, a non-finite draw, a
 * scale <= 0, num_try outside 1..PP_AUG_MAX_TRY, or a batch other than the resident one; the handle stays usable.
 * Synchronous. */
int pp_augment(pp_handle h, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
               const int32_t* gt_counts, int32_t batch, const pp_augment_config* ac, const pp_aug_frame* frames,
               const double* box_draws, float* points_out, float* boxes_out, int32_t* classes_out, int32_t* counts_out);
/* pp_train_step_gt_async / pp_train_step_gt on the augmented frames: the augmentation runs on the handle's stream
 * before the forward half (plain launches, outside the step's graphs), and the targets are assigned from the augmented
 * boxes.  Exactly what pp_augment followed by pp_train_step_gt on its outputs computes.  The host arrays must stay
 * unchanged until pp_train_step_wait returns. */
int pp_train_step_aug_async(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev,
                            const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch,
                            const pp_loss_config* lc, const pp_target_config* tc, const uint8_t* gt_valid,
                            const pp_augment_config* ac, const pp_aug_frame* frames, const double* box_draws);
int pp_train_step_aug(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                      const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                      const pp_target_config* tc, const uint8_t* gt_valid, const pp_augment_config* ac,
                      const pp_aug_frame* frames, const double* box_draws, float* losses);

/* Parity tap of the last augmentation (pp_augment or pp_train_step_aug*, after it finished): the try each input box
 * took, -1 for none and for an invalid box, in the order of gt_boxes.  *count = the number of input boxes; at most
 * `capacity` values are written.  PP_ERR_STATE after a pp_train_step_sample* (its draw rows are allotted per frame; which
 * of them belong to boxes is known on the device only). */
int pp_augment_selected(pp_handle h, int32_t* selected, int64_t capacity, int64_t* count);

/* ---- GT-database sampling (SURVEY section 8f, row 15 -- the loader's first step) ------------------------------------ */
/* prep_pointcloud's sampling step (load_data.py:2702-2751: sample_all :1690-1921 on the BatchSamplers' candidates
 * :1344-1409): stored objects are pasted into the resident frames where they collide with no box (box_collision_test as
 * pp_augment executes it) and pass the point test against the frame's original points.  Which objects are candidates
 * and the `low` coin of every slot come from the caller (<package>/gt_sampler.py draw_candidates: the reference's
 * cursor and getrandbits calls); every decision is taken in float64 in the reference's operation order, a pasted point
 * is its stored float32 value plus the float64 box centre, rounded to float32 once.
 * Deviation: a frame without boxes is retried at most PP_GTS_MAX_ROUNDS times (the reference: without limit); a frame
 * whose rounds all fail comes back unchanged. */
#define PP_GTS_MAX_CAND 32   /* candidate slots per frame, all classes and rounds together */
#define PP_GTS_MAX_ROUNDS 4  /* rounds drawn per frame; a frame that has boxes uses the first only */

/* status of a candidate slot (pp_gt_sample_info) */
enum pp_gts_status {
    PP_GTS_ACCEPTED = 0,
    PP_GTS_BOX_COLLISION = 1,   /* hit a frame box, an accepted earlier object or a candidate of its group not yet walked */
    PP_GTS_TOO_MANY_POINTS = 2, /* frame points inside >= max_point_collision */
    PP_GTS_TOO_FEW_POINTS = 3,  /* fewer than min_point_collision and not (nearer than 2.5 m with its `low` coin set) */
    PP_GTS_EMPTY_OBJECT = 4,    /* the stored object has no points */
    PP_GTS_ROUND_NOT_USED = 5   /* a later round of a frame that has boxes, or behind the round that succeeded */
};

typedef struct pp_gt_sample_config {
    int32_t max_point_collision;  /* train_input_reader.sampler_max_point_collision (500) */
    int32_t min_point_collision;  /* ...sampler_min_point_collision (1) */
    int32_t reserved[2];          /* 0 */
} pp_gt_sample_config;

/* One candidate slot of a frame's round. */
typedef struct pp_gts_cand {
    int32_t object;   /* index into the loaded database */
    int32_t group;    /* position of its class in sample_classes: groups are walked in ascending order, a later group
                         avoids the objects accepted for the earlier ones; non-decreasing within a round */
    int32_t low;      /* the `low` coin of the k-th SURVIVOR of the box test of this round, k = this slot's position in
                         its round (the reference draws it per survivor, in order) */
    int32_t reserved; /* 0 */
} pp_gts_cand;

/* Uploads the object database (replaces the one loaded before; freed with the handle): points [point_offsets[n], F] float32
 * centred on their box, point_offsets [n + 1], boxes [n, 7] float64 x y z w l h r (after BatchSampler.random_translate),
 * classes [n] (1..num_class).  The points have the handle's num_point_features columns; the call cannot check that (a
 * buffer of another width is read with the wrong stride).  PP_ERR_ARG for non-monotone offsets, a non-finite box, a size <= 0 or a class outside
 * 1..num_class.  Waits for the handle's stream. */
int pp_gtdb_load(pp_handle h, const float* points, const int64_t* point_offsets, const double* boxes,
                 const int32_t* classes, int64_t n);

/* Samples into the RESIDENT frames, which the result replaces (pasted points first, then the frame's own), and returns
 * them with their boxes.  gt_boxes / gt_classes / gt_valid / gt_counts as pp_augment (invalid boxes are obstacles like
 * the others and keep their flag).  cands [batch][PP_GTS_MAX_CAND]: the frame's rounds back to back; cand_counts
 * [batch][PP_GTS_MAX_ROUNDS]: slots per round (sum <= PP_GTS_MAX_CAND).  Outputs (host): points_out with room for
 * sum(n_b) + the points of every candidate, offsets_out [batch + 1], boxes_out / classes_out / valid_out with room for
 * sum(gt_counts) + batch * PP_GTS_MAX_CAND rows, counts_out [batch].  PP_ERR_STATE without a database; PP_ERR_ARG for
 * what pp_augment refuses in the boxes, an object index outside the database, groups out of order, a frame whose points
 * plus those of one round's candidates exceed max_points_per_frame, or whose boxes plus one round's candidates exceed
 * PP_MAX_GT_PER_FRAME -- before anything is launched; the handle stays usable.  Synchronous. */
int pp_gt_sample(pp_handle h, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                 const int32_t* gt_counts, int32_t batch, const pp_gt_sample_config* sc, const pp_gts_cand* cands,
                 const int32_t* cand_counts, float* points_out, int64_t points_capacity, int32_t* offsets_out,
                 float* boxes_out, int32_t* classes_out, uint8_t* valid_out, int32_t* counts_out);

/* pp_train_step_gt_async / pp_train_step_gt on frames sampled -- and, with ac != NULL, augmented -- on the GPU first: plain
 * launches on the handle's stream ahead of the forward half; the targets are assigned from the final boxes.  Exactly what
 * pp_gt_sample, then pp_augment on its outputs, then pp_train_step_gt on theirs compute.  Nothing is read back in
 * between: everything behind the sampling is sized from its bound (pp_gt_sample's refusals apply), and the handle then
 * knows the resident frames' sizes on the device only -- pp_gt_sample and pp_augment return PP_ERR_STATE until the next
 * upload.  box_draws: frame b has gt_counts[b] + (the slots of its largest round) rows of [num_try][5], of which the first
 * gt_counts[b] + accepted are used, in the order of pp_gt_sample's boxes_out.  PP_ERR_UNSUPPORTED with
 * ac->global_rot_per_object (those draws depend on the box, which is chosen on the device).  The host arrays must stay
 * unchanged until pp_train_step_wait returns. */
int pp_train_step_sample_async(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev,
                               const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch,
                               const pp_loss_config* lc, const pp_target_config* tc, const uint8_t* gt_valid,
                               const pp_gt_sample_config* sc, const pp_gts_cand* cands, const int32_t* cand_counts,
                               const pp_augment_config* ac, const pp_aug_frame* frames, const double* box_draws);
int pp_train_step_sample(pp_handle h, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                         const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                         const pp_target_config* tc, const uint8_t* gt_valid, const pp_gt_sample_config* sc,
                         const pp_gts_cand* cands, const int32_t* cand_counts, const pp_augment_config* ac,
                         const pp_aug_frame* frames, const double* box_draws, float* losses);

/* Parity tap of the last pp_gt_sample: per candidate slot [batch][PP_GTS_MAX_CAND] its enum pp_gts_status (slots past a
 * round's count: PP_GTS_ROUND_NOT_USED) and the number of the frame's original points inside its box (0 for a slot that
 * did not survive the box test); round_used [batch]: the round whose objects were pasted, -1 for none. */
int pp_gt_sample_info(pp_handle h, int32_t* status, int32_t* point_counts, int32_t* round_used, int32_t batch);

/* ---- building the object database ------------------------------------------------------------------- */
/* create_groundtruth_database (create_data.py:365-551) on the RESIDENT frames, which are only read (a pp_detect_async
 * after it sees them unchanged): every point of frame b against each of its box_counts[b] labelled boxes -- boxes
 * [sum box_counts][7] float64 LIDAR boxes x y z w l h r, the frames' back to back (the camera -> lidar conversion is the
 * caller's: <package>/gt_database.py box_camera_to_lidar).  A point is inside a box iff ((x n0 + y n1) + z n2) + d < 0 for
 * all six faces, in float64 on the widened float32 coordinates, planes as points_in_rbbox builds them; a point inside
 * several boxes goes to each.  Host outputs: counts_out [sum box_counts] points per box; offsets_out [sum box_counts + 1]
 * first row of each object in points_out; points_out [offsets_out[last]][F]: an object's points in the frame's order,
 * x y z as (float)((double)p - centre) -- one rounding, what `float32 array -= float64 centre` gives --, the other columns
 * copied.  points_capacity (in points) too small: PP_ERR_ARG with only counts_out written, so the caller can size the buffer
 * from it and call again.  PP_ERR_ARG, before anything is launched, for a non-finite box, a size <= 0, a count outside
 * 0..PP_MAX_GT_PER_FRAME or a batch other than the resident one; PP_ERR_STATE when the resident frames' sizes are device
 * values (after a pp_train_step_sample* or an ingest) or a training step is in flight; the handle stays usable.  The
 * result is the same bytes on every run.  Synchronous. */
int pp_gtdb_build(pp_handle h, const double* boxes, const int32_t* box_counts, int32_t batch, int32_t* counts_out,
                  int64_t* offsets_out, float* points_out, int64_t points_capacity);
/* The same without the cut-out: counts_out only -- _calculate_num_points_in_gt (create_data.py:28-93). */
int pp_gtdb_count(pp_handle h, const double* boxes, const int32_t* box_counts, int32_t batch, int32_t* counts_out);

/* ---- live-camera ingest --------------------------------------------------------------- */
/* The reference's production mode in front of the network (load_data.py:2433-2443, train.py:810-828):
 * ros_numpy.point_cloud2.pointcloud2_to_xyz_array(msg) (x y z out of the message bytes, records with a non-finite
 * coordinate dropped), points[first::decimate], np.dot(np.dot(points, r), r2) + lift -- on the GPU, from the raw bytes of
 * `batch` sensor_msgs/PointCloud2 messages to the resident frames of the next pp_detect_async.  Per record (message order,
 * i = row * width + col at row * row_step + col * point_step): finite = x, y and z finite (+-inf is not); rank = finite
 * records in front of it; kept when finite, rank >= first and (rank - first) % decimate == 0, as row (rank - first) /
 * decimate of its frame; a kept point is ((p . r) . r2) + lift in float64 -- each 3-term dot product summed left to right,
 * products and sums rounded separately, which is bit for bit what numpy computes -- rounded to float32 once.  The result
 * equals <package>/ingest.py's realsense_to_lidar(pointcloud2_to_xyz(...), decimate, first, lift) exactly. */
typedef struct pp_pc2_layout {   /* one sensor_msgs/PointCloud2, without its bytes */
    int32_t width, height, point_step, row_step;
    int32_t x_offset, y_offset, z_offset;   /* PointField.offset of x, y, z; nothing needs to be aligned */
    int32_t datatype;            /* 7 FLOAT32 or 8 FLOAT64, the same for x y z.  Integer types (1..6) are refused with
                                    PP_ERR_UNSUPPORTED; a message whose three fields differ is passed as
                                    x | y << 8 | z << 16 and refused the same way */
    int32_t is_bigendian;
    int32_t reserved;            /* 0 */
} pp_pc2_layout;
typedef struct pp_ingest_config {
    int32_t first, decimate;     /* reference: 1, 4 */
    double r[9], r2[9], lift[3]; /* row-major; the caller's scipy matrices (their cos 90 deg entries are ~1e-16, not 0,
                                    and depend on the scipy build) and [0, 0, sensor height] */
} pp_ingest_config;

/* Ingests `batch` messages into the handle's other input buffer (as pp_upload_points does: the frames are then resident
 * for pp_detect_async) and waits.  data: the messages' bytes; message b occupies data[byte_offsets[b] ..
 * byte_offsets[b + 1]) and holds at least height * row_step bytes.  points_out (may be NULL): receives the resident
 * points [sum kept, 3], frames back to back -- the parity tap; points_out_capacity is in points, PP_ERR_ARG when it is
 * below the kept total (the frames stay resident).  The kept counts exist on the device only (pp_ingest_info reads them
 * back): everything behind the call is sized from the host-side bound max(0, ceil((width * height - first) / decimate))
 * per frame.  Refused before anything is queued, pp_last_error naming the frame and the field: PP_ERR_ARG when that bound
 * exceeds max_points_per_frame (a 640 x 480 cloud at 1, 4 needs max_points_per_frame >= 76800), row_step < width *
 * point_step, a field that does not fit point_step, a message shorter than height * row_step, decimate < 1, first < 0;
 * PP_ERR_STATE while a training step is in flight; PP_ERR_UNSUPPORTED for integer field datatypes, x / y / z of different
 * datatypes, and a handle whose num_point_features is not 3 (the reference's live path is xyz only).  Frames that keep no
 * point are legal. */
int pp_ingest_pointcloud2(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                          int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity);
/* Same without waiting: `data_pinned` is page-locked (pp_host_alloc) and stays unchanged until the pass that consumes the
 * frames has finished; byte_offsets / layouts / cfg are copied before the call returns.  The bytes travel on the handle's
 * copy stream, the ingest kernels and the voxeliser run behind them there, beside the pass in flight; the ordering rules
 * are pp_upload_points_async's, and the two may be mixed freely. */
int pp_ingest_pointcloud2_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                const pp_pc2_layout* layouts, int32_t batch, const pp_ingest_config* cfg);
/* Parity tap of the last ingest (waits for it): per frame the finite records and the points kept.  Either pointer may be
 * NULL.  PP_ERR_STATE when none has run, PP_ERR_ARG when `batch` is not that call's. */
int pp_ingest_info(pp_handle h, int32_t* finite_counts, int32_t* kept_counts, int32_t batch);

/* ---- depth-image ingest -------------------------------------------------------------------------------- */
/* The same resident frames from the depth camera's raw sensor_msgs/Image instead of the PointCloud2 message a point-cloud
 * node computes from it (a 640 x 480 16UC1 image is 0.6 MB, its message 6 to 10 MB).  Per pixel (v, u), in float32:
 *   16UC1 / mono16: z = depth_scale * (float)d (one product), valid when d != 0;
 *   32FC1: z is the stored value, valid when it is finite and > 0 (depth_scale is not applied: REP 118);
 *   both: valid only when z > z_min && z <= z_max (0 and +inf leave the conditions above as they are);
 *   a valid pixel is the point x = z * (((float)u - ppx) / fx), y = z * (((float)v - ppy) / fy), z -- every operation
 *   rounded separately, IEEE division: the pinhole (no distortion) case of the camera vendor's published
 *   rs2_deproject_pixel_to_point.  Parity with the bytes the camera driver's point-cloud block publishes is NOT pinned
 *   (neither the vendor library nor its ROS node is available to this project's tests); everything behind the point is:
 *   rank = valid pixels in front of it in row-major order, then the selection, the float64 transform and the single
 *   rounding of pp_ingest_pointcloud2, from the same pp_ingest_config.  The result equals <package>/ingest.py's
 *   depth_ingest_np, and realsense_to_lidar(pointcloud2_to_xyz(depth_to_pointcloud2(...)), decimate, first, lift), exactly.
 * Not done, and not approximated: lens distortion (the caller refuses a CameraInfo with a non-zero D; the d435i depth
 * stream's coefficients are zero), alignment of depth to the colour stream, dropping points by texture coordinate, RGB
 * or any feature beyond x y z, the vendor's spatial and temporal filters. */
#define PP_DEPTH_U16 0           /* 16UC1 / mono16 */
#define PP_DEPTH_F32 1           /* 32FC1 */
typedef struct pp_depth_layout { /* one sensor_msgs/Image with the intrinsics of its camera, without its bytes */
    int32_t width, height, row_step;        /* Image.step: any value >= width * itemsize, odd ones included */
    int32_t encoding;                       /* PP_DEPTH_U16 or PP_DEPTH_F32 */
    int32_t is_bigendian;
    float fx, fy, ppx, ppy;                 /* CameraInfo K[0], K[4], K[2], K[5] cast to float32 once */
    float depth_scale;                      /* metres per unit of a 16UC1 pixel (d435i: 0.001f); read for PP_DEPTH_U16 only */
    float z_min, z_max;                     /* 0, +inf: no clip */
} pp_depth_layout;

/* pp_ingest_pointcloud2 for depth images: image b occupies data[byte_offsets[b] .. byte_offsets[b + 1]) and holds at
 * least height * row_step bytes; points_out / points_out_capacity, the input-buffer flip, the staging and the host-side
 * bound max(0, ceil((width * height - first) / decimate)) per frame are that call's, and pp_ingest_info reads the counts
 * back (finite_counts = valid pixels).  Everything an ingest bars afterwards is barred the same way.  Refused before
 * anything is queued, pp_last_error naming the frame and the field: PP_ERR_ARG when the bound exceeds
 * max_points_per_frame, for row_step < width * itemsize, an unknown encoding, byte_offsets that give a frame fewer than
 * height * row_step bytes, fx or fy zero or not finite, ppx or ppy not finite, depth_scale <= 0 or not finite on
 * PP_DEPTH_U16, z_min > z_max (or a NaN), decimate < 1, first < 0, batch > max_batch; PP_ERR_STATE while a training step
 * is in flight; PP_ERR_UNSUPPORTED for a handle whose num_point_features is not 3. */
int pp_ingest_depth(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_depth_layout* layouts,
                    int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity);
/* Same without waiting, as pp_ingest_pointcloud2_async: page-locked bytes on the copy stream, the kernels and the
 * voxeliser behind them there; mixes freely with that call and with pp_upload_points_async. */
int pp_ingest_depth_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                          const pp_depth_layout* layouts, int32_t batch, const pp_ingest_config* cfg);

/* ---- camera-rig ingest ---------------------------------------------------------------------------------- */
/* Several sensors into one frame.  A call takes `sources` sources of ONE kind (depth images, or PointCloud2 messages) and
 * `batch` frames.  Source s occupies data[byte_offsets[s] .. byte_offsets[s + 1]), has its own layout layouts[s] and its own
 * cfgs[s] (first, decimate, r, r2, lift), and belongs to frame source_frame[s]; the map is non-decreasing, starts at 0, ends
 * at batch - 1, and gives every frame 1 to PP_RIG_MAX_SOURCES sources.  The resident points of frame b are the kept points
 * of its sources in source order, back to back, each source computed exactly as pp_ingest_depth / pp_ingest_pointcloud2
 * compute it alone under cfgs[s]: validity, finiteness, rank, selection, transform and rounding restart per source
 * (<package>/ingest.py: rig_depth_ingest_np, rig_ingest_np).  A general extrinsic [R | t] (p' = R p + t, p a column vector)
 * is r = R transposed, r2 = identity, lift = t.  One source per frame with equal cfgs leaves the bytes of the plain calls.
 * The reference has no such path (one camera, one frame); what is pinned is its single-camera chain, per source.
 * points_out / points_out_capacity, the staging, the input-buffer flip and what is barred afterwards are
 * pp_ingest_pointcloud2's; pp_ingest_info then reports the frames' sums, pp_ingest_rig_info the sources' own counts.
 * Refused before anything is queued, pp_last_error naming the source and the field: whatever the single-camera call
 * refuses about a frame, about the source; PP_ERR_ARG for a frame map that decreases, skips a frame, does not start at 0
 * or end at batch - 1, or gives a frame more than PP_RIG_MAX_SOURCES sources, for batch > max_batch, and for a frame whose
 * sources' summed bounds max(0, ceil((width * height - first) / decimate)) exceed max_points_per_frame; PP_ERR_STATE while a
 * training step is in flight; PP_ERR_UNSUPPORTED for a handle whose num_point_features is not 3.  Not done: time
 * synchronisation, de-duplication where cameras overlap, lens distortion, sources of both kinds in one call. */
#define PP_RIG_MAX_SOURCES 16    /* sources per frame */
int pp_ingest_rig_depth(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_depth_layout* layouts,
                        const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                        float* points_out, int64_t points_out_capacity);
/* Same without waiting, as pp_ingest_depth_async: page-locked bytes on the copy stream, the kernels and the voxeliser
 * behind them there; layouts / cfgs / source_frame are copied before the call returns. */
int pp_ingest_rig_depth_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                              const pp_depth_layout* layouts, const pp_ingest_config* cfgs, const int32_t* source_frame,
                              int32_t sources, int32_t batch);
int pp_ingest_rig_pointcloud2(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                              const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                              float* points_out, int64_t points_out_capacity);
int pp_ingest_rig_pointcloud2_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                    const pp_pc2_layout* layouts, const pp_ingest_config* cfgs, const int32_t* source_frame,
                                    int32_t sources, int32_t batch);
/* Parity tap of the last ingest when it was a rig call (waits for it): per source the finite records (valid pixels) and the
 * points kept.  Either pointer may be NULL.  PP_ERR_STATE when the last ingest was no rig call, PP_ERR_ARG when `sources`
 * is not that call's. */
int pp_ingest_rig_info(pp_handle h, int32_t* finite_counts, int32_t* kept_counts, int32_t sources);

/* ---- PointCloud2 feature fields -------------------------------------------------------------------------- */
/* A model with num_point_features F > 3 (x y z intensity: F = 4) fed from messages: row columns 3 ... F - 1 come out of the
 * message's own fields, one pp_pc2_feature per column and per message.  datatype 1 ... 8 (INT8 ... FLOAT64): the raw
 * element is read at record + offset in the message's byte order, nothing assumed aligned, widened exactly to float64, and
 * the column is float32(float64(raw) * scale + bias) -- product and sum rounded separately, no fused multiply-add, one
 * rounding to float32: numpy's (rec[name].astype(float64) * scale + bias).astype(float32).  datatype 0: a constant column,
 * nothing is read, the value is float32(bias).  Validity, rank and selection are pp_ingest_pointcloud2's, from x y z alone:
 * finite, kept, the offsets and columns 0 - 2 of every row are what that call gives; a non-finite FEATURE value is carried
 * through as it is (NaN as NaN, +-inf as +-inf).  Equals <package>/ingest.py's ingest_np(msg, ..., features=...) exactly.
 * Not done: feature-based validity, unpacking a packed rgb float into channels, depth images (an image has no field:
 * pp_ingest_depth* and pp_ingest_rig_depth* keep refusing F != 3). */
typedef struct pp_pc2_feature {
    int32_t offset;              /* byte offset of the element within a record (element index of a count > 1 field folded in) */
    int32_t datatype;            /* PointField code 1 ... 8, or 0: constant */
    double scale, bias;          /* finite */
} pp_pc2_feature;
/* pp_ingest_pointcloud2 / _async with `features` [batch][nfeat] behind cfg; nfeat must be num_point_features - 3, and with
 * nfeat 0 (features may be NULL) on a 3-feature handle these ARE those calls.  points_out is [sum kept, 3 + nfeat].
 * pp_ingest_info serves them unchanged.  Refused before anything is queued with PP_ERR_ARG, pp_last_error naming the frame and
 * the feature index: features NULL with nfeat > 0, nfeat != num_point_features - 3, a datatype outside 0 ... 8, offset < 0 or
 * offset + size > point_step, a non-finite scale or bias -- and everything the twin call refuses. */
int pp_ingest_pointcloud2_fields(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                                 int32_t batch, const pp_ingest_config* cfg, const pp_pc2_feature* features, int32_t nfeat,
                                 float* points_out, int64_t points_out_capacity);
int pp_ingest_pointcloud2_fields_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                       const pp_pc2_layout* layouts, int32_t batch, const pp_ingest_config* cfg,
                                       const pp_pc2_feature* features, int32_t nfeat);
/* The same for pp_ingest_rig_pointcloud2 / _async: `features` is [sources][nfeat], the refusals name the source;
 * pp_ingest_rig_info serves them unchanged. */
int pp_ingest_rig_pointcloud2_fields(pp_handle h, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                                     const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                                     const pp_pc2_feature* features, int32_t nfeat, float* points_out,
                                     int64_t points_out_capacity);
int pp_ingest_rig_pointcloud2_fields_async(pp_handle h, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                           const pp_pc2_layout* layouts, const pp_ingest_config* cfgs,
                                           const int32_t* source_frame, int32_t sources, int32_t batch,
                                           const pp_pc2_feature* features, int32_t nfeat);

/* ---- frustum crop (box_np_ops.remove_outside_points) ----------------------------------------------------- */
/* Crops the RESIDENT frames to the camera image's frustum on the GPU: what _create_reduced_point_cloud,
 * _calculate_num_points_in_gt(remove_outside=True) and create_groundtruth_database do to a KITTI cloud first.  planes
 * [batch][6][4] float64: per frame the six faces (n0, n1, n2, d) exactly as surface_equ_3d_jit returns them for the
 * frustum's lidar corners -- the caller's (<package>/frustum.py frustum_planes: a LAPACK inverse and a QR stand behind
 * them); the normals are not unit length and are used as they are.  Per point, s_k = ((x n0 + y n1) + z n2) + d in
 * float64 on the widened float32 coordinates, summed left to right, products and sums rounded separately; the point is
 * removed iff s_k >= 0 for some face, so a point with a NaN coordinate is kept and +-inf follows IEEE arithmetic.  Kept
 * points keep the frame's order and all F columns, bit for bit.  flags: PP_CROP_BACK negates column 0 first (exact); the
 * test is made on the negated value and the negated value is stored (the reference's `_back` files).  The same frames
 * give the same bytes on every run.
 * The frames are read where they lie (a zero-copy feed in the caller's page-locked memory) and written back to back into
 * the handle's other input buffer, which becomes the resident one, as after an upload.  Refused before anything is
 * queued, the handle staying usable: PP_ERR_ARG for a non-finite plane value (pp_last_error names the frame), a batch
 * other than the resident one or unknown flag bits; PP_ERR_STATE with no frames resident, when the resident frames' sizes
 * are device values (after an ingest, a sampled training step or pp_frustum_crop_async: crops do not chain) or while a
 * training step is in flight. */
#define PP_CROP_BACK 1
/* Synchronous: waits, writes kept_out [batch] and takes the kept counts as the frames' sizes -- pp_gtdb_build,
 * pp_gtdb_count, pp_augment, pp_detect_async, the stage taps and the training steps then see the cropped frames like any
 * upload.  points_out (may be NULL): receives the resident points [sum kept][F], frames back to back -- the parity tap;
 * points_capacity is in points, PP_ERR_ARG when it is below the kept total (kept_out is written and the frames stay
 * resident and cropped). */
int pp_frustum_crop(pp_handle h, const double* planes, int32_t batch, int32_t flags, int32_t* kept_out, float* points_out,
                    int64_t points_capacity);
/* Same without waiting, on the handle's copy stream behind the frames' upload, the voxeliser behind it there; planes is
 * copied before the call returns; the ordering rules are pp_upload_points_async's.  The kept counts stay on the device
 * (pp_frustum_crop_info reads them back): the handle is left as after an ingest, everything behind the call sized from
 * the frames' sizes before the crop, and the calls an ingest bars are barred the same way until the next upload. */
int pp_frustum_crop_async(pp_handle h, const double* planes, int32_t batch, int32_t flags);
/* The kept counts of the last crop (waits for it).  PP_ERR_STATE when none has run, PP_ERR_ARG when `batch` is not that
 * call's. */
int pp_frustum_crop_info(pp_handle h, int32_t* kept_out, int32_t batch);

/* ---- multi-sweep accumulation (sweeps.py of the Python package states the rule) --------------------------- */
/* Carries the last few sweeps of every stream (frame b of a call is stream b) into the current sensor frame under the ego
 * poses, on the GPU, between the feed and the pass: the RESIDENT frames become the resident frames plus their history.
 * A pose is 12 float64, the rows of [R | t] (3 x 4), mapping the sensor frame to a fixed frame: p_fixed = R p + t.  Per
 * stream a ring of history + 1 slots lives on the device (rows, row count, pose, stamp per slot).  One call, per stream:
 *   1. the used sweeps: the stored ones, newest first, with 0 < stamp_c - stamp_s <= max_age (float64);
 *   2. per used sweep M = R_c^T R_s, every entry ((a0 b0 + a1 b1) + a2 b2), d = t_s - t_c, u = R_c^T d in the same order
 *      -- float64, + - * only, products and sums rounded separately, computed on the device;
 *   3. output: the current rows, bit-unchanged (column time_feature, when >= 0, set to 0.0f); then each used sweep's rows
 *      in stored order, x' = (float)(((M00 x + M01 y) + M02 z) + u0) on the widened float32 coordinates (y', z' alike),
 *      column time_feature = (float)(stamp_c - stamp_s), every other column copied bitwise;
 *   4. the output frame is cut at max_points_per_frame rows (`truncated` counts the rows dropped; the cut may fall inside
 *      a sweep); frames are packed back to back;
 *   5. the ORIGINAL current frame is stored as its rows 0, j, 2j ... (j = history_decimate), cut at `capacity`
 *      (`push_truncated`), with its pose and stamp, in the slot that holds the oldest sweep -- never one this call reads.
 * The reference has no such path: nothing here is parity with it.  The same calls give the same bytes on every run. */
#define PP_SWEEP_MAX 8 /* past sweeps per stream */

typedef struct pp_sweep_config {
    double max_age;           /* seconds, finite and > 0: stored sweeps older than this are not used */
    int32_t history;          /* 1 .. PP_SWEEP_MAX past sweeps kept per stream */
    int32_t capacity;         /* rows per stored sweep, 1 .. ; 0: max_points_per_frame */
    int32_t history_decimate; /* j >= 1 */
    int32_t time_feature;     /* -1, or the column 3 .. num_point_features - 1 overwritten with the time lag */
} pp_sweep_config;

/* cfg == NULL: the stage is off (the default); the ring and its history are kept.  Otherwise the configuration is
 * validated (PP_ERR_ARG naming the field) and the ring is allocated here: max_batch x (history + 1) x capacity rows;
 * PP_ERR_HIP naming the bytes when the device cannot hold it (the stage is then off).  A configuration with another
 * history or capacity re-makes the ring and forgets every stream's history; one that differs in the other fields keeps
 * it.  PP_ERR_UNSUPPORTED for rows wider than the frustum crop moves; PP_ERR_STATE while a training step is in flight. */
int pp_set_sweeps(pp_handle h, const pp_sweep_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the configuration in force, capacity filled in (zeros before the first). */
int pp_get_sweeps(pp_handle h, int32_t* on, pp_sweep_config* cfg_out);
/* One call on the resident frames: poses [batch][12], stamps [batch] (seconds).  The frames are read where they lie --
 * their sizes are read on the DEVICE, so the state after any pp_ingest_* or pp_frustum_crop_async is accepted -- and the
 * output is written into the handle's other input buffer, which becomes the resident one.  Refused before anything is
 * queued, the handle and the history untouched: PP_ERR_STATE when pp_set_sweeps has not turned the stage on, with no
 * frames resident or while a training step is in flight; PP_ERR_ARG for a batch other than the resident one, a
 * non-finite pose or stamp, a rotation whose R R^T differs from the identity by more than 1e-6 in an entry, or a stamp
 * that does not increase over the stream's previous one (pp_last_error names the stream).
 * Synchronous, on the handle's stream: waits, writes counts_out [batch] (the output frames' rows) and takes them as the
 * frames' sizes, as pp_frustum_crop does.  points_out (may be NULL): the output frames [sum counts][F], back to back;
 * points_capacity in points, PP_ERR_ARG when it is below the total (the call has happened all the same). */
int pp_sweeps_accumulate(pp_handle h, const double* poses, const double* stamps, int32_t batch, int32_t* counts_out,
                         float* points_out, int64_t points_capacity);
/* Same without waiting, on the copy stream behind an asynchronous upload, ingest or crop, the voxeliser behind it there;
 * poses and stamps are copied before the call returns.  The counts stay on the device (pp_sweeps_info): the handle is
 * left as after an ingest, everything behind the call sized from bounds. */
int pp_sweeps_accumulate_async(pp_handle h, const double* poses, const double* stamps, int32_t batch);
/* Of the last call (waits for it), [batch] each, any may be NULL: output rows, used sweeps, rows dropped at
 * max_points_per_frame, rows cut at `capacity` when the frame was stored.  PP_ERR_STATE when none has run, PP_ERR_ARG
 * when `batch` is not that call's. */
int pp_sweeps_info(pp_handle h, int32_t* counts, int32_t* used, int32_t* truncated, int32_t* push_truncated, int32_t batch);
/* stream 0 .. max_batch - 1, or -1 for all: forgets the stream's stored sweeps and its last stamp (waits for the work
 * queued).  PP_ERR_STATE while a training step is in flight. */
int pp_sweeps_reset(pp_handle h, int32_t stream);

/* The handle's HIP stream (hipStream_t as void*).  A caller that enqueues its own device work behind a pp_train_step_async
 * -- the gradient all-reduce and pp_adamw_step_device of the optimizer step (train.py:301) -- does it on this stream and
 * needs no host synchronisation in between: pp_train_step_wait then waits for that work too. */
int pp_stream(pp_handle h, void** stream);

/* Debug / parity tap of the last finished training step: the decisions taken at its non-differentiable points.
 * layer >= 0: the layer-th BatchNorm + ReLU of the RPN in forward order (separable layers and transposed convolutions
 * as the network lists them: block1/0 .., deconv1, block2/0 .., deconv2, ...): relu_mask receives one byte per element
 * of the layer's pre-BatchNorm output ([b][y][x][c]; a transposed convolution: [b][y][x][tap][c] over its INPUT
 * pixels), 1 where the backward pass lets the gradient through.  layer < 0: the PFN's max -- relu_mask receives
 * int32 values (4 bytes each) [batch][max_voxels][C]: the winning row of the pillar, -1 = a zero-padded row, -2 = the
 * maximum is not positive (no gradient); slots >= the frame's pillar count are undefined.  *count = elements of that
 * layer; relu_mask NULL: only the count.  A test compares the step's gradients with a float64 graph that takes the
 * SAME decisions (ReLU and max are not differentiable where a value is within round-off of the kink). */
int pp_train_fetch_decisions(pp_handle h, int32_t layer, uint8_t* relu_mask, int64_t capacity, int64_t* count);

/* How often pp_train_step captured a hipGraph and how often it replayed one (one graph per input buffer of the
 * handle): steady-state steps must replay -- a regression check, not part of the reference's surface. */
int pp_train_graph_stats(pp_handle h, int32_t* captures, int32_t* replays);

/* Fine-tuning with frozen layers (the reference's set_trainable(net, False), train.py:62-113): the next training steps
 * treat the `n` named units as Keras treats layers with trainable = False -- their BatchNorm normalises with the moving
 * statistics (inference mode, even in a training step) and leaves them unchanged, and their tensors get no gradient
 * (their entries of grads_dev are written as 0).  The gradient still flows through a frozen unit to trainable units in
 * front of it.  Units: "pfn" (Dense + BatchNorm), "rpn/block<b>/<j>" (one separable layer with its BatchNorm),
 * "rpn/deconv<b>", "rpn/conv_box", "rpn/conv_cls", "rpn/conv_dir_cls" (with a direction head).  n = 0 unfreezes
 * everything.  PP_ERR_ARG for an unknown or repeated name, or when every unit would be frozen (the freeze then stays
 * as it was).  The freeze is part of what a captured step graph is keyed on: a change re-captures it once. */
int pp_train_set_frozen(pp_handle h, const char* const* units, int32_t n);

/* ---- training metrics -------------------------------------------------------------------- */

#define PP_METRICS_COUNTS 32 /* int64 values per result: [0] acc_hit, [1] n_pos, [2] n_neg, [3..9] tp, [10..16] fp at the
                              * score thresholds 0.1 0.3 0.5 0.7 0.8 0.9 0.95 (as float32); the rest 0 */

/* The per-step counts behind the reference's monitoring block (libraries/metrics.py: Accuracy.call :60-83,
 * PrecisionRecall.call and _calc_binary_metrics :103-161, as update_metrics :164-198 calls them with weights = cared),
 * for encode_background_as_zeros and use_sigmoid_score both true.  Per anchor, in float32: s_c = 1 / (1 + exp(-x_c)),
 * score = max_c s_c; predicted label = (first maximum of x_c) + 1 where any s_c > 0.5, else 0.  acc_hit counts predicted
 * label == label over all anchors (an ignored anchor, label -1, never matches), n_pos label > 0, n_neg label == 0,
 * tp[i] label > 0 and score > t_i, fp[i] label == 0 and score > t_i; fn[i] = n_pos - tp[i], tn[i] = n_neg - fp[i].  A NaN
 * logit compares false everywhere.  labels [batch][A] int32 (>0 class, 0 background, -1 ignored).  cls_preds NULL: the head
 * map the last forward pass or training step of this handle left on the device, as pp_head_loss reads it; otherwise
 * [batch][A][num_class] float32 logits, which are uploaded and counted instead.  counts [PP_METRICS_COUNTS].  Integer
 * sums: the same input gives the same bytes on every run.  Host pointers; synchronous.  PP_ERR_STATE while a training step
 * is in flight, PP_ERR_UNSUPPORTED for the shapes pp_head_loss refuses. */
int pp_head_metrics(pp_handle h, const int32_t* labels, int32_t batch, const float* cls_preds, int64_t* counts);

/* on = 1: every following training step (pp_train_step*, all four entry points) counts the same on the labels it trains on,
 * inside its captured graph right behind the loss (two more graph nodes); on = 0, the default: nothing is added and every
 * output is what it was before the switch existed.  The switch is part of what a captured step graph is keyed on: a
 * change re-captures it once.  PP_ERR_ARG for another value, PP_ERR_STATE while a step is in flight. */
int pp_set_train_metrics(pp_handle h, int32_t on);
int pp_get_train_metrics_enabled(pp_handle h, int32_t* on);
/* The counts of the last step, after its pp_train_step_wait.  PP_ERR_STATE when that step ran with the switch off, when no
 * step has run, or while one is in flight. */
int pp_get_train_metrics(pp_handle h, int64_t* counts);

/* ---- detection during training: a trainer's weights into the detector, on the device --------------------------------- */

typedef struct pp_publish_stats {
    int64_t publishes;           /* successful pp_publish_train_weights calls on this handle */
    int64_t reallocations;       /* ... of them, those that allocated the weight arrays (the first; the first after a
                                  * pp_finalize_weights) */
    int64_t graph_invalidations; /* times published weights dropped the captured inference graphs: every reallocation,
                                  * and every change of the set of layers on the float32 fallback (a publish, or
                                  * pp_set_gemm_precision on published weights) */
    int64_t f32_fallback_layers; /* separable layers and transposed convolutions of the handle's CURRENT weights that run on
                                  * the float32 matrix instruction -- also for weights loaded by pp_finalize_weights */
} pp_publish_stats;

/* params_dev / state_dev: the flat device buffers of pp_train_layout (only read).  Kernels on the handle's stream -- so
 * behind a training step or optimizer update enqueued there -- write every array pp_finalize_weights would produce from
 * the same tensors, with the same bytes: BatchNorm folded from the MOVING statistics (frozen or not), transposed
 * kernels, the head matrix, the float16 piece pairs and their range rule (a layer with a folded |w| >= 32768 runs in
 * PP_PREC_F32 by itself).  Returns with the weights usable (one small read-back of the range flags).  The first publish
 * on a handle allocates the arrays -- pp_set_weight need never have been called; a later one writes the same
 * allocations and keeps the captured inference graphs unless the set of fallback layers changed.  The published values are
 * the handle's weights from then on (pp_set_gemm_precision re-derives from them); a later pp_set_weight +
 * pp_finalize_weights replaces them.  PP_ERR_STATE while a training step is in flight. */
int pp_publish_train_weights(pp_handle h, const float* params_dev, const float* state_dev);
int pp_publish_info(pp_handle h, pp_publish_stats* out);

/* ---- tracking: identities and velocities across the frames of a live feed ---------------------------------------------
 * One track table per STREAM: frame b of every pass belongs to stream b, a handle has max_batch streams, and a pass that
 * ran with tracking on advances each of its `batch` streams by one step behind its post-process (one more kernel in the
 * pass's chain and its captured graph; the state never leaves the device).  The step, in float64 with + - * / and
 * comparisons only (tracking.py of the Python package restates it operation for operation, and the kernel equals it bit
 * for bit): predict every live track by the stream's dt (constant velocity, white-acceleration process noise q_acc);
 * associate tracks and detection rows greedily by the smallest (BEV squared distance, slot, row) among the pairs with
 * d2 <= gate * gate (and, class_aware, equal labels); update the matched tracks (scalar-gain Kalman update per axis,
 * measurement variance r_pos; sizes blended by size_alpha; yaw, score, label from the row); age the others (freed after
 * more than max_misses misses in a row); open a track in the lowest free slot for every unmatched row with
 * score >= birth_score, in row order (no slot left: the row is dropped and the stream's overflow count goes up); output
 * the live tracks in ascending slot order.  The reference has no tracker: nothing here is parity with it. */
#define PP_TRACK_MAX 64 /* tracks per stream */

typedef struct pp_track_config {
    double gate;        /* association gate in metres (BEV centre distance, inclusive), > 0 */
    double q_acc;       /* variance of the white acceleration, (m/s^2)^2, > 0 */
    double r_pos;       /* measurement variance of a detection's centre per axis, m^2, > 0 */
    double p0_pos;      /* position variance of a new track, m^2, > 0 */
    double p0_vel;      /* velocity variance of a new track, (m/s)^2, > 0 */
    double size_alpha;  /* weight of the new row in the size blend, 0 .. 1 */
    double birth_score; /* least score of a row that may open a track */
    double period;      /* seconds a stream advances by when pp_set_track_dt gave no value, > 0 */
    int32_t max_misses; /* >= 0: a track is freed at its (max_misses + 1)-th miss in a row */
    int32_t min_hits;   /* >= 1: `confirmed` becomes 1 at that many hits and stays */
    int32_t class_aware;/* != 0: a pair must have equal labels */
    int32_t reserved;
} pp_track_config;

typedef struct pp_track {
    double state[6];    /* x y z vx vy vz (lidar frame; after the step's update) */
    double size[3];     /* w l h */
    double yaw;         /* of the last matched row */
    float score;        /* of the last matched row */
    int32_t id;         /* per stream, from 1, never reused until a reset */
    int32_t label;
    int32_t hits, misses, confirmed;
    int32_t det_row;    /* the row of this step's detections the track was matched with or opened from, else -1 */
    int32_t reserved;
} pp_track;

/* cfg == NULL: tracking off (the default); the tables and the configuration are kept.  Otherwise the configuration is
 * validated (PP_ERR_ARG naming the field: a non-finite value, gate / q_acc / r_pos / p0_pos / p0_vel / period <= 0,
 * size_alpha outside 0..1, max_misses < 0, min_hits < 1), written to device memory and tracking is on from the next
 * pp_detect_async.  On / off is part of what a captured pass is keyed on; the parameters are not (the kernel reads them
 * from device memory).  PP_ERR_UNSUPPORTED when the handle's rows per frame (pp_get_detection_rows) exceed the 128 the
 * step's row bitmask holds -- also raised by the pass and by pp_track_update after a later change of the class mode;
 * PP_ERR_STATE while a training step is in flight.  The stage calls (pp_predict ...) never track. */
int pp_set_tracking(pp_handle h, const pp_track_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_tracking(pp_handle h, int32_t* on, pp_track_config* cfg_out);
/* Seconds by which the NEXT tracked step advances streams 0 .. batch - 1 (each finite and > 0, else PP_ERR_ARG naming the
 * stream).  The values travel through a page-locked ring slot into device memory on the handle's stream, ahead of the pass
 * that consumes them: two passes queued without a pp_sync each see their own.  A stream without a value advances by
 * cfg.period.  A value is spent by the next tracked pass (or pp_track_update) that covers its stream, also when that pass
 * flags the stream's frame; an UNTRACKED pass in between does not touch it.  PP_ERR_STATE before the first
 * pp_set_tracking and while a training step is in flight. */
int pp_set_track_dt(pp_handle h, const double* dt, int32_t batch);
/* The tables of the last tracked pass or pp_track_update (waits for the stream): tracks [batch][PP_TRACK_MAX] (the live
 * tracks of stream b in ascending slot order, zeros behind them), n_tracks [batch], overflow [batch] (rows dropped for
 * want of a slot since the last reset; may be NULL).  PP_ERR_STATE when the last pass ran untracked (or none has run);
 * PP_ERR_NUMERIC where pp_get_detections would return it -- a flagged frame leaves its stream's table untouched. */
int pp_get_tracks(pp_handle h, pp_track* tracks, int32_t* n_tracks, int32_t* overflow);
/* The same step on the handle's same tables, on host-given rows: dets [batch][rows] (rows 0 .. n_dets[b] - 1 of stream b
 * are read: box3d_lidar, score, label), 0 <= n_dets[b] <= rows <= 128, dt [batch] or NULL (cfg.period).  Uploads into
 * scratch of its own (a pass's results stay fetchable with pp_get_detections), synchronous; pp_get_tracks then returns
 * this step's tables.  A count with bit 30 set (how a pass marks a frame whose head maps were not finite) is taken as
 * it is: that stream stays untouched, as in a pass.  PP_ERR_ARG for rows < 1; PP_ERR_STATE before the first pp_set_tracking (tracking need not be on) and
 * while a training step is in flight. */
int pp_track_update(pp_handle h, const pp_detection* dets, const int32_t* n_dets, int32_t rows, int32_t batch,
                    const double* dt);
/* stream 0 .. max_batch - 1, or -1 for all: frees every track, the next id is 1 again, overflow 0, the previous ego pose
 * (pp_set_track_pose) forgotten (waits for the stream).
 * PP_ERR_STATE while a training step is in flight, like every tracking call that queues work or writes the tables. */
int pp_track_reset(pp_handle h, int32_t stream);
/* Per stream, [max_batch] each (any may be NULL): live tracks, the next id, overflow.  Waits for the stream and only
 * reads, so it is allowed while a training step is in flight (it then waits for that step's launches as well). */
int pp_track_info(pp_handle h, int32_t* live, int32_t* next_id, int32_t* overflow);
/* Ego motion.  The tracks of a stream live in the sensor frame of its latest step.  poses [batch][3][4]: the
 * sensor-to-fixed transforms [R | t] (row-major, as pp_sweeps_accumulate takes them) of the NEXT tracked step -- the
 * pass's or pp_track_update's -- for streams 0 .. batch - 1.  Before its predict stage that step carries the live tracks of
 * a posed stream from the sensor frame of the stream's previous posed step into the current one: with
 * M = R_c^T R_p, u = R_c^T (t_p - t_c) (pp_sweeps_accumulate's operation order), x' = ((M00 x + M01 y) + M02 z) + u0,
 * vx' = (M00 vx + M01 vy) + M02 vz (the other axes alike) and yaw' = yaw + (psi_c - psi_p), psi = atan2(R10, R00) taken
 * on the host; a track's velocity is then the object's velocity over ground in the current sensor axes.  A stream's
 * first posed step carries nothing; a stream without a pose steps exactly as without this call and keeps its previous
 * pose.  The poses travel as pp_set_track_dt's values do and are spent likewise, also by a step that flags the stream's
 * frame (the previous pose then stays: the next posed step carries over the whole motion); pp_track_update does not
 * clear them; pp_track_reset forgets the stream's previous pose.  Refused before anything is queued: PP_ERR_ARG for a
 * NULL handle or argument, a batch out of range, a pose that is not finite or whose rotation is further than 1e-6 from
 * orthonormal (naming the stream); PP_ERR_STATE before the first pp_set_tracking and while a training step is in flight. */
int pp_set_track_pose(pp_handle h, const double* poses /* [batch][3][4] */, int32_t batch);
/* pp_get_tracks' rows of the same step in the FIXED frame: position R x + t, velocity R v, yaw + psi_c, every other
 * field copied; n_tracks[b] is -1 (and the stream's rows zero) for a stream whose step had no pose.  Errors as
 * pp_get_tracks. */
int pp_get_tracks_fixed(pp_handle h, pp_track* tracks, int32_t* n_tracks);

/* ---- Obstacle costmap per frame (costmap.py states the rule): the resident points, the last pass's detections or the
 * streams' tracks as one int8 grid per frame in the layout of nav_msgs/OccupancyGrid: -1 unknown, 0 free, up to 100
 * lethal; row-major grid[iy * width + ix], origin (x_min, y_min), in the sensor frame of that frame.  An opt-in stage
 * behind the pass: plain launches on the handle's stream, not part of a captured pass. ---- */
#define PP_COSTMAP_MAX_STEPS 8      /* predicted footprints per track */
#define PP_COSTMAP_MAX_CELLS 262144 /* width * height */

typedef struct pp_costmap_config {
    double x_min;          /* the grid's origin, metres */
    double y_min;
    double resolution;     /* metres per cell, > 0 */
    double z_min;          /* a point counts as an obstacle with z_min <= z <= z_max */
    double z_max;
    double pad;            /* metres added to a footprint's half extents, >= 0 */
    double min_score;      /* detections under it leave no footprint */
    double horizon_dt;     /* seconds between two predicted footprints of a track, > 0 */
    int32_t width;         /* cells; width, height >= 1, width * height <= PP_COSTMAP_MAX_CELLS */
    int32_t height;
    int32_t min_points;    /* >= 1: counted points that make a cell an obstacle */
    int32_t objects;       /* 0 none, 1 the last pass's detections, 2 the streams' tracks */
    int32_t confirmed_only;/* tracks: only the confirmed ones */
    int32_t horizon_steps; /* 0 .. PP_COSTMAP_MAX_STEPS predicted footprints per track */
    int32_t point_cost;    /* 0 .. 100 */
    int32_t object_cost;   /* 0 .. 100 */
    int32_t predict_cost[PP_COSTMAP_MAX_STEPS]; /* 0 .. 100 each of the first horizon_steps; the rest is ignored */
} pp_costmap_config;

/* cfg == NULL: the stage off (the default); its buffers are kept.  Otherwise the configuration is validated (PP_ERR_ARG
 * naming the field) and max_batch x cells x (4 + 1) bytes of count words and grid, the count tap (4 bytes a cell) and
 * the footprint tables are allocated (rows padded to 4 cells); PP_ERR_HIP naming the bytes when the device cannot hold
 * them.  PP_ERR_STATE while a training step is in flight. */
int pp_set_costmap(pp_handle h, const pp_costmap_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_costmap_config(pp_handle h, int32_t* on, pp_costmap_config* cfg_out);
/* Queues the stage on the resident frames behind whatever the handle's stream holds: a clear of the count words, then
 * three launches whatever the batch (footprints, points, compose).  The stage's read of the resident frames is ordered
 * against a later upload or flip as a pass's read is.  Refused before anything is queued with PP_ERR_STATE: the stage is
 * off; no frames are resident; a training step is in flight; objects = detections and no pass has run on the resident
 * batch; objects = tracks before the first pp_set_tracking. */
int pp_costmap_async(pp_handle h);
/* The grids of the last pp_costmap_async (waits for the stream): grid int8 [batch][height][width]; counts int32 of the
 * same shape (the points counted per cell) or NULL.  PP_ERR_STATE when no stage has run, PP_ERR_ARG when batch is not
 * that run's.  With objects = detections, PP_ERR_NUMERIC where pp_get_detections would return it: a flagged frame takes
 * no objects; every frame's grid is still written. */
int pp_get_costmaps(pp_handle h, int8_t* grid, int32_t* counts, int32_t batch);
/* Per frame of that run, [batch] each (either may be NULL): the frame's points inside the grid, its footprints.
 * Errors as pp_get_costmaps, without PP_ERR_NUMERIC. */
int pp_costmap_info(pp_handle h, int32_t* points_in_grid, int32_t* footprints, int32_t batch);

/* ---- Rolling occupancy map per stream in the fixed (odometry) frame (occupancy.py states the rule): the resident points
 * of frame b, under the stream's sensor-to-fixed pose, update an int16 log-odds grid (units of 0.01 nat) of width x
 * height cells that stays centred on the sensor: the cell of an endpoint in the height band takes +l_hit, every cell a ray
 * from the sensor's cell to an endpoint's cell crosses takes -l_miss (one ray per end cell, an integer walk from the
 * sensor outwards), clamped to [l_min, l_max].  Published as int8 in the layout of nav_msgs/OccupancyGrid: -1 unknown,
 * else cost_table[L - l_min] (0 .. 100); row-major grid[iy * width + ix], origin (ox, oy) * resolution in the fixed frame.
 * An opt-in stage: plain launches on the handle's stream, not part of a captured pass. ---- */
#define PP_OCC_MAX_CELLS 1048576 /* width * height */

typedef struct pp_occupancy_config {
    double resolution;     /* metres per cell, > 0 */
    double z_min;          /* a used row with z >= z_min is a hit, below it a ground return (sensor-frame z) */
    double z_max;          /* rows above it are ignored */
    double max_range;      /* metres in the sensor's x y plane, > 0; rows beyond it are ignored */
    int32_t width;         /* cells; width, height >= 1, width * height <= PP_OCC_MAX_CELLS */
    int32_t height;
    int32_t l_hit;         /* 1 .. 1000 */
    int32_t l_miss;        /* 1 .. 1000 */
    int32_t l_min;         /* -1000 <= l_min < 0 */
    int32_t l_max;         /* 0 < l_max <= 1000 */
} pp_occupancy_config;

/* cfg == NULL: the stage off (the default); buffers and maps are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field) and, for another shape, max_batch x cells x (4 + 1 + 2 x (2 + 1)) bytes of marks and two
 * copies of log-odds and grid are allocated (rows padded to 4 cells; PP_ERR_HIP naming the bytes when the device cannot
 * hold them).  cost_table: n_table = l_max - l_min + 1 values 0 .. 100, table[i] the cost of L = l_min + i; NULL (n_table
 * ignored): floor(100 / (1 + exp(-(l_min + i) / 100)) + 0.5), computed here on the host.  A configuration with another
 * width, height, resolution or log-odds field than the last forgets every stream's map; z_min, z_max, max_range and the
 * table may change under a map.  Waits for the stream.  PP_ERR_STATE while a training step is in flight. */
int pp_set_occupancy(pp_handle h, const pp_occupancy_config* cfg, const int8_t* cost_table, int32_t n_table);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_occupancy_config(pp_handle h, int32_t* on, pp_occupancy_config* cfg_out);
/* Updates the maps of streams 0 .. batch - 1 from the resident frames 0 .. batch - 1 under poses [batch][3][4], the
 * sensor-to-fixed transforms [R | t] (row-major, as pp_sweeps_accumulate takes them): queued behind whatever the handle's
 * stream holds -- the poses through a small device buffer, a clear of the marks, then three launches whatever the batch
 * (endpoints, rays, apply).  The other streams' maps stay as they are.  The read of the resident frames is ordered
 * against a later upload or flip as a pass's read is.  Refused before anything is queued: PP_ERR_STATE when the stage is
 * off, no frames are resident or a training step is in flight; PP_ERR_ARG for a NULL argument, a batch that is not the
 * resident one, a pose that is not finite or further than 1e-6 from orthonormal (naming the stream), or a translation
 * with |t_x| / resolution or |t_y| / resolution >= 2^30. */
int pp_occupancy_update_async(pp_handle h, const double* poses /* [batch][3][4] */, int32_t batch);
/* The maps of the streams of the last update (waits for the stream): grid int8 [batch][height][width], logodds int16 of
 * the same shape or NULL, origins [batch][2] the fixed-frame x y of each window's cell (0, 0).  A stream reset since then
 * reads all unknown, with a NaN origin.  PP_ERR_STATE when no update has run since the map's configuration was given,
 * PP_ERR_ARG when batch is not that update's. */
int pp_get_occupancy(pp_handle h, int8_t* grid, int16_t* logodds, double* origins, int32_t batch);
/* Per frame of that update, [batch] each (any may be NULL): rows that hit, ground rows, ignored rows, cells that took a
 * hit, cells that were passed and not hit, cells of the new window that started unknown because the old window did not
 * hold them (all of them at a stream's first update).  Errors as pp_get_occupancy. */
int pp_occupancy_info(pp_handle h, int32_t* hits, int32_t* ground, int32_t* ignored, int32_t* cells_hit,
                      int32_t* cells_free, int32_t* cleared, int32_t batch);
/* stream 0 .. max_batch - 1, or -1 for all: forgets the stream's map; its next update starts from an unknown window.
 * PP_ERR_STATE while a training step is in flight. */
int pp_occupancy_reset(pp_handle h, int32_t stream);

/* ---- Obstacle inflation behind either grid, and of any int8 OccupancyGrid (inflation.py states the rule): a cell with
 * g >= lethal_threshold is an obstacle; d2 of a cell is its exact squared Euclidean distance in cells to the nearest
 * obstacle of the grid, looked for within R = ceil(inflation_radius / resolution) cells (R * R + 1: none in reach);
 * t = table[d2] (0 for none); a known cell (g >= 0) reads max(g, t), an unknown one t where t >= unknown_min_cost, else
 * -1.  table[d2], with d = sqrt(d2) * resolution: 100 for d2 = 0, 99 for d <= inscribed_radius,
 * floor(98 * exp(-cost_scaling_factor * (d - inscribed_radius)) + 0.5) for d <= inflation_radius, else 0.  The device
 * only looks the table up: integer arithmetic throughout.  An opt-in stage: one plain launch on the handle's stream
 * whatever the batch, not part of a captured pass. ---- */
#define PP_INFLATE_MAX_RADIUS 64 /* R, cells */

typedef struct pp_inflation_config {
    double resolution;           /* metres per cell, > 0: the source's (the table is built for it) */
    double inscribed_radius;     /* metres, >= 0 */
    double inflation_radius;     /* metres, >= inscribed_radius; ceil(inflation_radius / resolution) <= PP_INFLATE_MAX_RADIUS */
    double cost_scaling_factor;  /* 1 / m, > 0 */
    int32_t lethal_threshold;    /* 1 .. 100 */
    int32_t unknown_min_cost;    /* 1 .. 100 */
} pp_inflation_config;

enum { PP_INFLATE_COSTMAP = 0, PP_INFLATE_OCCUPANCY = 1 }; /* `source`: the grids of pp_costmap_async / of the occupancy maps */

/* cfg == NULL: the source's inflation off (the default); its buffers are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field).  table: n_table = R * R + 1 values 0 .. 100 (PP_ERR_ARG otherwise); NULL (n_table
 * ignored): the table above, computed here on the host.  Waits for the stream.  PP_ERR_STATE while a training step is in
 * flight. */
int pp_set_inflation(pp_handle h, int32_t source, const pp_inflation_config* cfg, const int8_t* table, int32_t n_table);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given for the source (zeros before the first). */
int pp_get_inflation_config(pp_handle h, int32_t source, int32_t* on, pp_inflation_config* cfg_out);
/* Inflates the grids of the source's last run (pp_costmap_async / pp_occupancy_update_async), all of its frames / streams:
 * queued behind whatever the handle's stream holds, one launch.  Reads the source's device grid in place (rows of
 * (width + 3) & ~3 cells) and writes buffers of its own, made here for the source's shape: never the source's grid or
 * log-odds.  Refused before anything is queued, PP_ERR_STATE: the source's inflation or the source stage is off, the
 * source has not run, its resolution is not the one the table was built for, a training step is in flight.  The
 * costmap's resolution is that of its last run, the cells that lie there, whatever pp_set_costmap has given since. */
int pp_inflate_async(pp_handle h, int32_t source);
/* The grids of the source's last pp_inflate_async (waits for the stream): grid int8 [batch][height][width]; dist2 uint16
 * of the same shape or NULL, the squared cell distance to the nearest obstacle (R * R + 1: none in reach).  A stream of
 * the occupancy source that was reset before the call reads all unknown (its origin is pp_get_occupancy's, as every
 * stream's).  PP_ERR_STATE when none has run, PP_ERR_ARG when batch is not that run's. */
int pp_get_inflated(pp_handle h, int32_t source, int8_t* grid, uint16_t* dist2, int32_t batch);
/* Per grid of that run, [batch] each (either may be NULL): obstacle cells, cells the inflation changed.  Errors as
 * pp_get_inflated. */
int pp_inflation_info(pp_handle h, int32_t source, int32_t* lethal, int32_t* raised, int32_t batch);
/* Without a handle: grids int8 [batch][height][width] in host memory (height * width <= PP_OCC_MAX_CELLS, batch <= 65535)
 * -> out of the same shape, dist2 uint16 of the same shape or NULL, counts int32 [batch][2] (lethal, raised) or NULL.
 * cfg and table as pp_set_inflation takes them. */
int pp_inflate_grids(int device, const int8_t* grids, int32_t batch, int32_t height, int32_t width,
                     const pp_inflation_config* cfg, const int8_t* table, int32_t n_table, int8_t* out, uint16_t* dist2,
                     int32_t* counts);

/* ---- Navigation function behind either inflation, and of any int8 OccupancyGrid (navfn.py states the rule): the
 * cost-to-go field from one goal cell per grid and the path that descends it from one start cell.  Cell cost c uint16, 0 =
 * blocked: g >= lethal_cost is blocked; an unknown cell is blocked unless allow_unknown, then c = neutral_cost +
 * cost_factor * unknown_cost; else c = neutral_cost + cost_factor * g.  Orthogonal moves weigh 5, diagonal ones
 * (connectivity 8) 7, and a diagonal move needs both cells beside it unblocked.  pot(goal) = 0; pot(p) = min over
 * admissible reached neighbours q of pot(q) + w * c(p); PP_NAVFN_UNREACHED elsewhere.  The ranges below bound c by
 * 50 + 5 * 100 = 550 and a step by 7 * 550 = 3850, and 3850 * PP_OCC_MAX_CELLS < 2^32 - 1: a uint32 potential cannot
 * overflow on any grid these calls admit.  Integer arithmetic throughout; the field is the unique fixed point of the
 * relaxation, so the number of rounds never shows in a result.  An opt-in stage: plain launches on the handle's stream,
 * not part of a captured pass. ---- */
#define PP_NAVFN_UNREACHED 0xFFFFFFFFu
#define PP_NAVFN_MAX_PATH 4096 /* cells */

typedef struct pp_navfn_config {
    int32_t lethal_cost;    /* 1 .. 100 */
    int32_t neutral_cost;   /* 1 .. 50 */
    int32_t cost_factor;    /* 0 .. 5 */
    int32_t allow_unknown;  /* 0 / 1 */
    int32_t unknown_cost;   /* 0 .. 100 */
    int32_t connectivity;   /* 4 / 8 */
    int32_t max_path;       /* 1 .. PP_NAVFN_MAX_PATH: cells a returned path may hold */
    int32_t queued_rounds;  /* 0 .. 4096: relaxation rounds pp_navfn_async queues (0: a default from the grid's shape);
                             * timing only, never a result */
} pp_navfn_config;

/* cfg == NULL: the source's stage off (the default); its buffers are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field).  `source` is the inflation's: PP_INFLATE_COSTMAP / PP_INFLATE_OCCUPANCY.  Waits for the
 * stream.  PP_ERR_STATE while a training step is in flight. */
int pp_set_navfn(pp_handle h, int32_t source, const pp_navfn_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given for the source (zeros before the first). */
int pp_get_navfn_config(pp_handle h, int32_t source, int32_t* on, pp_navfn_config* cfg_out);
/* Queues the field and the paths on the grids of the source's last pp_inflate_async behind whatever the handle's stream
 * holds: goals int32 [batch][2] cells (x, y); starts likewise, or NULL (no paths, path_state 4).  Reads the inflated
 * grid in place and never writes it; a stream reset before that inflation reads all unknown.  Queues queued_rounds
 * relaxation rounds and returns; the getters queue what is still missing.  Refused before anything is queued,
 * PP_ERR_STATE: the stage or the source's inflation is off, that inflation has not run, a training step is in flight;
 * PP_ERR_ARG: a batch that is not the inflation run's, goals NULL, a bad source. */
int pp_navfn_async(pp_handle h, int32_t source, const int32_t* goals, const int32_t* starts, int32_t batch);
/* The results of the source's last pp_navfn_async (waits for the stream, and runs further relaxation rounds until every
 * grid's field stands: always the exact field).  pot uint32 [batch][height][width]; paths int32 [batch][max_path][2]
 * cells (x, y) and path_len int32 [batch]; each may be NULL.  PP_ERR_STATE when none has run, PP_ERR_ARG when batch is
 * not that run's, PP_ERR_INTERNAL should height * width rounds not suffice (they provably do). */
int pp_get_navfn(pp_handle h, int32_t source, uint32_t* pot, int32_t* paths, int32_t* path_len, int32_t batch);
/* Per grid of that run, [batch] each (any may be NULL): goal_state 0 ok / 1 blocked / 2 outside; path_state 0 reached /
 * 1 start unreached or blocked / 2 start outside / 3 cut at max_path / 4 no start; relaxation rounds run; cells reached.
 * Errors as pp_get_navfn. */
int pp_navfn_info(pp_handle h, int32_t source, int32_t* goal_state, int32_t* path_state, int32_t* rounds,
                  int32_t* reached, int32_t batch);
/* Without a handle: grids int8 [batch][height][width] in host memory (height * width <= PP_OCC_MAX_CELLS, batch <= 65535),
 * goals and starts as above -> pot, paths, path_len as pp_get_navfn gives them (each may be NULL) and info int32
 * [4][batch] or NULL: goal_state, path_state, rounds, reached. */
int pp_navfn_grids(int device, const int8_t* grids, int32_t batch, int32_t height, int32_t width,
                   const pp_navfn_config* cfg, const int32_t* goals, const int32_t* starts, uint32_t* pot, int32_t* paths,
                   int32_t* path_len, int32_t* info);

/* ---- Local planner behind either navigation function, and of any int8 OccupancyGrid with its field
 * (local_planner.py states the rule): a window of nv * nw (v, w) samples rolled forward from one pose per grid over the
 * inflated grid, each scored on the cost-to-go field, and the least key's sample as the command.  Integers only: a
 * position is int32 sub-cells (PP_LOCAL_SUB per cell), a heading one of PP_LOCAL_HEADINGS ticks (tick 0 is +x, ticks
 * grow towards +y), and cos / sin come from a table of rint(cos / sin(2 pi h / 4096) * 2^14) that travels with the
 * configuration.  Sample s = i * nw + j: sv = v0 + i * dv sub-cells per step (negative: reverse), sw = w0 + j * dw
 * ticks per step, |sv| <= 1024 and |sw| <= 512.  A step: X += (sv * C[h] + 8192) >> 14, Y likewise with S[h], then
 * h = (h + sw) & 4095; the cell (X >> 10, Y >> 10) outside the grid ends the sample as OUTSIDE, a blocked one
 * (g >= lethal_cost, or unknown while allow_unknown is 0: the source's pp_navfn_config) as COLLISION, else occ =
 * max(occ, g) with unknown_cost for an unknown cell.  The scored cell is the end pose pushed `lookahead` sub-cells along
 * the final heading; outside, blocked or PP_NAVFN_UNREACHED there makes the sample UNREACHED.  score = pot_weight * pot +
 * occ_weight * occ + speed_weight * (1024 - |sv|) + turn_weight * |sw| < 2^41, key = (score << 14) | s, 2^64 - 1 for an
 * invalid sample; the least key wins.  cmd_state: 4 the field has no goal, 3 the pose's cell is outside, blocked or
 * unreached, 2 arrived (pot 0 at the pose's cell), 1 no valid sample, 0 ok.  An opt-in stage: plain launches on the
 * handle's stream, not part of a captured pass. ---- */
#define PP_LOCAL_SUB 1024           /* sub-cells per cell */
#define PP_LOCAL_HEADINGS 4096      /* heading ticks per revolution */
#define PP_LOCAL_MAX_SAMPLES 16384  /* nv * nw at most */
#define PP_LOCAL_MAX_STEPS 256
#define PP_LOCAL_MAX_LOOKAHEAD 16384 /* sub-cells */
#define PP_LOCAL_RESULT 8           /* int32 words per grid: cmd_state, best, sv, sw, n_ok, n_outside, n_collision, n_unreached */

typedef struct pp_local_plan_config {
    int32_t nv;            /* >= 1: velocity samples; nv * nw <= PP_LOCAL_MAX_SAMPLES */
    int32_t nw;            /* >= 1: turn-rate samples */
    int32_t steps;         /* 1 .. PP_LOCAL_MAX_STEPS */
    int32_t lookahead;     /* 0 .. PP_LOCAL_MAX_LOOKAHEAD sub-cells */
    int32_t pot_weight;    /* 0 .. 255 */
    int32_t occ_weight;    /* 0 .. 65535 */
    int32_t speed_weight;  /* 0 .. 65535 */
    int32_t turn_weight;   /* 0 .. 65535 */
} pp_local_plan_config;

/* cfg == NULL: the source's stage off (the default); its buffers are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field) and trig, int32 [n_trig][2] = (C[h], S[h]), is uploaded: n_trig must be
 * PP_LOCAL_HEADINGS and every |value| <= 16384.  `source` is the inflation's.  Waits for the stream.  PP_ERR_STATE while
 * a training step is in flight. */
int pp_set_local_plan(pp_handle h, int32_t source, const pp_local_plan_config* cfg, const int32_t* trig, int32_t n_trig);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given for the source (zeros before the first). */
int pp_get_local_plan_config(pp_handle h, int32_t source, int32_t* on, pp_local_plan_config* cfg_out);
/* Queues the rollout and the command on the grids and fields of the source's last pp_navfn_async behind the rounds that
 * call queued: poses int32 [batch][3] = (X, Y, h) sub-cells and a tick (h is taken & 4095), windows int32 [batch][4] =
 * (v0, dv, w0, dw).  Reads the inflated grid and the field in place and never writes them.  Refused before anything is
 * queued, PP_ERR_STATE: the stage or the source's navigation function is off, that navigation function has not run, the
 * inflated grids were re-made since it ran (any pp_inflate_async of the source: it reuses the buffers, so the field on
 * the handle belongs to grids that are gone -- pp_navfn_async again), a training step is in flight; PP_ERR_ARG: a batch that is not the navigation
 * function run's, poses or windows NULL, a sample with |sv| > 1024 or |sw| > 512, a bad source. */
int pp_local_plan_async(pp_handle h, int32_t source, const int32_t* poses, const int32_t* windows, int32_t batch);
/* The results of the source's last pp_local_plan_async.  First settles the field as pp_get_navfn does; if that queued a
 * further round, or keys are asked for and were not stored, the rollout and the command are queued again, so a fetched
 * command always rests on the exact field.  result int32 [batch][PP_LOCAL_RESULT]; score uint64 [batch] (0 unless
 * cmd_state is 0); traj int32 [batch][steps + 1][3] poses, the start included (zeros unless cmd_state is 0); keys uint64
 * [batch][nv * nw]; each may be NULL.  PP_ERR_STATE when none has run, a pp_navfn_async of the source came after it, or
 * the launches have to be queued again and the inflated grids were re-made meanwhile (a pp_inflate_async of the source
 * since its pp_navfn_async, whether or not the buffers moved; when nothing has to be queued again the results are
 * copied as the launches left them); PP_ERR_ARG when batch is not that run's. */
int pp_get_local_plan(pp_handle h, int32_t source, int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys,
                      int32_t batch);
/* Without a handle: grids int8 and pots uint32 [batch][height][width] in host memory (height * width <=
 * PP_OCC_MAX_CELLS, batch <= 65535); of navfn_cfg only lethal_cost, allow_unknown and unknown_cost are read; trig as
 * pp_set_local_plan takes it; goal_state int32 [batch] or NULL (all 0): nonzero gives cmd_state 4; outputs as
 * pp_get_local_plan gives them, each may be NULL. */
int pp_local_plan_grids(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height, int32_t width,
                        const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg, const int32_t* trig,
                        int32_t n_trig, const int32_t* poses, const int32_t* windows, const int32_t* goal_state,
                        int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys);

/* ---- Movers of the local planner: time-indexed collision of every rolled sample with the stream's live tracks
 * (local_planner.py states both rules).  A mover is six int32 (mx, my, mvx, mvy, r_hard, r_soft): its position at step
 * 0 in sub-cells of the grid's frame (it may lie outside the grid), its movement per rollout step, and two radii, all
 * in sub-cells; |mx|, |my| <= 2^29, |mvx|, |mvy| <= PP_LOCAL_MAX_MOVER_SPEED, 0 <= r_hard <= r_soft <=
 * PP_LOCAL_MAX_MOVER_RADIUS, at most PP_LOCAL_MAX_MOVERS per grid.  THE ROLLOUT: a sample that is still alive after
 * the static test of step k (OUTSIDE, then COLLISION, then occ) and has k <= horizon looks at every mover in table
 * order: dx = X - (mx + k * mvx), dy likewise, d2 = dx * dx + dy * dy in exact integers; d2 <= r_hard^2 ends the sample
 * as DYNAMIC (reason 4), otherwise d2 <= r_soft^2 sets near = max(near, horizon + 1 - k).  Neither the start pose nor
 * the lookahead point is tested.  The score gains mover_weight * near (it stays below 2^41).  THE TABLE
 * (pp_local_plan_movers_async) comes from the stream's track slots on the device, in float64 with every operation
 * rounded on its own: a slot's x y z vx vy vz w l in the grid's frame -- as it stands for the costmap source; carried
 * into the fixed frame by the pose of the stream's last posed tracking step for the occupancy source, with the
 * expressions that make pp_get_tracks_fixed's rows (a stream that has had no posed step: n_movers = -1, no movers) --
 * give MX = floor(((x - ox) / res) * 1024), MVX = rint(((vx * dt) / res) * 1024) (half to even), RH = ceil(((fmax(w, l) *
 * 0.5 + pad_hard) / res) * 1024) clipped to [0, PP_LOCAL_MAX_MOVER_RADIUS], and MY, MVY, RS likewise.  Live slots
 * (confirmed ones where confirmed_only is set) become movers in ascending slot order; one with a non-finite input, |MX|
 * or |MY| > 2^29 or |MVX| or |MVY| > PP_LOCAL_MAX_MOVER_SPEED is skipped and counted. ---- */
#define PP_LOCAL_MAX_MOVERS 64          /* per grid: PP_TRACK_MAX */
#define PP_LOCAL_MAX_MOVER_SPEED 16384  /* sub-cells per step */
#define PP_LOCAL_MAX_MOVER_RADIUS 32767 /* sub-cells */
#define PP_LOCAL_MOVER_INFO 4           /* int32 words per grid: n_movers (-1: no posed step), n_skipped, n_dynamic, near */

typedef struct pp_local_mover_config {
    double pad_hard;         /* metres added to max(w, l) / 2 for r_hard: the robot's radius belongs here; finite, >= 0 */
    double pad_soft;         /* ... for r_soft; finite, >= pad_hard */
    int32_t horizon;         /* 0 .. PP_LOCAL_MAX_STEPS: steps over which a prediction is trusted */
    int32_t mover_weight;    /* 0 .. 65535 */
    int32_t confirmed_only;  /* 0 / 1: only confirmed tracks become movers */
    int32_t reserved;        /* 0 */
} pp_local_mover_config;

/* cfg == NULL: the source's movers off (the default); the buffers are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field).  Independent of pp_set_local_plan.  Waits for the stream.  PP_ERR_STATE while a training
 * step is in flight. */
int pp_set_local_movers(pp_handle h, int32_t source, const pp_local_mover_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given for the source (zeros before the first). */
int pp_get_local_movers_config(pp_handle h, int32_t source, int32_t* on, pp_local_mover_config* cfg_out);
/* pp_local_plan_async with the stream's tracks as movers: does and refuses everything that call does, and first builds
 * the movers' table of every grid on the device from the track slots of stream b for grid b.  frame double [batch][4] =
 * (ox, oy, res, dt): the metres of the grid's cell [0, 0] corner in the tracks' frame, the metres of a cell and the
 * seconds of a rollout step.  Further refusals, all before anything is queued: PP_ERR_STATE when the source's movers are
 * off or pp_set_tracking has never been called on the handle; PP_ERR_ARG for frame NULL, a non-finite ox or oy, and a
 * res or dt that is not finite and > 0.  pp_local_plan_async itself never uses movers, whatever pp_set_local_movers
 * said. */
int pp_local_plan_movers_async(pp_handle h, int32_t source, const int32_t* poses, const int32_t* windows,
                               const double* frame, int32_t batch);
/* The movers of the source's last pp_local_plan_movers_async: movers int32 [batch][PP_LOCAL_MAX_MOVERS][6] (zeros behind
 * a grid's n_movers), info int32 [batch][PP_LOCAL_MOVER_INFO]; each may be NULL.  Waits and settles as pp_get_local_plan
 * does; where that queues the rollout again it runs on the table the call built, which is not rebuilt.  PP_ERR_STATE
 * also when the source's last run was a pp_local_plan_async. */
int pp_get_local_movers(pp_handle h, int32_t source, int32_t* movers, int32_t* info, int32_t batch);
/* pp_local_plan_grids with host-given movers: movers int32 [batch][PP_LOCAL_MAX_MOVERS][6] of which grid b uses the
 * first n_movers[b] (0 .. PP_LOCAL_MAX_MOVERS); every one of those is range-checked (PP_ERR_ARG naming the grid and the
 * mover).  horizon and mover_weight as pp_local_mover_config has them.  info int32 [batch][PP_LOCAL_MOVER_INFO] or
 * NULL (n_skipped is 0). */
int pp_local_plan_grids_movers(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height,
                               int32_t width, const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg,
                               const int32_t* trig, int32_t n_trig, const int32_t* poses, const int32_t* windows,
                               const int32_t* goal_state, int32_t horizon, int32_t mover_weight, const int32_t* movers,
                               const int32_t* n_movers, int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys,
                               int32_t* info);

/* ---- Footprint of the local planner: an oriented polygon instead of a point (local_planner.py states the rule).  A
 * footprint is a table of n probe points (fx, fy) in the robot's frame, int32 sub-cells, x forward along the heading
 * tick, y to the left; 1 <= n <= PP_LOCAL_MAX_PROBES, |fx|, |fy| <= PP_LOCAL_MAX_PROBE.  At a pose (X, Y, h) probe q lies
 * at (X + ((fx C[h] - fy S[h] + 8192) >> 14), Y + ((fx S[h] + fy C[h] + 8192) >> 14)), its cell is that >> 10; the cell is
 * OUTSIDE the grid, BLOCKED (g >= foot_lethal, or unknown while the navfn configuration's allow_unknown is 0) or free.
 * THE ROLLOUT: a sample still alive behind the centre's static test of a step looks at the probes in table order under
 * the heading after the step's turn; the first probe that is not free ends it, as OUTSIDE (reason 1) if its cell is
 * outside, as FOOTPRINT (reason 5) if blocked.  Probes never raise occ.  The movers' test, where they are on, follows.
 * cmd_state 5 (behind 4, 3, 2, before 1 and 0): a probe is not free at the start pose; no sample is rolled.  Once set, the
 * footprint is used by pp_local_plan_async and pp_local_plan_movers_async alike. ---- */
#define PP_LOCAL_MAX_PROBES 256         /* probes of a footprint at most */
#define PP_LOCAL_MAX_PROBE 32767        /* sub-cells: |fx|, |fy| at most */
#define PP_LOCAL_FOOT_INFO 4            /* int32 words per grid: n_probes, n_footprint, start_probe (-1: none), 0 */

typedef struct pp_local_footprint_config {
    int32_t foot_lethal;     /* 1 .. 100: a probe's cell with g >= foot_lethal is blocked */
    int32_t reserved[3];     /* 0 */
} pp_local_footprint_config;

/* n == 0 with probes == NULL (cfg may be NULL then): the source's footprint off (the default); its buffers are kept and
 * every launch and result is what it was.  Otherwise probes int32 [n][2] and the configuration are validated (PP_ERR_ARG
 * naming the probe or the field).  Independent of pp_set_local_plan and pp_set_local_movers.  Waits for the stream.  A
 * new table replaces the one a last run with a footprint read, so that run's results can no longer be fetched (its
 * getters answer PP_ERR_STATE until the next pp_local_plan_async).  PP_ERR_STATE while a training step is in flight. */
int pp_set_local_footprint(pp_handle h, int32_t source, const pp_local_footprint_config* cfg, const int32_t* probes, int32_t n);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first); probes_out (may be NULL):
 * int32 [PP_LOCAL_MAX_PROBES][2] of which the first *n_out (may be NULL) are the last table given. */
int pp_get_local_footprint_config(pp_handle h, int32_t source, int32_t* on, pp_local_footprint_config* cfg_out,
                                  int32_t* probes_out, int32_t* n_out);
/* The footprint words of the source's last pp_local_plan_async or pp_local_plan_movers_async: info int32
 * [batch][PP_LOCAL_FOOT_INFO] (may be NULL).  Waits and settles as pp_get_local_plan does.  PP_ERR_STATE also when that
 * run had no footprint. */
int pp_get_local_footprint(pp_handle h, int32_t source, int32_t* info, int32_t batch);
/* pp_local_plan_grids_movers with a footprint: probes int32 [n_probes][2] (1 .. PP_LOCAL_MAX_PROBES, every one
 * range-checked, PP_ERR_ARG naming the probe), one table for every grid, and foot_lethal as pp_local_footprint_config
 * has it.  movers may be NULL: no movers (n_movers, horizon, mover_weight and info are then not read).  foot_info int32
 * [batch][PP_LOCAL_FOOT_INFO] or NULL. */
int pp_local_plan_grids_footprint(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height,
                                  int32_t width, const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg,
                                  const int32_t* trig, int32_t n_trig, const int32_t* poses, const int32_t* windows,
                                  const int32_t* goal_state, int32_t horizon, int32_t mover_weight, const int32_t* movers,
                                  const int32_t* n_movers, const int32_t* probes, int32_t n_probes, int32_t foot_lethal,
                                  int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys, int32_t* info,
                                  int32_t* foot_info);

/* ---- scan match: the resident points of frame b under stream b's PRIOR sensor-to-fixed pose, matched against the
 * stream's occupancy map as it stands BEFORE the frame is fused into it (scan_match.py states the rule).  Opt-in, off by
 * default.  SCAN CELLS: per row, float64, dx = ((R00 x + R01 y) + R02 z), dy with row 1 (no translation); gx = floor(dx /
 * resolution) + width / 2, gy likewise; the row is used iff it passes pp_occupancy_update_async's tests and z >= z_min;
 * every distinct cell is one scan cell, its centre in sub-cells from the sensor ux = (gx - width / 2) * 1024 + 512.
 * SENSOR: sx = floor((t_x / resolution - ox) * 1024) with the window's current origin cell, on the host.  CANDIDATES:
 * c = (it * (2 ny + 1) + iy) * (2 nx + 1) + ix; dh = (it - nt) * theta_step, (C, S) = trig[dh & 4095]; rx = (C ux - S uy +
 * 8192) >> 14, ry = (S ux + C uy + 8192) >> 14 in int64; the cell cx = (sx + (ix - nx) * xy_step + rx) >> 10, cy likewise;
 * score[c] = the sum of the log-odds of those cells that lie in the window (unknown cells hold 0).  BEST: the least key
 * ((2^30 - score) << 32) | ((|it - nt| + |iy - ny| + |ix - nx|) << 16) | c. ---- */
#define PP_SCAN_MAX_CANDIDATES 65536 /* (2 nx + 1)(2 ny + 1)(2 nt + 1) at most */
#define PP_SCAN_RESULT 8             /* int32 words per stream: status, ix - nx, iy - ny, it - nt, best score, the prior's score,
                                        scan cells, rows ignored */
enum pp_scan_status {                /* bits of word 0 */
    PP_SCAN_NO_MAP = 1,              /* the stream has no map: nothing scored, every score 0 */
    PP_SCAN_OUTSIDE = 2,             /* the prior's cell lies outside the stream's window: likewise */
    PP_SCAN_FEW_CELLS = 4,           /* scan cells < min_cells */
    PP_SCAN_LOW_SCORE = 8,           /* best * 100 < min_mean * scan cells */
    PP_SCAN_EDGE = 16                /* the best lies on a face of a search axis whose half-width is > 0 */
};

typedef struct pp_scan_match_config {
    int32_t nx;            /* 0 .. 127: half-width of the search window in x, steps */
    int32_t ny;            /* 0 .. 127 */
    int32_t nt;            /* 0 .. 127: in heading; (2 nx + 1)(2 ny + 1)(2 nt + 1) <= PP_SCAN_MAX_CANDIDATES */
    int32_t xy_step;       /* 1 .. 4096 sub-cells (PP_LOCAL_SUB per cell) per translation step */
    int32_t theta_step;    /* 1 .. 512 ticks (PP_LOCAL_HEADINGS per revolution) per rotation step */
    int32_t min_cells;     /* 0 .. PP_OCC_MAX_CELLS */
    int32_t min_mean;      /* -100000 .. 100000: a best score below min_mean * scan cells / 100 is PP_SCAN_LOW_SCORE */
    int32_t reserved;      /* 0 */
} pp_scan_match_config;

/* cfg == NULL: the stage off (the default); the buffers are kept.  Otherwise the configuration is validated (PP_ERR_ARG
 * naming the field); trig as pp_set_local_plan takes it.  PP_ERR_STATE while the occupancy stage is not configured or a
 * training step is in flight.  Waits for the stream. */
int pp_set_scan_match(pp_handle h, const pp_scan_match_config* cfg, const int32_t* trig, int32_t n_trig);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_scan_match_config(pp_handle h, int32_t* on, pp_scan_match_config* cfg_out);
/* Matches the resident frames against the maps of streams 0 .. batch - 1 under the priors poses double [batch][3][4],
 * checked as pp_occupancy_update_async checks its poses.  Queued behind whatever the stream holds (an update queued before
 * it has been applied, one queued after it has not); returns at once.  Neither the maps nor their windows change. */
int pp_scan_match_async(pp_handle h, const double* poses, int32_t batch);
/* The last match: words int32 [batch][PP_SCAN_RESULT], scores int32 [batch][candidates] (may be NULL).  Waits for it. */
int pp_get_scan_match(pp_handle h, int32_t* words, int32_t* scores, int32_t batch);
/* Without a handle: logodds int16 and known uint8 (0 / 1) [batch][height][width] in host memory, the rows float32
 * [offsets[batch]][num_features] with offsets int32 [batch + 1], the priors, origin_cells int32 [batch][2] and has_map
 * int32 [batch] (0: PP_SCAN_NO_MAP); of occ_cfg resolution, z_min, z_max and max_range are read (its width and height must
 * be the grids').  words and scores as pp_get_scan_match gives them. */
int pp_scan_match_grids(int device, const int16_t* logodds, const uint8_t* known, int32_t batch, int32_t height, int32_t width,
                        const float* points, const int32_t* offsets, int32_t num_features, const double* poses,
                        const int32_t* origin_cells, const int32_t* has_map, const pp_occupancy_config* occ_cfg,
                        const pp_scan_match_config* cfg, const int32_t* trig, int32_t n_trig, int32_t* words, int32_t* scores);

/* ---- Frontier clusters behind either inflation, and of any int8 OccupancyGrid (frontier.py states the rule): where to
 * explore next.  FRONTIER CELL: 0 <= g <= free_max and at least one of the four edge neighbours inside the grid is -1.
 * CLUSTERS: the connected components of the frontier cells under `connectivity`; a cluster's label is the least linear
 * index y * width + x of its cells (labels uint32 [height][width], PP_FRONTIER_NONE elsewhere).  Per cluster n = cells,
 * sx = sum of x, sy = sum of y, the centroid cell cx = (2 sx + n) / (2 n) (cy likewise), the REPRESENTATIVE the member
 * with the least key (((x - cx)^2 + (y - cy)^2) << 20) | (y * width + x).  Clusters with n < min_size are dropped (counted
 * in `small`).  COST D: use_field 0, the squared cell distance from the grid's reference cell to the representative
 * (< 2^43); use_field 1, the uint32 potential of a navigation-function field at the representative, and a cluster whose D
 * is PP_NAVFN_UNREACHED is dropped (counted in `unreached`).  ORDER: ascending (D << 20) | label (rank 0) or
 * ((2^20 - n) << 20) | label (rank 1); the first max_frontiers are returned, eight int32 words each: x, y, cx, cy, n,
 * label, D low, D high.  Integers only, a unique answer whatever the schedule.  An opt-in stage: plain launches on the
 * handle's stream, not part of a captured pass. ---- */
#define PP_FRONTIER_MAX 64   /* frontiers returned per grid at most */
#define PP_FRONTIER_INFO 6   /* int32 per grid: frontier_cells, clusters, small, unreached, kept, returned */
#define PP_FRONTIER_NONE 0xFFFFFFFFu

typedef struct pp_frontier_config {
    int32_t free_max;       /* 0 .. 99: a known cell with g <= free_max is free */
    int32_t connectivity;   /* 4 / 8: of the clusters (the frontier test always looks at four neighbours) */
    int32_t min_size;       /* 1 .. PP_OCC_MAX_CELLS cells */
    int32_t max_frontiers;  /* 1 .. PP_FRONTIER_MAX */
    int32_t rank;           /* 0 nearest (least D), 1 largest (most cells) */
    int32_t use_field;      /* 0: D from the reference cell; 1: D from the source's navigation-function field */
    int32_t reserved[2];    /* 0 */
} pp_frontier_config;

/* cfg == NULL: the source's stage off (the default); its buffers are kept.  Otherwise the configuration is validated
 * (PP_ERR_ARG naming the field).  `source` is the inflation's.  Waits for the stream.  PP_ERR_STATE while a training step
 * is in flight. */
int pp_set_frontier(pp_handle h, int32_t source, const pp_frontier_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given for the source (zeros before the first). */
int pp_get_frontier_config(pp_handle h, int32_t source, int32_t* on, pp_frontier_config* cfg_out);
/* Queues the five launches on the grids of the source's last pp_inflate_async behind whatever the handle's stream holds:
 * refs int32 [batch][2], the reference cell (x, y) of every grid, each coordinate within +-2^20 (it need not lie in the
 * grid; read only while use_field is 0).  Reads the inflated grid in place and never writes it; a stream reset before that
 * inflation reads all unknown and has no frontier.  With use_field 1 the field of the source's last pp_navfn_async is read
 * in place, as pp_local_plan_async reads it.  Refused before anything is queued, PP_ERR_STATE: the stage or the source's
 * inflation is off, that inflation has not run, a training step is in flight, and under use_field no navigation function
 * has run or its field belongs to grids a later pp_inflate_async replaced; PP_ERR_ARG: a bad source, refs NULL, a batch
 * that is not the inflation run's, a reference cell out of range. */
int pp_frontier_async(pp_handle h, int32_t source, const int32_t* refs, int32_t batch);
/* The results of the source's last pp_frontier_async (waits for it; under use_field it first settles the field as
 * pp_get_navfn does and ranks again if that took a further round): words int32 [batch][PP_FRONTIER_MAX][8] (zeros behind
 * a grid's `returned` frontiers), info int32 [batch][PP_FRONTIER_INFO], labels uint32 [batch][height][width]; each may be
 * NULL.  PP_ERR_STATE when none has run (or, under use_field, a pp_navfn_async or pp_inflate_async came after it and the
 * ranking would have to run again), PP_ERR_ARG when batch is not that run's, PP_ERR_INTERNAL should a loop bound derived
 * from the cell count not suffice (they provably do). */
int pp_get_frontiers(pp_handle h, int32_t source, int32_t* words, int32_t* info, uint32_t* labels, int32_t batch);
/* Without a handle: grids int8 [batch][height][width] in host memory (height * width <= PP_OCC_MAX_CELLS, batch <= 65535),
 * pot uint32 of the same shape (required iff cfg->use_field, else it may be NULL), refs as above -> words, info, labels as
 * pp_get_frontiers gives them (each may be NULL). */
int pp_frontier_grids(int device, const int8_t* grids, const uint32_t* pot, int32_t batch, int32_t height, int32_t width,
                      const pp_frontier_config* cfg, const int32_t* refs, int32_t* words, int32_t* info, uint32_t* labels);

/* ---- Per-point object mask (object_mask.py states the rule): per resident row, one bit "this return belongs to an
 * object" -- the row's (x, y) lies in the BEV rectangle of a detection of the last pass or of a live track, exactly the
 * costmap's footprint test (u = (dx * c) - (dy * s), v = (dx * s) + (dy * c), |u| <= hx and |v| <= hy, float64; a NaN
 * fails) with the row in the place of a cell's centre.  The three readers of the rows use the bit while they are named in
 * `consumers`: the occupancy update takes a masked row in the hit band as a MASKED end (its cell still gets its one ray,
 * and is itself neither hit nor passed by that ray), the scan match ignores it, the costmap's point layer marks its cell
 * observed and counts nothing.  An opt-in stage: two plain launches on the handle's stream, nothing of it in a captured
 * pass; with the stage off every launch, buffer and result of every other stage is what it was.  A mask belongs to the
 * resident frames it was computed for: any change of them (upload, ingest, crop, sweeps) makes it stale, and a reader
 * named in `consumers` then answers PP_ERR_STATE until pp_object_mask_async has run again. ---- */
#define PP_OBJMASK_MAX_FOOTPRINTS 128 /* footprints of a frame: PP_TRACK_MAX slots, or the 128 detection rows the tracker admits */
#define PP_OBJMASK_INFO 4             /* int32 per frame: footprints, masked rows, rows, flagged */
enum { PP_OBJMASK_OCCUPANCY = 1, PP_OBJMASK_SCAN_MATCH = 2, PP_OBJMASK_COSTMAP = 4 };   /* bits of `consumers` */

typedef struct pp_object_mask_config {
    double min_score;      /* detections under it leave no footprint */
    double min_speed;      /* m/s, >= 0: a track masks only if (vx * vx + vy * vy) >= min_speed * min_speed */
    double pad;            /* metres added to a footprint's half extents, >= 0 */
    int32_t objects;       /* 1 the last pass's detections, 2 the streams' tracks */
    int32_t confirmed_only;/* tracks: only the confirmed ones */
    int32_t consumers;     /* PP_OBJMASK_* bits: the stages that read the mask */
    int32_t reserved;      /* 0 */
} pp_object_mask_config;

/* cfg == NULL: the stage off (the default); its buffers are kept.  Otherwise the configuration is validated (PP_ERR_ARG
 * naming the field); a configuration other than the last makes the last mask stale.  PP_ERR_STATE while a training step
 * is in flight. */
int pp_set_object_mask(pp_handle h, const pp_object_mask_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_object_mask_config(pp_handle h, int32_t* on, pp_object_mask_config* cfg_out);
/* Queues the stage on the resident frames behind whatever the handle's stream holds: the footprint tables (one workgroup
 * per frame), then a lane per resident row.  objects = tracks reads the streams' slots as the last step left them; poses
 * [batch][3][4] (may be NULL) carries a COPY of every slot from the stream's last posed tracking step into the frame of
 * the pose, exactly as that step's stage 0 would (skipped for a stream without such a step), and dt [batch] seconds
 * (may be NULL; each finite and >= 0) then predicts the copy, x + vx * dt.  The tracker's tables are not written.
 * Refused before anything is queued, the last mask staying as it is: PP_ERR_STATE when the stage is off, no frames are
 * resident, a training step is in flight, objects = detections and no pass has run on the resident frames, objects =
 * tracks before the first pp_set_tracking; PP_ERR_ARG for poses or dt under objects = detections, a batch that is not the
 * resident one, a dt that is not finite or negative, a pose that is not finite or not orthonormal; PP_ERR_UNSUPPORTED for
 * objects = detections with more than PP_OBJMASK_MAX_FOOTPRINTS result rows per frame. */
int pp_object_mask_async(pp_handle h, const double* poses /* [batch][3][4] or NULL */, const double* dt /* [batch] or NULL */,
                         int32_t batch);
/* The shape of the last run: *words_per_frame = ceil(max_n / 64) for the longest frame's bound max_n.  Waits for nothing. */
int pp_object_mask_shape(pp_handle h, int32_t* batch, int32_t* words_per_frame);
/* The mask of the last pp_object_mask_async (waits for the stream): words uint64 [batch][words_per_frame], bit (i & 63)
 * of word i >> 6 for row i of the frame, zero past the frame's rows; info int32 [batch][PP_OBJMASK_INFO].  Either may be
 * NULL.  PP_ERR_STATE when none has run or the frames it belongs to are gone, PP_ERR_ARG when batch is not that run's. */
int pp_get_object_mask(pp_handle h, uint64_t* words, int32_t* info, int32_t batch);
/* The rows of the last occupancy update that were masked ends, [batch].  Errors as pp_occupancy_info. */
int pp_occupancy_masked(pp_handle h, int32_t* masked, int32_t batch);
/* Without a handle: points [offsets[batch]][num_features >= 3] float32 and offsets [batch + 1] in host memory; footprints
 * [sum counts][5] float64 = x y w l yaw, the frames' back to back, counts [batch] each 0 .. PP_OBJMASK_MAX_FOOTPRINTS;
 * pad >= 0 -> words uint64 [batch][words_per_frame] (words_per_frame >= ceil(longest frame / 64)) and info as above
 * (either may be NULL).  A footprint with a non-finite field covers nothing. */
int pp_object_mask_points(int device, const float* points, const int32_t* offsets, int32_t num_features, int32_t batch,
                          const double* footprints, const int32_t* counts, double pad, uint64_t* words,
                          int32_t words_per_frame, int32_t* info);

/* ---- Ground plane per frame (ground.py states the rule and every operation's order): one plane z = a x + b y + c fitted
 * by RANSAC over K hypotheses, an optional integer least-squares refit over the winner's inliers, and per resident row a
 * class from its vertical residual r = z - (((a * x) + (b * y)) + c): GROUND |r| <= ground_dist, OBSTACLE ground_dist < r
 * <= overhead_max, OVERHEAD above, BELOW under -ground_dist, IGNORED for a NaN.  All float64 with + - * / and comparisons,
 * integer atomics only: two runs give the same bytes, and they are the restatement's.  The three readers of the rows use
 * the classes in place of their fixed z band while they are named in `consumers`: the occupancy update takes an in-window,
 * in-range row as a hit iff OBSTACLE and as a ground return iff GROUND, the scan match and the costmap's point layer count
 * a row iff OBSTACLE (an object-mask bit applies on top, as before).  An opt-in stage of plain launches on the handle's
 * stream, nothing of it in a captured pass; with the stage off every launch, buffer and result of every other stage is
 * what it was.  The classes belong to the resident frames they were computed for: any change of them (upload, ingest,
 * crop, sweeps) makes them stale, and a reader named in `consumers` then answers PP_ERR_STATE until pp_ground_async has
 * run again. ---- */
#define PP_GROUND_MAX_HYP 512         /* hypotheses of a frame at most */
#define PP_GROUND_INFO 12             /* int32 per frame: status (0 ok, 1 fallback), winner (-1: no valid hypothesis), inliers,
                                       * candidates, valid hypotheses, rows GROUND, OBSTACLE, OVERHEAD, BELOW, IGNORED, refit
                                       * (1: the refit's plane stands), rows */
#define PP_GROUND_SUMS 9              /* int64 per frame: N Sx Sy Sz Sxx Sxy Syy Sxz Syz of the refit (zeros when it did not run) */
enum { PP_GROUND_OCCUPANCY = 1, PP_GROUND_SCAN_MATCH = 2, PP_GROUND_COSTMAP = 4 };   /* bits of `consumers` */

typedef struct pp_ground_config {
    double max_range;      /* metres, > 0: a candidate row has (x * x + y * y) <= max_range * max_range */
    double cand_z_max;     /* ... and z <= cand_z_max */
    double max_slope;      /* >= 0: a plane stands only if (a * a + b * b) <= max_slope * max_slope */
    double h_min, h_max;   /* ... and h_min <= -c <= h_max */
    double inlier_dist;    /* >= 0 */
    double ground_dist;    /* >= 0 */
    double overhead_max;   /* >= ground_dist */
    double fallback_c;     /* the plane (0, 0, fallback_c) of a frame without a fit */
    uint64_t seed;         /* of the caller's generator of triples; kept and returned, never read here */
    int32_t hypotheses;    /* K, 1 .. PP_GROUND_MAX_HYP */
    int32_t min_inliers;   /* >= 1 */
    int32_t refine;        /* 0 / 1; 1 needs max_range <= 64, |cand_z_max| <= 64, max_slope * max_range + max(|h_min|, |h_max|)
                            * + inlier_dist <= 63 and rows per frame * 2^28 < 2^53: the refit's sums are then exact */
    int32_t consumers;     /* PP_GROUND_* bits: the stages that read the classes */
} pp_ground_config;

/* cfg == NULL: the stage off (the default); its buffers are kept.  Otherwise the configuration is validated (PP_ERR_ARG
 * naming the field); a configuration other than the last makes the last classes stale.  PP_ERR_STATE while a training
 * step is in flight. */
int pp_set_ground(pp_handle h, const pp_ground_config* cfg);
/* *on: 0 / 1; cfg_out (may be NULL): the last configuration given (zeros before the first). */
int pp_get_ground_config(pp_handle h, int32_t* on, pp_ground_config* cfg_out);
/* Queues the stage on the resident frames behind whatever the handle's stream holds.  triples uint32 [batch][K][3], K the
 * configured hypotheses: entry u names row (u * n) >> 32 of its frame of n rows.  Refused before anything is queued, the
 * last classes staying as they are: PP_ERR_STATE when the stage is off, no frames are resident or a training step is in
 * flight; PP_ERR_ARG for a NULL triples or a batch that is not the resident one. */
int pp_ground_async(pp_handle h, const uint32_t* triples, int32_t batch);
/* *readers: the PP_GROUND_* bits of the readers whose LAST queued run took the classes in the place of its z band
 * (pp_occupancy_update_async, pp_scan_match_async, pp_costmap_async), as pp_occupancy_masked tells of the object mask: a
 * bit is set when that call found the stage on, itself named and classes of the resident frames, and cleared when it ran
 * on its band.  Waits for nothing. */
int pp_ground_used(pp_handle h, int32_t* readers);
/* The shape of the last run: *words_per_frame = ceil(max_n / 64) for the longest frame's bound max_n.  Waits for nothing. */
int pp_ground_shape(pp_handle h, int32_t* batch, int32_t* words_per_frame);
/* The results of the last pp_ground_async (waits for the stream): planes float64 [batch][3] = a b c; info int32
 * [batch][PP_GROUND_INFO]; ground_words and obstacle_words uint64 [batch][words_per_frame], bit (i & 63) of word i >> 6
 * for row i of the frame, zero past the frame's rows; sums int64 [batch][PP_GROUND_SUMS]; counts int32 [batch][K], the
 * hypotheses' inliers (0 where invalid).  Each may be NULL.  PP_ERR_STATE when none has run or the frames it belongs to
 * are gone, PP_ERR_ARG when batch is not that run's. */
int pp_get_ground(pp_handle h, double* planes, int32_t* info, uint64_t* ground_words, uint64_t* obstacle_words, int64_t* sums,
                  int32_t* counts, int32_t batch);
/* Without a handle: points [offsets[batch]][num_features >= 3] float32 and offsets [batch + 1] in host memory, triples
 * [batch][cfg->hypotheses][3] -> the outputs of pp_get_ground (words_per_frame >= ceil(longest frame / 64); each may be
 * NULL).  `consumers` is not read. */
int pp_ground_points(int device, const float* points, const int32_t* offsets, int32_t num_features, int32_t batch,
                     const pp_ground_config* cfg, const uint32_t* triples, double* planes, int32_t* info, uint64_t* ground_words,
                     uint64_t* obstacle_words, int32_t words_per_frame, int64_t* sums, int32_t* counts);

/* Measurement helper: `reps` device-to-device copies of `bytes` on the handle's stream, timed with HIP events;
 * *gbytes_per_s = read + written bytes per second (what an HBM-bound kernel can reach on this part, next to the
 * spec constant the roofline fractions use). */
int pp_device_copy_bench(pp_handle h, int64_t bytes, int32_t reps, float* gbytes_per_s);

/* Device properties for reports: name (<=255 chars), CU count, bytes of HBM. */
int pp_device_info(pp_handle h, char* name, int32_t name_capacity, int32_t* compute_units, int64_t* hbm_bytes);
/* Bytes of HBM currently free on the handle's device (hipMemGetInfo): leak checks, sizing. */
int pp_device_mem_free(pp_handle h, int64_t* free_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_H */
