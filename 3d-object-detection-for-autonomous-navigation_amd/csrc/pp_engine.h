// Host side of the C-ABI (include/pp_hip.h), shared by its translation units: the handle, the error / allocation
// helpers and what one unit calls in another.  pp_api.hip: lifetime, weights, feeds, the inference pipeline;
// api_ingest.hip: PointCloud2, depth-image and camera-rig ingest; api_crop.hip: the frustum crop; api_train.hip: loss, training step, optimizer; api_dataprep.hip: targets,
// augmentation, GT sampling, object database; api_eval.hip: the AP evaluator (needs no handle); api_nms.hip: the detector's NMS rule and the standalone rotated NMS;
// api_project.hip: the detector's image boxes and the standalone projection; api_class_nms.hip: joint / per-class suppression;
// api_metrics.hip: the training metrics' counts; api_publish.hip: a trainer's weights into the detector, on the device;
// api_track.hip: the per-stream track tables behind the detector's post-process; api_sweeps.hip: the per-stream sweep rings
// in front of the pass; api_costmap.hip: the obstacle grid per frame behind it; api_occupancy.hip: the rolling occupancy
// map per stream; api_inflate.hip: obstacle inflation behind either grid; api_navfn.hip: the navigation function over the inflated grid; api_local_plan.hip: the local planner over that grid and its field; api_object_mask.hip: the per-point object mask in front of the three readers of the resident rows; api_ground.hip: the ground plane and the rows' classes in front of the same readers.  pp_ring.h: the pinned call ring and the stages' memory owner, which the handle's members are made of.
#pragma once

#include <cmath>
#include <algorithm>
#include <functional>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pp_common.h"
#include "pp_plan.h"
#include "pp_ring.h"
#include "train.h"

struct KTime { const char* name; int ev; };

// Ground-truth boxes on the device, the frames' boxes back to back (a kernel reads cls == NULL as class 1, valid == NULL as all valid)
struct GtSet {
    float* boxes = nullptr;      // [B * PP_MAX_GT_PER_FRAME][7]
    int* cls = nullptr;          // [B * PP_MAX_GT_PER_FRAME]
    uint8_t* valid = nullptr;
    int* cnt = nullptr;          // [B]
};

// The detector's post-process settings: what pp_set_nms_mode, pp_set_soft_nms, pp_set_class_nms and the on / off half of
// pp_set_projection write and the next run_post reads.  The soft parameters are kernel arguments of the PP_NMS_SOFT
// instantiation only.
struct PostRule {
    int nms_mode = PP_NMS_STANDUP;
    int soft_method = PP_SOFT_NMS_GAUSSIAN;
    float soft_sigma = 0.5f, soft_floor = 0.001f;
    int class_nms = PP_CLASS_NMS_JOINT;   // joint (one pass for all classes) or per class
    int proj = 0;                         // image boxes of the kept detections on / off
    int track = 0;                        // pp_set_tracking: k_track_step behind the post-process on / off
    bool operator==(const PostRule& o) const {
        return nms_mode == o.nms_mode && soft_method == o.soft_method && soft_sigma == o.soft_sigma &&
               soft_floor == o.soft_floor && class_nms == o.class_nms && proj == o.proj && track == o.track;
    }
};

// Everything a captured inference pass depends on, apart from what graph_invalidate drops the passes for (weights, cache
// budget): frames, point-count bucket, input buffer, zero-copy feed, voxelised at upload time, and the rule.
struct DetectKey {
    int batch = -1, bucket = -1, buf = -1, zc = 0, vox = 0;
    PostRule rule;
    bool operator==(const DetectKey& o) const {
        return batch == o.batch && bucket == o.bucket && buf == o.buf && zc == o.zc && vox == o.vox && rule == o.rule;
    }
};

// What the two halves of a training step were captured with; train_key (api_train.hip) is the only place to extend it.
struct TrainKey {
    int batch = -1, bucket = -1, zc = 0;
    const void *params = nullptr, *grads = nullptr, *state = nullptr;
    pp_loss_config loss = {};
    std::vector<unsigned char> frozen;     // TrainPlan::frozen
    bool metrics = false;                  // pp_set_train_metrics
    bool operator==(const TrainKey& o) const {
        return batch == o.batch && bucket == o.bucket && zc == o.zc && params == o.params && grads == o.grads &&
               state == o.state && memcmp(&loss, &o.loss, sizeof(loss)) == 0 && frozen == o.frozen && metrics == o.metrics;
    }
};

struct pp_engine {
    pp_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    PlanEnv plan_env;             // pp_create: the device's compute units and the process's switch table (pp_switches()).
                                  // Every choice of a kernel, a grid or a path that depends on either reads it from here
    std::string err;
    VoxGeom geom;
    int nx = 0, ny = 0, nz = 0, ncell = 0;
    int head_h = 0, head_w = 0, napl = 0, ncls = 1;
    bool use_dir = true, with_dist = false;
    int64_t A = 0;
    int C = 0, F = 0, T = 0, FA = 0, CC = 0;
    int B = 0, NMAX = 0;

    std::map<std::string, std::vector<float>> hw;
    std::map<std::string, std::vector<int64_t>> hshape;
    bool weights_ready = false, anchors_ready = false;
    std::vector<void*> allocs;    // device memory released by pp_destroy (dalloc)
    std::vector<void*> wallocs;   // weight buffers: released and re-made by every pp_finalize_weights

    // raw points and frame offsets are double-buffered: an upload fills the buffer the previous pass is NOT
    // reading (pp_upload_points_async on the copy stream, so the copy of batch k+1 runs beside the kernels of
    // batch k); d_points / d_offsets point at the buffer the next pp_detect_async consumes
    float* d_points_buf[2] = {nullptr, nullptr};
    int* d_offsets_buf[2] = {nullptr, nullptr};
    int in_buf = 0;                       // index of d_points / d_offsets (and of the voxeliser products: vox[])
    // The voxeliser's products exist twice as well (round 4): pp_upload_points_async voxelises batch k+1 right behind
    // its copy, on the copy stream, while batch k's PFN .. post-process read the other set -- the single-workgroup-
    // per-frame voxeliser (36 us on 64 of 256 CUs at B = 64) is then off the pass's chain of dependent launches.
    // The d_* members below always point at set in_buf (flip_input).
    struct VoxSet {
        float* points_sorted = nullptr;
        int *cellmap = nullptr, *pstart = nullptr, *pcell = nullptr, *npillars = nullptr, *nvalid = nullptr;
        unsigned long long* occbits = nullptr;
        bool occ_cleared = false;         // its k_cell_first cleared the occupancy bitmap (consumed by run_pfn)
    } vox[2];
    int cache_budget_mb = 256;            // run_backbone's frame sub-ranges (pp_set_cache_budget; 0 = off)
    bool vox_ahead = false;               // the resident batch was voxelised at upload time (pp_detect_async skips it)
    bool prevox_issued = false;           // a voxeliser launch is (or was) queued on the copy stream: a main-stream one waits for ev_up
    // ... and the other direction: a voxeliser launch is (or was) queued on the main stream (the zero-copy, synchronous and
    // device feeds, profiling, the stage call, training), so the next copy-stream one waits for ev_vox_main
    bool main_vox_pending = false;
    hipEvent_t ev_vox_main = nullptr;     // recorded on the main stream (outside any capture) by that wait
    int results_buf = 0;                  // set the last pp_detect_async read (pp_fetch_intermediates)
    hipStream_t copy_stream = nullptr;   // the device's shared upload stream (not owned by the handle)
    hipEvent_t ev_up = nullptr;           // recorded on the copy stream behind an asynchronous upload
    hipEvent_t ev_tgt = nullptr;          // ... behind the labels / boxes / draws of a training step (copies_done)
    bool up_pending = false;              // the next reader of the resident frames must wait for ev_up (wait_for_upload)
    hipEvent_t ev_read[2] = {nullptr, nullptr};   // recorded on the main stream behind the pass that read buffer i
    float* d_points = nullptr;
    float* d_points_sorted = nullptr;   // pillar-sorted copy left by k_sort_points (what the PFN streams)
    int* d_offsets = nullptr;
    float* spare_pts = nullptr;         // [B * NMAX][F] where the augmentation and the GT sampling write the new cloud
                                        // before it replaces the resident one (ensure_spare_pts: first use by either)
    int* d_cell = nullptr;
    int* d_first = nullptr;
    int* d_cellmap = nullptr;
    unsigned *d_keyA = nullptr, *d_idxA = nullptr, *d_keyB = nullptr, *d_idxB = nullptr;
    int* d_pstart = nullptr;
    int* d_pcell = nullptr;
    int* d_npillars = nullptr;
    int* d_nvalid = nullptr;
    float *d_pfn_w = nullptr, *d_pfn_b = nullptr;
    float* d_canvas = nullptr;
    float* d_act[2] = {nullptr, nullptr};
    float* d_concat = nullptr;
    float* d_head = nullptr;      // fused head map [B][H'*W'][PP_HEAD_COLS]
    float* d_cls = nullptr;       // compact class-logit plane [B][H'*W'][napl*ncls] (last fused-head deconv -> post-process)
    bool cls_plane_live = false;  // the last forward pass wrote d_cls (fused path with the uniform deconv kernels)
    bool fuse_heads = false;      // heads computed in the deconv epilogues (no concat buffer, no head launch)
    bool sparse_canvas = false;   // PFN writes occupied cells only; layer 0 consults the cell map (pp_finalize_weights)
    int* d_integ = nullptr;
    unsigned long long* d_occbits = nullptr;   // [B][ny][occ_words(nx)] occupancy bitmap of the sparse-canvas passes
    bool occbits_live = false;                 // this pass's PFN launch wrote it (the pillar-centric kernel)
    uint8_t* d_mask = nullptr;
    float* d_anchors = nullptr;
    int* d_cells = nullptr;
    float4* d_anchor_near = nullptr;   // [A] nearest standing / lying box of every anchor (target assignment)
    float* d_calib = nullptr;
    pp_detection* d_dets = nullptr;
    int* d_ndets = nullptr;
    pp_detection* h_dets = nullptr;  // pinned
    int* h_ndets = nullptr;          // pinned
    std::vector<LayerDesc> layers;
    std::vector<std::string> layer_tags;  // "<kernel symbol>:<layer>" for the profiler (for batch tag_batch)
    int tag_batch = -1;

    // compat scratch (grow-only)
    float* d_voxels = nullptr; size_t cap_voxels = 0;
    int* d_numpts = nullptr;   size_t cap_numpts = 0;
    int* d_coors = nullptr;    size_t cap_coors = 0;
    float* d_feat = nullptr;   size_t cap_feat = 0;

    // the resident batch: written by set_resident only
    int cur_batch = 0, cur_max_n = 0;
    int cur_total = 0;                    // points of the resident frames (host copy of the last offset)
    std::vector<int> h_cur_off;           // host copy of the resident frames' offsets [cur_batch + 1]
    bool off_host_exact = true;           // ... false: they are bounds, the sizes are device values (require_host_exact)
    int results_batch = 0;        // frames of the last enqueued pp_detect_async (0: no results to fetch)
    CallRing ring;                // the handle's call ring (pp_ring.h): the frame offsets and their riders
    RingArray<int> h_off;         // [B + 1] per slot
    hipEvent_t ev_main = nullptr; // orders an asynchronous rewrite of the frames (copy stream) behind the main stream
    hipEvent_t ev_in = nullptr;   // orders the engine's stream behind a producer stream (pp_upload_points_device)
    // zero-copy feed of small batches (pp_upload_points_async, batch <= ZC_MAX_BATCH): one page-locked descriptor
    // per input buffer, read by k_cell_first; no copy-engine transfer, no events
    PpFeed* h_feed[2] = {nullptr, nullptr};
    const PpFeed* d_feed[2] = {nullptr, nullptr};
    bool zc = false;              // the uploaded batch is fed that way

    // ---- the subsystems' buffers; all but `tgt` are allocated on first use, by the ensure_*() next to their user ----
    struct Loss {                          // pp_head_loss and the training step (api_train.hip: ensure_loss_buffers)
        int* labels = nullptr;             // [B][A]
        float* regt = nullptr;             // [B][A][7]
        int* npos = nullptr;
        double* partials = nullptr;
        float* out = nullptr;              // [8]
        float* head_grad = nullptr;
    } loss;
    struct Tgt {                           // target assignment from boxes (pp_assign_targets / pp_train_step_gt*)
        GtSet gt;                          // the boxes the assignment reads (no `valid`): uploaded, or the augmentation's output
        unsigned* top = nullptr;           // per box: its best overlap (float bits), reset before every assignment
        uint8_t* mask = nullptr;           // [B][A] the assignment's anchor mask (d_mask stays the inference pass's)
        int* index = nullptr;              // [B][A] optional outputs of pp_assign_targets, allocated on first use
        float* overlap = nullptr;
    } tgt;
    struct Aug {                           // training-time augmentation (pp_augment / pp_train_step_aug*)
        bool ready = false;
        GtSet in;                          // the boxes as given
        double* draws = nullptr;           // [B * PP_MAX_GT_PER_FRAME][PP_AUG_MAX_TRY][5]
        pp_aug_frame* frames = nullptr;
        AugBox* rec = nullptr;
        float* box_tmp = nullptr;
        uint8_t* keep = nullptr;
        int* sel = nullptr;                // [B * PP_MAX_GT_PER_FRAME] the selected try per input box (pp_augment_selected)
        int* draw_off = nullptr;           // [B] first draw row of each frame (the sampled step: rows are allotted per frame)
        std::vector<int> h_draw_off;       // its host side
        double* cs = nullptr;              // [B][2]
        int64_t total = 0;                 // input boxes of the last augmentation
    } aug;
    struct Db {                            // the loaded object database (pp_gtdb_load): replaced as a whole, not in `allocs`
        float* pts = nullptr;
        int* off = nullptr;
        double* box = nullptr;
        int* cls = nullptr;
        std::vector<int> h_npts;           // points per object (the host-side bound on the pasted cloud)
        int64_t n = -1;                    // objects loaded; -1: no database
    } db;
    struct Gts {                           // GT-database sampling (pp_gt_sample / pp_train_step_sample*)
        bool ready = false;
        GtSet in, out;                     // the boxes as given; the frame's boxes, then the accepted objects'
        pp_gts_cand* cands = nullptr;      // [B][PP_GTS_MAX_CAND]
        int* cand_counts = nullptr;        // [B][PP_GTS_MAX_ROUNDS]
        GtsPlane* planes = nullptr;
        int *status = nullptr, *counts = nullptr, *round = nullptr;
        int *acc_n = nullptr, *acc_slot = nullptr, *acc_pstart = nullptr, *box_off = nullptr;
        int* offsets = nullptr;            // [B + 1] the frames' offsets after pasting
        int batch = 0;                     // frames of the last pp_gt_sample (pp_gt_sample_info)
    } gts;
    struct Gdb {                           // building the object database from the resident frames (pp_gtdb_build / _count)
        bool ready = false;
        double* boxes = nullptr;           // [B * PP_MAX_GT_PER_FRAME][7]
        int *cnt = nullptr, *boxoff = nullptr;   // [B], [B + 1]
        GtsPlane* planes = nullptr;        // [B * PP_MAX_GT_PER_FRAME]
        int* chunks = nullptr;             // [B][ceil(NMAX / PP_GDB_CHUNK)][PP_MAX_GT_PER_FRAME]
        int* totals = nullptr;             // [B * PP_MAX_GT_PER_FRAME]
        long long* off = nullptr;          // [B * PP_MAX_GT_PER_FRAME + 1]
        float* out = nullptr;  size_t cap_out = 0;   // the cut-out points grow to the largest build seen (dgrow)
    } gdb;
    struct Ing {                           // live-camera ingest (pp_ingest_pointcloud2*, pp_ingest_depth*, pp_ingest_rig_*); raw / chunks grow (dgrow)
        union Slot { IngFrame pc2; DepthFrame depth; };    // room for a frame of either feed (a call packs its own type tightly)
        uint8_t* raw = nullptr;  size_t cap_raw = 0;       // the messages' (images') bytes
        int* chunks = nullptr;   size_t cap_chunks = 0;    // [2][batch * stride]: chunk counts, chunk bases
        Slot* frames = nullptr;            // [B]
        RingArray<Slot> h_ring;            // [B] per slot of the handle's ring
        int *finite = nullptr, *kept = nullptr;            // [B] finite records (valid pixels), points kept
        IngFeat* feats = nullptr;          // [B][F - 3] feature columns of a pp_ingest_pointcloud2_fields* call
        RingArray<IngFeat> h_feats;        // [B][F - 3] per slot
        int batch = 0;                     // frames of the last ingest (pp_ingest_info)
        // a rig call (pp_ingest_rig_*) has one record per SOURCE: tables of their own, sized by sources_cap =
        // PP_RIG_MAX_SOURCES * B on first use (api_ingest.hip: ensure_rig); finite / kept above then hold the frames' sums
        struct Rig {
            Slot* frames = nullptr;        // [sources_cap]
            RigSource* src = nullptr;      // [sources_cap]
            RingArray<Slot> h_frames;      // [sources_cap] per slot of the handle's ring
            RingArray<RigSource> h_src;    // [sources_cap] per slot
            IngFeat* feats = nullptr;      // [sources_cap][F - 3], as Ing::feats
            RingArray<IngFeat> h_feats;    // [sources_cap][F - 3] per slot
            int *finite = nullptr, *kept = nullptr, *out_base = nullptr;   // [sources_cap]
            int sources_cap = 0;
            int sources = 0;               // sources of the last ingest when it was a rig call, else 0 (pp_ingest_rig_info)
        } rig;
    } ing;
    struct Crop {                          // frustum crop of the resident frames (pp_frustum_crop*; api_crop.hip: ensure_crop)
        double* planes = nullptr;          // [B][6][4]
        RingArray<double> h_ring;          // [B][6][4] per slot of the handle's ring
        int* chunks = nullptr;             // [2][B * crop_chunks(NMAX)]: chunk counts, chunk bases
        int* kept = nullptr;               // [B]
        int batch = 0;                     // frames of the last crop (pp_frustum_crop_info)
    } crop;
    struct Sweeps {                        // multi-sweep accumulation (pp_set_sweeps, pp_sweeps_accumulate*; api_sweeps.hip)
        bool on = false;                   // pp_set_sweeps gave a configuration and has not taken it back
        pp_sweep_config cfg = {};          // the configuration in force, capacity filled in (history 0: no ring yet)
        StageMem mem;                      // owns the streams' rings and tables below (SweepParams): not in `allocs`
        float* ring = nullptr;
        int *slot_cnt = nullptr, *slot_valid = nullptr, *head = nullptr;
        double *slot_pose = nullptr, *slot_stamp = nullptr;
        SweepXf* xf = nullptr;
        SweepChunk *segs = nullptr, *chunks = nullptr;
        int *seg_chunk0 = nullptr, *frame_chunks = nullptr, *nchunks = nullptr;
        int chunk_cap = 0;
        int* info = nullptr;               // [4][B]: count, used, truncated, push_truncated
        double* d_call = nullptr;          // [B][13] the call's poses and stamps
        RingArray<double> h_ring;          // [B][13] per slot of the handle's ring
        std::vector<double> last_stamp;    // [B] per stream: the last stamp accepted (NaN: none)
        std::vector<int> stored;           // [B] per stream: sweeps its ring holds at most (the host's bound)
        int batch = 0;                     // frames of the last call (pp_sweeps_info)
    } swp;

    struct Metrics {                       // training metrics (pp_head_metrics / pp_set_train_metrics; api_metrics.hip: ensure_metrics)
        bool on = false;                   // pp_set_train_metrics: the following steps count
        int* partials = nullptr;           // [B * metrics_blocks(H' * W')][PP_METRICS_COUNTS]
        long long* counts = nullptr;       // [PP_METRICS_COUNTS]
        long long* h_counts = nullptr;     // pinned twin: a step's counts travel behind its losses
        float* logits = nullptr;           // [B][A][ncls] the cls_preds handed to pp_head_metrics (allocated on first use)
        bool step_counted = false;         // the last launched step ran with the switch on (pp_get_train_metrics)
        MetricsParams step;                // what that step's launch reads (TrainCtx::metrics)
    } metrics;

    // training step (train.hip): shapes, plan (the flat layout among it) and device buffers, set up by the first
    // pp_train_* call
    struct TrainState {
        TrainShape shape;
        TrainPlan plan;
        TrainCtx cx;
        bool buffers = false;
        // the ~250 launches of a step replay as one hipGraph while nothing they depend on changes; ONE GRAPH PER INPUT
        // BUFFER: every upload flips the handle's input buffer (the kernels' point / offset pointers), so a single
        // graph would be re-captured on every optimizer step
        struct Graph {
            hipGraphExec_t exec = nullptr;     // voxelise + forward
            hipGraphExec_t exec_bwd = nullptr; // loss + backward (launched behind the target upload's event)
            TrainKey key;
        } graph[2];
        int last_batch = 0;    // frames of the last step (pp_train_fetch_decisions)
        int graph_state = 0;   // -1: capture failed once, plain launches from then on
        int n_captures = 0, n_replays = 0;   // pp_train_graph_stats
    };
    TrainState* train = nullptr;
    float* h_train_losses = nullptr;      // page-locked [8]: the losses of a step launched by pp_train_step_async
    bool train_pending = false;           // ... which pp_train_step_wait has not collected yet
    bool mask_in_pfn = false;      // the last run_pfn also computed the anchor mask (few frames)
    int f32_fallback_layers = 0;   // layers whose folded weights do not fit float16 pieces (pp_finalize_weights)
    bool force_f32 = false;        // pp_set_gemm_precision(PP_PREC_F32): no layer gets split weights
    // pp_publish_train_weights (api_publish.hip): the weight arrays written on the device from a trainer's buffers.  They
    // live in `wallocs` like a host-loaded set, so pp_finalize_weights replaces them (live = false) and the next
    // publish allocates again.
    struct Publish {
        bool live = false;                      // the handle's weights are the published arrays
        std::vector<float*> wt16, head_wt16;    // per layer: the float16 array of an eligible layer (NULL: not eligible),
                                                // allocated once whether or not the layer runs on it (LayerDesc::d_wt16)
        std::vector<int> h_flags;               // [2 * layers] range flags of the last publish: d_wt, d_head_wt
        int* d_flags = nullptr;
        PubTask *d_fold = nullptr, *d_split = nullptr;
        int n_fold = 0, n_split = 0, fold_blocks = 0, split_blocks = 0;
        PubHead head;
        int64_t publishes = 0, reallocations = 0, graph_invalidations = 0;
    } pub;
    PostRule rule;                        // the next pass's post-process settings
    // The result buffers (d_dets, h_dets, the projection's boxes) hold ncls * nms_post_max_size rows per frame; a pass uses
    // the row stride of the class mode it ran in (det_rows)
    int results_rows = 0;                 // row stride of the last pass whose results can be fetched (pp_get_detections, pp_get_bboxes)
    pp_detection* d_cls_dets = nullptr;   // [B][ncls][nms_post_max_size]: the classes' segments, before k_gather_classes
    int* d_cls_cnt = nullptr;             // [B][ncls]
    // pp_set_projection: image boxes of the kept detections (allocated on first use; on / off is rule.proj)
    struct Projection {
        int batch = 0;                 // frames the matrices were given for
        std::vector<double> h_p2;      // what d_p2 holds (an unchanged set is not uploaded again)
        double* d_p2 = nullptr;        // [B][16]
        double* d_bbox = nullptr;      // [B * ncls * nms_post_max_size][4] (row stride of a pass: det_rows)
        double* d_cls_bbox = nullptr;  // [B][ncls][nms_post_max_size][4]: the per-class segments
        double* h_bbox = nullptr;      // pinned twin: the fused path's kernel stores into it, pp_predict copies into it
        int results = 0;               // frames of the last pass that projected (pp_get_bboxes; 0: none, or projection off)
    } proj;

    // pp_set_tracking: one track table per stream (frame b of a pass is stream b), advanced by k_track_step behind the
    // post-process (on / off is rule.track).  Allocated on first use (api_track.hip: ensure_track).
    struct Track {
        bool ready = false;
        bool configured = false;       // pp_set_tracking has given a configuration
        pp_track_config cfg = {};      // what d_cfg holds
        pp_track_config* d_cfg = nullptr;
        TrkSlot* state = nullptr;      // [B][PP_TRACK_MAX]
        int *next_id = nullptr, *overflow = nullptr;   // [B]
        double* d_dt = nullptr;        // [B] seconds of the next step per stream (0: the configuration's period)
        CallRing dt_ring;              // pp_set_track_dt's values, consumed on the main stream
        RingArray<double> h_dt;        // [B] per slot
        pp_track* h_out = nullptr;     // pinned [B][PP_TRACK_MAX]: the kernel stores the live rows straight into it (nothing on
        int *h_nout = nullptr, *h_overflow = nullptr;   // the device reads them: no device copy, no copy node behind the pass)
        pp_detection* in_dets = nullptr;   // [B][PP_TRACK_MASK_ROWS] pp_track_update's rows (d_dets stays a pass's)
        int* in_n = nullptr;               // [B]
        // pp_set_track_pose: the ego pose of the next step per stream, and of the last posed step that ran
        TrkPose *d_pose_q = nullptr, *d_pose_prev = nullptr;   // [B] each
        CallRing pose_ring;                // the poses travel as the dt values do, on a ring of their own
        RingArray<TrkPose> h_pose;         // [B] per slot
        pp_track* h_out_fixed = nullptr;   // pinned [B][PP_TRACK_MAX]: the step's rows in the fixed frame (pp_get_tracks_fixed)
        int* h_nout_fixed = nullptr;       // pinned [B]; -1: the stream's step had no pose
        int results = 0;              // streams of the last tracked pass or pp_track_update (pp_get_tracks; 0: none)
        bool from_pass = false;        // ... it was a pass: pp_get_tracks consults its frames' numeric flags
    } trk;

    // pp_set_costmap: one obstacle grid per frame from the resident points and the pass's detections or the streams'
    // tracks (api_costmap.hip).  A stage behind the pass: plain launches, nothing of it in PostRule or a captured pass.
    struct Costmap {
        bool on = false;                   // pp_set_costmap gave a configuration and has not taken it back
        pp_costmap_config cfg = {};        // the last configuration given
        int pitch = 0;                     // cells of a row in the buffers below: width rounded up to 4
        size_t cells = 0;                  // height * pitch, what the buffers were allocated for (0: none yet)
        int hdr = 0;                       // int32 words in front of the count words: the frames' in-grid tallies
        StageMem mem;                      // owns the buffers below, made by pp_set_costmap: not in `allocs`
        unsigned* words = nullptr;         // [hdr + B * cells]: cleared before every run
        int8_t* grid = nullptr;            // [B * cells]
        int* tap = nullptr;                // [B * cells]
        CmFootprint* table = nullptr;      // [B][table_rows]
        int table_rows = 0;
        int* info = nullptr;               // [2][B]: footprints, flagged
        int batch = 0;                     // frames of the last run (pp_get_costmaps; 0: none)
        int run_pitch = 0, run_w = 0, run_h = 0, run_objects = 0;   // ... and its grid
        double run_res = 0.0;              // ... and the resolution its cells were counted at (pp_inflate_async compares its table's)
    } cmap;

    // pp_set_occupancy: one rolling log-odds window per stream in the fixed frame, updated from the resident frames under
    // a pose per stream (api_occupancy.hip).  Plain launches on the handle's stream, nothing of it in a captured pass.
    struct Occupancy {
        bool on = false;                   // pp_set_occupancy gave a configuration and has not taken it back
        pp_occupancy_config cfg = {};      // the last configuration given
        int pitch = 0;                     // cells of a row in the buffers below: width rounded up to 4
        size_t cells = 0;                  // height * pitch, what the buffers were allocated for (0: none yet)
        int list_cap = 0;
        StageMem mem;                      // owns the window-shaped buffers, made by pp_set_occupancy: not in `allocs`
        unsigned* marks = nullptr;         // [B * cells]
        unsigned char* passed = nullptr;   // [B * cells]
        int* list = nullptr;               // [B][list_cap]
        int16_t* logodds[2] = {nullptr, nullptr};   // [B * cells] each
        int8_t* grid[2] = {nullptr, nullptr};       // [B * cells] each
        int* info = nullptr;               // [B][PP_OCC_INFO]; this and the next two whatever the window's shape (`allocs`)
        int8_t* table = nullptr;           // [2001]
        OccCall* d_call = nullptr;         // [B]
        CallRing ring;                     // the calls' records, consumed on the main stream
        RingArray<OccCall> h_call;         // [B] per slot
        // per stream, [B]: what the host knows of the map (the window's origin is the host's own arithmetic)
        std::vector<char> has;             // a window exists
        std::vector<int> ox, oy;           // its origin cell
        std::vector<int> cur;              // the state copy that holds it
        std::vector<int> cleared;          // pp_occupancy_info: of the stream's last update
        int batch = 0;                     // streams of the last update (pp_get_occupancy; 0: none)
    } occ;

    // pp_set_inflation: the costmap's or the occupancy maps' grids with every obstacle grown by the robot's radius
    // (api_inflate.hip).  One plain launch on the handle's stream; it reads the source's grid and writes `out` / `dist2`.
    struct Inflation {
        bool on = false;                   // pp_set_inflation gave a configuration and has not taken it back
        pp_inflation_config cfg = {};      // the last configuration given
        int R = 0;                         // ceil(inflation_radius / resolution)
        int8_t* table = nullptr;           // [PP_INFLATE_MAX_RADIUS^2 + 1]; this and `counts` live as long as the handle (`allocs`)
        int* counts = nullptr;             // [B][2]: lethal, raised
        StageMem mem;                      // owns out and dist2, made by pp_inflate_async for the source's shape: not in `allocs`
        int8_t* out = nullptr;             // [B * cells]
        uint16_t* dist2 = nullptr;         // [B * cells]
        size_t cells = 0;                  // height * pitch the two were allocated for (0: none yet)
        int batch = 0;                     // grids of the last run (pp_get_inflated; 0: none)
        int run_pitch = 0, run_w = 0, run_h = 0, run_R = 0;   // ... and their shape
        std::vector<char> known;           // [batch] of that run; 0: the stream had been reset, its grid reads all unknown
        unsigned long long run_id = 0;     // counts the pp_inflate_async calls of the source: `out` is reused, its contents are not
    } infl[2];                             // by source: PP_INFLATE_COSTMAP, PP_INFLATE_OCCUPANCY

    // pp_set_navfn: the cost-to-go field from a goal cell and the path from a start cell over infl[source].out, which it
    // reads in place and never writes (api_navfn.hip).  Plain launches on the handle's stream: init, relaxation rounds,
    // finish; the getters queue the rounds still missing.  Nothing of it in PostRule, DetectKey or a captured pass.
    struct Navfn {
        bool on = false;                   // pp_set_navfn gave a configuration and has not taken it back
        pp_navfn_config cfg = {};          // the last configuration given
        int* state = nullptr;              // [NAV_STATE][B]; this and d_call live as long as the handle (`allocs`)
        NavCall* d_call = nullptr;         // [B]
        CallRing ring;                     // the calls' goals and starts, consumed on the main stream
        RingArray<NavCall> h_call;         // [B] per slot
        StageMem mem;                      // owns the four buffers below, made by pp_navfn_async for the source's shape: not in `allocs`
        uint16_t* cost = nullptr;          // [B * cells]
        unsigned* pot[2] = {nullptr, nullptr};     // [B * cells] each
        int* paths = nullptr;              // [B][path_cap][2]
        size_t cells = 0;                  // height * pitch they were allocated for (0: none yet)
        int path_cap = 0;
        int batch = 0;                     // grids of the last run (pp_get_navfn; 0: none)
        NavParams run = {};                // ... what it was launched with
        int rounds = 0;                    // relaxation rounds queued behind its init so far
        unsigned long long run_id = 0;     // counts the pp_navfn_async calls of the source (pp_get_local_plan)
        unsigned long long infl_run = 0;   // infl[source].run_id of the grids the last run read (check_navfn_run)
        bool settled = false;              // a getter has seen every grid's field stand, and `host` holds the state words
        std::vector<int> host;             // [NAV_STATE][B]
    } navfn[2];                            // by source, as infl

    // pp_set_local_plan: the (v, w) command from a window of rollouts over infl[source].out and navfn[source]'s field, both
    // read in place and never written (api_local_plan.hip).  Plain launches on the handle's stream: rollout, finish; the
    // getter settles the field first and queues both again if that took a further round.
    struct LocalPlan {
        bool on = false;                   // pp_set_local_plan gave a configuration and has not taken it back
        pp_local_plan_config cfg = {};     // the last configuration given
        unsigned* trig = nullptr;          // [PP_LOCAL_HEADINGS] packed; this and the next four live as long as the handle (`allocs`)
        int* state = nullptr;              // [LOC_STATE][B]
        unsigned long long* partial = nullptr;     // [B][LOC_MAX_CHUNKS]
        unsigned long long* score = nullptr;       // [B]
        LocalCall* d_call = nullptr;       // [B]
        CallRing ring;                     // the calls' poses and windows, consumed on the main stream
        RingArray<LocalCall> h_call;       // [B] per slot
        StageMem mem;                      // owns keys and traj, made by pp_local_plan_async for the configuration's shape: not in `allocs`
        unsigned long long* keys = nullptr;        // [B][samples_cap]
        int* traj = nullptr;               // [B][steps_cap + 1][3]
        int samples_cap = 0, steps_cap = 0;
        int batch = 0;                     // grids of the last run (pp_get_local_plan; 0: none)
        LocalParams run = {};              // ... what it was launched with
        unsigned long long nav_run = 0;    // navfn[source].run_id it was queued behind
        int nav_rounds = 0;                // navfn[source].rounds its last launches were queued behind
        // pp_set_local_movers: the stream's tracks as movers of pp_local_plan_movers_async (k_local_movers in front of
        // the rollout); `run.movers` says whether the last run had them
        bool movers_on = false;            // pp_set_local_movers gave a configuration and has not taken it back
        pp_local_mover_config mcfg = {};   // the last configuration given
        int* movers = nullptr;             // [B][PP_LOCAL_MAX_MOVERS][6]; this and the next two live as long as the handle (`allocs`)
        int* mover_info = nullptr;         // [PP_LOCAL_MOVER_INFO][B]
        LocalFrame* d_frame = nullptr;     // [B]
        RingArray<LocalFrame> h_frame;     // [B] per slot, a rider of `ring`
        // pp_set_local_footprint: the robot as a table of probes, used by both async calls while it is on; `run.probes`
        // says whether the last run had it
        bool foot_on = false;              // pp_set_local_footprint gave a table and has not taken it back
        pp_local_footprint_config fcfg = {};       // the last configuration given
        std::vector<int32_t> probes;       // [n][2], the last table given (pp_get_local_footprint_config)
        unsigned* d_probes = nullptr;      // [PP_LOCAL_MAX_PROBES] packed; this and the next live as long as the handle (`allocs`)
        int* foot_info = nullptr;          // [PP_LOCAL_FOOT_INFO][B]
    } local[2];                           // by source, as infl

    // pp_set_scan_match: the resident frames under a prior pose per stream, matched against occ.logodds, which it reads in
    // place and never writes (api_scan_match.hip).  Plain launches on the handle's stream: cells, scores, finish.  Nothing
    // of it in PostRule, DetectKey or a captured pass, and api_occupancy.hip knows nothing of it: the stage compares the
    // occupancy window's shape with its own buffers' at every call.
    struct ScanMatch {
        bool on = false;                   // pp_set_scan_match gave a configuration and has not taken it back
        pp_scan_match_config cfg = {};     // the last configuration given
        unsigned* trig = nullptr;          // [PP_LOCAL_HEADINGS] packed; this and the next two live as long as the handle (`allocs`)
        int* words = nullptr;              // [B][PP_SCAN_RESULT]
        ScanCall* d_call = nullptr;        // [B]
        CallRing ring;                     // the calls' priors, consumed on the main stream
        RingArray<ScanCall> h_call;        // [B] per slot
        StageMem mem_cfg;                  // owns scores and partial, made by pp_set_scan_match for the configuration: not in `allocs`
        int* scores = nullptr;             // [B][cand_cap]
        unsigned long long* partial = nullptr;     // [B][part_cap]
        int cand_cap = 0, part_cap = 0;
        StageMem mem_win;                  // owns clear and list, made by pp_scan_match_async for the occupancy window's shape: not in `allocs`
        unsigned* clear = nullptr;         // [B][SCAN_INFO] the tallies, then [B][mark_words] the marks: one clear per call
        int2* list = nullptr;              // [B][list_cap]
        int win_w = 0, win_h = 0, list_cap = 0, mark_words = 0;     // what the two were made for (0: none yet)
        int batch = 0;                     // streams of the last match (pp_get_scan_match; 0: none)
        int run_cands = 0;                 // ... and its candidates per stream
    } scan;

    // pp_set_frontier: the clusters of the frontier cells of infl[source].out, ranked as exploration goals; with use_field
    // the ranking reads navfn[source]'s field.  Both are read in place and never written (api_frontier.hip).  Plain
    // launches on the handle's stream: mark, label, stats, rep, select; the getter settles the field first and queues
    // select again if that took a further round.  Nothing of it in PostRule, DetectKey or a captured pass.
    struct Frontier {
        bool on = false;                   // pp_set_frontier gave a configuration and has not taken it back
        pp_frontier_config cfg = {};       // the last configuration given
        int* info = nullptr;               // [B][FR_INFO_WORDS]; this and the next two live as long as the handle (`allocs`)
        int* words = nullptr;              // [B][PP_FRONTIER_MAX][8]
        FrontierCall* d_call = nullptr;    // [B]
        CallRing ring;                     // the calls' reference cells, consumed on the main stream
        RingArray<FrontierCall> h_call;    // [B] per slot
        StageMem mem;                      // owns the five buffers below, made by pp_frontier_async for the inflation run's shape: not in `allocs`
        unsigned* labels = nullptr;        // [B][h * w]
        unsigned* count = nullptr;         // [B][h * w]
        unsigned* roots = nullptr;         // [B][h * w]
        unsigned long long* sums = nullptr;        // [B][h * w][2]
        unsigned long long* rep = nullptr;         // [B][h * w]
        int w = 0, h = 0;                  // the shape they were made for (0: none yet)
        int batch = 0;                     // grids of the last run (pp_get_frontiers; 0: none)
        FrontierParams run = {};           // ... what it was launched with
        unsigned long long nav_run = 0;    // navfn[source].run_id it was queued behind (use_field)
        int nav_rounds = 0;                // navfn[source].rounds its last select was queued behind
    } frontier[2];                         // by source, as infl

    // pp_set_object_mask: a bit per resident row, "this return lies in the BEV rectangle of a detection / a track"
    // (api_object_mask.hip).  Two plain launches on the handle's stream; the three readers of the rows (occupancy update,
    // scan match, costmap points) take its words through object_mask_for while they are named in cfg.consumers.  Nothing
    // of it in PostRule, DetectKey or a captured pass.
    struct ObjMask {
        bool on = false;                   // pp_set_object_mask gave a configuration and has not taken it back
        pp_object_mask_config cfg = {};    // the last configuration given
        OmFootprint* table = nullptr;      // [B][PP_OBJMASK_MAX_FOOTPRINTS]; this and the next three live as long as the handle (`allocs`)
        int* info = nullptr;               // [B][PP_OBJMASK_INFO]
        unsigned long long* words = nullptr;       // [B][stride]
        OmCall* d_call = nullptr;          // [B]
        int stride = 0;                    // 4 * ceil(NMAX / 256): a word per wave of k_objmask_rows' largest grid
        CallRing ring;                     // the calls' poses and dt values, consumed on the main stream
        RingArray<OmCall> h_call;          // [B] per slot
        int batch = 0;                     // frames of the last run (pp_get_object_mask; 0: none, or made stale by a new configuration)
        int run_words = 0;                 // ... ceil(max_n / 64) of it
        unsigned long long gen = 0;        // ... and the resident_gen it belongs to
    } omask;

    // pp_set_ground: one plane per resident frame and two bits per row, GROUND and OBSTACLE (api_ground.hip).  Plain
    // launches on the handle's stream; the three readers of the rows take its words through ground_for while they are
    // named in cfg.consumers.  Nothing of it in PostRule, DetectKey or a captured pass.
    struct Ground {
        bool on = false;                   // pp_set_ground gave a configuration and has not taken it back
        pp_ground_config cfg = {};         // the last configuration given
        GrHyp* hyp = nullptr;              // [B][PP_GROUND_MAX_HYP]; this and the next eight live as long as the handle (`allocs`)
        GrHyp* chyp = nullptr;             // [B][PP_GROUND_MAX_HYP]: the valid ones, compacted
        int* counts = nullptr;             // [B][PP_GROUND_MAX_HYP]
        long long* sums = nullptr;         // [B][PP_GROUND_SUMS]
        double* plane = nullptr;           // [B][3]
        int* info = nullptr;               // [B][PP_GROUND_INFO]
        unsigned long long* gnd = nullptr; // [B][stride]
        unsigned long long* obs = nullptr; // [B][stride]
        unsigned* d_tri = nullptr;         // [B][PP_GROUND_MAX_HYP][3]
        int stride = 0;                    // 4 * ceil(NMAX / 256): a word per wave of k_ground_class' largest grid
        CallRing ring;                     // the calls' triples, consumed on the main stream
        RingArray<unsigned> h_tri;         // [B][PP_GROUND_MAX_HYP][3] per slot
        int batch = 0;                     // frames of the last run (pp_get_ground; 0: none, or made stale by a new configuration)
        int run_words = 0;                 // ... ceil(max_n / 64) of it
        int run_k = 0;                     // ... and its hypotheses
        unsigned long long gen = 0;        // ... and the resident_gen it belongs to
        int used = 0;                      // PP_GROUND_* bits: the readers whose last queued run took the classes (ground_for)
    } ground;
    unsigned long long resident_gen = 0;   // counts the changes of the resident frames (set_resident, a stage call)
    unsigned long long results_gen = 0;    // resident_gen of the last pp_detect_async

    int prof = 0;
    // pp_detect_async as one hipGraph launch, captured on first use per key.  The key is a DetectKey: whatever a pass
    // reads that is neither behind a device pointer nor dropped by graph_invalidate.  detect_key (pp_api.hip) builds it and
    // is the only place to extend it: lookup and fill-in compare and assign the value as a whole.
    struct GraphSlot {
        hipGraphExec_t exec = nullptr;
        DetectKey key;
        unsigned long long used = 0;      // graph_tick of its last launch
    };
    GraphSlot graphs[8];          // small LRU
    unsigned long long graph_tick = 0;
    int graph_state = 0;          // 0: try, -1: capture failed once (use plain launches)
    std::vector<hipEvent_t> events;
    std::vector<KTime> ktimes;
    int ev_used = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr;
};

// records the message on the handle (e == NULL: for pp_last_error(NULL)) and returns `code`
int fail(pp_engine* e, int code, const char* fmt, ...);

#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t _st = (call);                                                                     \
        if (_st != hipSuccess)                                                                       \
            return fail(e, PP_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(_st), __FILE__, __LINE__); \
    } while (0)

// ---- what every call that takes ego poses refuses (pp_sweeps_accumulate*, pp_set_track_pose): P is stream b's [3][4]
// sensor-to-fixed [R | t], row-major ----
constexpr double PP_POSE_ORTHO_TOL = 1e-6;      // largest |R R^T - I| entry of an accepted rotation (sweeps.ORTHO_TOL)
inline int pose_check_finite(pp_engine* e, const char* who, const double* P, int b) {
    for (int i = 0; i < 12; ++i)
        if (!std::isfinite(P[i])) return fail(e, PP_ERR_ARG, "%s: poses: stream %d: row %d, column %d is not finite", who, b, i / 4, i % 4);
    return PP_OK;
}
inline int pose_check_orthonormal(pp_engine* e, const char* who, const double* P, int b) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double gij = (P[i * 4] * P[j * 4] + P[i * 4 + 1] * P[j * 4 + 1]) + P[i * 4 + 2] * P[j * 4 + 2];
            if (!(std::fabs(gij - (i == j ? 1.0 : 0.0)) <= PP_POSE_ORTHO_TOL))
                return fail(e, PP_ERR_ARG, "%s: poses: the rotation of stream %d is not orthonormal (R R^T [%d][%d] = %.9g)", who, b, i, j, gij);
        }
    return PP_OK;
}
// Both, stream by stream: finite, the stream's stamp (stamps NULL: the call has none), orthonormal, then `more(b, P)`
template <typename More>
int check_poses(pp_engine* e, const char* who, const double* poses, const double* stamps, int batch, More more) {
    for (int b = 0; b < batch; ++b) {
        const double* P = poses + (size_t)b * 12;
        if (int st = pose_check_finite(e, who, P, b)) return st;
        if (stamps && !std::isfinite(stamps[b])) return fail(e, PP_ERR_ARG, "%s: stamps: the stamp of stream %d is not finite", who, b);
        if (int st = pose_check_orthonormal(e, who, P, b)) return st;
        if (int st = more(b, P)) return st;
    }
    return PP_OK;
}

// ---- the calls that need no handle: host buffers in, host buffers out, device memory for the call's duration ----
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
int check_device(const char* who, int device);          // pp_api.hip: a HIP device exists and `device` names one
// (expects the entry point's name in a local `who`)
#define DEVCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(nullptr, PP_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)); } while (0)

template <typename Tp>
int dalloc(pp_engine* e, Tp** p, size_t count) {
    void* q = nullptr;
    size_t bytes = count * sizeof(Tp);
    if (bytes == 0) bytes = sizeof(Tp);
    HIPCHK(e, hipMalloc(&q, bytes));
    e->allocs.push_back(q);
    *p = (Tp*)q;
    return PP_OK;
}
// a run of allocations that stops at the first failure: `DevAlloc A{e}; A(&p, n); A(&q, m); return A.st;`
struct DevAlloc {
    pp_engine* e;
    int st = PP_OK;
    template <typename Tp> void operator()(Tp** p, size_t count) { if (st == PP_OK) st = dalloc(e, p, count); }
};
template <typename Tp>
int dgrow(pp_engine* e, Tp** p, size_t* cap, size_t count) {
    if (count <= *cap && *p) return PP_OK;
    if (*p) { (void)hipStreamSynchronize(e->stream); (void)hipFree(*p); *p = nullptr; *cap = 0; }
    void* q = nullptr;
    HIPCHK(e, hipMalloc(&q, (count ? count : 1) * sizeof(Tp)));
    *p = (Tp*)q;
    *cap = count;
    return PP_OK;
}

// ---- profiling: an event pair around each kernel launch ----
inline void prof_reset(pp_engine* e) { e->ktimes.clear(); e->ev_used = 0; }
int prof_event(pp_engine* e);

// Stage scope: the kernel launches inside record their own start / stop events (PP_LAUNCH) under `name`
// (NULL: under each launch site's kernel name); non-kernel work (a memset) is bracketed with plain event records.
struct ProfScope {
    pp_engine* e;
    int e1 = -1;
    PpProf saved;          // scopes nest (pp_train_step wraps the voxeliser's named scopes)
    ProfScope(pp_engine* en, const char* name, bool bracket = false) : e(en), saved(g_pp_prof) {
        if (e->prof <= 0) return;
        if (bracket) {
            int e0 = prof_event(e);
            e1 = prof_event(e);
            if (e0 < 0 || e1 < 0) { e1 = -1; return; }
            (void)hipEventRecord(e->events[e0], e->stream);
            e->ktimes.push_back({name, e0});
        } else {
            g_pp_prof.e = e;
            g_pp_prof.tag = name;
        }
    }
    ~ProfScope() {
        if (e1 >= 0) (void)hipEventRecord(e->events[e1], e->stream);
        g_pp_prof = saved;
    }
};

// ---- pp_api.hip: the pipeline stages (all enqueue on e->stream; run_voxelize on `vs` when given) ----
int run_voxelize(pp_engine* e, int batch, int max_n, hipStream_t vs = nullptr);
int finish_async_upload(pp_engine* e, int batch);  // voxelises behind a copy-stream upload (where allowed), records ev_up
int check_batch(pp_engine* e, int batch);
int check_numeric(pp_engine* e, const int* n_dets, int B, const char* who);   // PP_ERR_NUMERIC for a flagged frame
// result rows per frame in the handle's current class mode (pp_get_detection_rows)
inline int det_rows(const pp_engine* e) {
    return (e->rule.class_nms == PP_CLASS_NMS_PER_CLASS ? e->ncls : 1) * e->cfg.nms_post_max_size;
}
int graph_bucket(const pp_engine* e, int max_n);
inline bool graphs_enabled(const pp_engine* e) { return !e->plan_env.sw.no_graph; }   // PP_NO_GRAPH=1: plain launches
// Captures what `enqueue` queues on e->stream (thread-local capture) and instantiates it into *out.  false, with *out
// NULL and the sticky HIP error cleared, when a step of that fails; *enqueue_status (optional) is what `enqueue` returned.
bool capture_exec(pp_engine* e, const std::function<int()>& enqueue, hipGraphExec_t* out, int* enqueue_status);
inline void destroy_exec(hipGraphExec_t* x) { if (*x) (void)hipGraphExecDestroy(*x); *x = nullptr; }
void drop_detect_graphs(pp_engine* e);                  // waits for the stream, destroys the captured inference passes
void decide_sparse_canvas(pp_engine* e);                // from layer 0's weights (pp_finalize_weights, a publish)
int publish_reapply(pp_engine* e);                      // api_publish.hip: pp_set_gemm_precision on published weights
// ---- pp_api.hip: the resident frames' state, one function per transition ----
int wait_for_upload(pp_engine* e, hipStream_t s);       // `s` behind an upload / voxeliser queued on the copy stream
int copies_done(pp_engine* e, hipStream_t up);          // the main stream behind the copies queued on `up` (ev_tgt)
int flip_input(pp_engine* e);                           // to the other input buffer and voxeliser set; returns its index
void set_resident(pp_engine* e, int batch, const int* off, int max_n, bool exact);
int require_host_exact(pp_engine* e, const char* who);  // refuses frames whose sizes only the device knows
int resident_points(pp_engine* e, int batch, hipStream_t s, bool materialise, const float** src);
int ensure_spare_pts(pp_engine* e);

int ensure_loss_buffers(pp_engine* e);                  // api_train.hip
int track_check_pass(pp_engine* e);                     // api_track.hip: what a tracked pass refuses, before anything is queued
int run_track(pp_engine* e, int batch);                 // api_track.hip: k_track_step on this pass's d_dets / d_ndets
void track_release(pp_engine* e);                       // ... what pp_destroy frees of it (page-locked memory, events)
void sweeps_release(pp_engine* e);                      // api_sweeps.hip: what pp_destroy frees of the sweep rings
void costmap_release(pp_engine* e);                     // api_costmap.hip: what pp_destroy frees of the costmap stage
void occupancy_release(pp_engine* e);                   // api_occupancy.hip: what pp_destroy frees of the occupancy maps
void inflate_release(pp_engine* e);                     // api_inflate.hip: what pp_destroy frees of the inflation stage
void navfn_release(pp_engine* e);                       // api_navfn.hip: what pp_destroy frees of the navigation-function stage
// api_navfn.hip, for the stage behind it (api_local_plan.hip).  settle: waits for `s`, then queues rounds in groups until
// the last round of every grid changed nothing.  settled_run: what the getters start with, the source's last run, settled.
int settle(pp_engine* e, const char* who, const NavParams& p, int* rounds, hipStream_t s, std::vector<int>& host);
int settled_run(pp_engine* e, const char* who, int source, int batch, pp_engine::Navfn** out);
void local_plan_release(pp_engine* e);                  // api_local_plan.hip: what pp_destroy frees of the local planner
// api_local_plan.hip, for every stage that reads the field in place: the source's navigation function has run on the
// inflated grids that still lie there
int check_navfn_run(pp_engine* e, const char* who, int source);
void frontier_release(pp_engine* e);                    // api_frontier.hip: what pp_destroy frees of the frontier stage
void scan_match_release(pp_engine* e);                  // api_scan_match.hip: what pp_destroy frees of the scan match
void object_mask_release(pp_engine* e);                 // api_object_mask.hip: what pp_destroy frees of the object mask
void ground_release(pp_engine* e);                      // api_ground.hip: what pp_destroy frees of the ground stage
int ensure_metrics(pp_engine* e);                       // api_metrics.hip
void fill_metrics_params(pp_engine* e, int batch, MetricsParams& p);   // ... on the handle's head map and loss.labels
// ---- api_dataprep.hip: what the fused training steps (api_train.hip) queue ----
int check_gt(pp_engine* e, const char* who, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
             int batch, const pp_target_config* tc, int64_t* total);
int check_aug(pp_engine* e, const char* who, int batch, int64_t total, const pp_augment_config* ac,
              const pp_aug_frame* frames, const double* box_draws);
int check_gts(pp_engine* e, const char* who, const int32_t* gt_counts, int batch, const pp_gt_sample_config* sc,
              const pp_gts_cand* cands, const int32_t* cand_counts, int* max_out_n, std::vector<int>* bound_off);
int enqueue_targets(pp_engine* e, int batch, const GtSet& gt, bool resident_mask, const pp_target_config* tc, bool extra);
int targets_from_host(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                      int64_t total, bool resident_mask, const pp_target_config* tc, bool extra, hipStream_t up);
int enqueue_augment(pp_engine* e, int batch, const GtSet& in, int64_t total, const pp_augment_config* ac,
                    const pp_aug_frame* frames, const double* box_draws, hipStream_t up,
                    const std::vector<int>* draw_off = nullptr);
int augment_from_host(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                      const int32_t* gt_counts, int64_t total, const pp_augment_config* ac, const pp_aug_frame* frames,
                      const double* box_draws, hipStream_t up);
int enqueue_gt_sample(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                      const int32_t* gt_counts, int64_t total, const pp_gt_sample_config* sc, const pp_gts_cand* cands,
                      const int32_t* cand_counts, int max_out_n, hipStream_t up);

// ---- the stages on the resident frames: one entry check, one rewrite path ----
// What every call on the resident frames refuses before it looks at its own values (`hint`: how frames get there) ...
inline int check_resident_call(pp_engine* e, const char* who, int batch, const char* hint) {
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    if (e->cur_batch < 1) return fail(e, PP_ERR_STATE, "%s: no frames are resident (%s)", who, hint);
    if (int st = check_batch(e, batch)) return st;
    if (batch != e->cur_batch) return fail(e, PP_ERR_ARG, "%s: %d frames are resident, batch is %d", who, e->cur_batch, batch);
    return PP_OK;
}
// ... and what a reader of a stage's last run refuses (last_batch 0: there was none; `while_training`: it may run then)
inline int check_last_run(pp_engine* e, const char* who, int last_batch, int batch, bool while_training, const char* none,
                          const char* run, const char* unit) {
    if (!while_training && e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    if (last_batch < 1) return fail(e, PP_ERR_STATE, "%s: %s", who, none);
    if (batch != last_batch) return fail(e, PP_ERR_ARG, "%s: the last %s had %d %s, batch is %d", who, run, last_batch, unit, batch);
    return PP_OK;
}
// What a reader of the resident rows (`bit`: its PP_OBJMASK_* name) asks before it takes a ring slot or queues anything:
// *words stays NULL while the object mask is off or does not name the reader; a named reader without a mask of the
// resident frames is refused -- it never runs unmasked silently
inline int object_mask_for(pp_engine* e, const char* who, int bit, int batch, const unsigned long long** words, int* stride) {
    const pp_engine::ObjMask& g = e->omask;
    *words = nullptr; *stride = 0;
    if (!g.on || !(g.cfg.consumers & bit)) return PP_OK;
    if (g.batch != batch || g.gen != e->resident_gen)
        return fail(e, PP_ERR_STATE, "%s: the object mask names this stage and holds no mask of the resident frames (pp_object_mask_async first)", who);
    *words = g.words; *stride = g.stride;
    return PP_OK;
}
// The same question for the ground stage's classes (`bit`: the reader's PP_GROUND_* name): *gnd and *obs stay NULL while the
// stage is off or does not name the reader; a named reader without classes of the resident frames is refused
inline int ground_for(pp_engine* e, const char* who, int bit, int batch, const unsigned long long** gnd, const unsigned long long** obs,
                      int* stride) {
    pp_engine::Ground& g = e->ground;
    *gnd = nullptr; *obs = nullptr; *stride = 0;
    if (!g.on || !(g.cfg.consumers & bit)) { g.used &= ~bit; return PP_OK; }
    if (g.batch != batch || g.gen != e->resident_gen)
        return fail(e, PP_ERR_STATE, "%s: the ground stage names this stage and holds no classes of the resident frames (pp_ground_async first)", who);
    *gnd = g.gnd; *obs = g.obs; *stride = g.stride;
    g.used |= bit;                                         // (pp_ground_used; a later refusal of the same call leaves the run before it, which took them or not)
    return PP_OK;
}
// both streams idle: nothing queued reads a stage's tables any more
inline int quiesce(pp_engine* e) {
    HIPCHK(e, hipEventSynchronize(e->ev_up));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

// What pp_set_costmap and pp_set_occupancy refuse alike: a NaN in any double (an infinity where `finite`), a window that
// is empty or larger than max_cells
struct CfgDouble { const char* name; double v; bool finite; };
inline int check_cfg_doubles(pp_engine* e, const char* who, std::initializer_list<CfgDouble> f) {
    for (const CfgDouble& d : f)
        if (std::isnan(d.v) || (d.finite && !std::isfinite(d.v))) return fail(e, PP_ERR_ARG, "%s: %s is not finite", who, d.name);
    return PP_OK;
}
inline int check_cfg_window(pp_engine* e, const char* who, int width, int height, int max_cells, const char* max_name) {
    if (width < 1) return fail(e, PP_ERR_ARG, "%s: width = %d must be >= 1", who, width);
    if (height < 1) return fail(e, PP_ERR_ARG, "%s: height = %d must be >= 1", who, height);
    if ((long long)width * height > max_cells)
        return fail(e, PP_ERR_ARG, "%s: width * height = %lld cells, at most %s = %d", who, (long long)width * height, max_name, max_cells);
    return PP_OK;
}

// What pp_set_local_plan, pp_set_scan_match and their stand-alone calls take as the trig table: int32 [n_trig][2] = (C, S)
// -> a word per tick, C as int16 in the low half, S in the high half
constexpr int PP_TRIG_ONE = 16384;
inline int pack_trig(pp_engine* e, const char* who, const int32_t* trig, int n_trig, std::vector<unsigned>& out) {
    if (!trig) return fail(e, PP_ERR_ARG, "%s: trig is NULL", who);
    if (n_trig != PP_LOCAL_HEADINGS) return fail(e, PP_ERR_ARG, "%s: the trig table has %d entries, it must have PP_LOCAL_HEADINGS = %d", who, n_trig, PP_LOCAL_HEADINGS);
    out.resize((size_t)PP_LOCAL_HEADINGS);
    for (int h = 0; h < PP_LOCAL_HEADINGS; ++h) {
        const int c = trig[2 * h], s = trig[2 * h + 1];
        if (c < -PP_TRIG_ONE || c > PP_TRIG_ONE || s < -PP_TRIG_ONE || s > PP_TRIG_ONE)
            return fail(e, PP_ERR_ARG, "%s: trig[%d] = (%d, %d) outside [-%d, %d]", who, h, c, s, PP_TRIG_ONE, PP_TRIG_ONE);
        out[(size_t)h] = ((unsigned)c & 0xFFFFu) | ((unsigned)s << 16);
    }
    return PP_OK;
}

// Every writer of a new set of frames starts here: the other input buffer, `stream` behind the pass that last read it
inline int flip_for_write(pp_engine* e, hipStream_t stream) {
    const int nb = flip_input(e);
    HIPCHK(e, hipStreamWaitEvent(stream, e->ev_read[nb], 0));
    return PP_OK;
}
// A stage that replaces the resident frames (crop, sweeps) reads them where they lie and writes the new cloud into the
// other input buffer:  rewrite_run(enqueue: rewrite_begin, the stage's copies and launch, rewrite_end) [rewrite_sync_tail]
struct Rewrite {
    const float* src = nullptr;        // the frames as the stage's kernels read them, and their offsets
    const int* offsets_in = nullptr;
    int old = 0;                       // the input buffer they lie in
    std::vector<int> bound;            // the host's offsets (bounds) of the frames read; the stage may put the bounds of
    int max_n = 0;                     // what it writes in their place -- rewrite_end makes them the resident ones
};
inline int rewrite_begin(pp_engine* e, int batch, hipStream_t stream, Rewrite* w) {
    if (int st = resident_points(e, batch, stream, true, &w->src)) return st;
    w->offsets_in = e->d_offsets;
    w->bound = e->h_cur_off;           // (set_resident assigns the vector it would otherwise read)
    w->max_n = e->cur_max_n;
    w->old = e->in_buf;
    return flip_for_write(e, stream);
}
// behind the stage's launch; the host then knows bounds only: set_resident, not exact
inline int rewrite_end(pp_engine* e, int batch, const Rewrite& w, hipStream_t stream) {
    HIPCHK(e, hipGetLastError());
    // the next upload flips back to the buffer read here: its writer waits for this event as for a pass
    if (stream != e->stream) HIPCHK(e, hipEventRecord(e->ev_read[w.old], stream));
    set_resident(e, batch, w.bound.data(), w.max_n, false);
    return PP_OK;
}
// Either entry point of such a stage, its checks passed: `enqueue(stream)` on the main stream behind an asynchronous call
// that may still use the stage's tables, or on the copy stream behind what the main stream holds now (frames fed there, the
// pass reading the buffer written, a synchronous call on the same tables), then as pp_upload_points_async ends.
template <typename Enqueue>
int rewrite_run(pp_engine* e, int batch, bool asynchronous, Enqueue enqueue) {
    (void)hipSetDevice(e->device);
    if (asynchronous) {
        HIPCHK(e, hipEventRecord(e->ev_main, e->stream));
        HIPCHK(e, hipStreamWaitEvent(e->copy_stream, e->ev_main, 0));
    } else HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_up, 0));
    prof_reset(e);
    if (int st = enqueue(asynchronous ? e->copy_stream : e->stream)) return st;
    return asynchronous ? finish_async_upload(e, batch) : PP_OK;
}
// The synchronous tail: the frames' counts come back, are held against the host's bounds and become the host's offsets;
// the points are handed out when asked for.  Formats: bad_count (who, frame, count, bound), small_out (who, capacity, total).
inline int rewrite_sync_tail(pp_engine* e, const char* who, const char* bad_count, const char* small_out, const int* d_counts,
                             int batch, int32_t* counts_out, float* points_out, int64_t points_capacity) {
    HIPCHK(e, hipMemcpyAsync(counts_out, d_counts, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<int> off((size_t)batch + 1, 0);
    int max_n = 0;
    for (int b = 0; b < batch; ++b) {
        const int bound = e->h_cur_off[(size_t)b + 1] - e->h_cur_off[(size_t)b];
        if (counts_out[b] < 0 || counts_out[b] > bound) return fail(e, PP_ERR_HIP, bad_count, who, b, counts_out[b], bound);
        off[(size_t)b + 1] = off[(size_t)b] + counts_out[b];
        max_n = std::max(max_n, counts_out[b]);
    }
    set_resident(e, batch, off.data(), max_n, true);
    if (points_out) {
        const int total = off[(size_t)batch];
        if (points_capacity < total) return fail(e, PP_ERR_ARG, small_out, who, (long long)points_capacity, total);
        if (total) HIPCHK(e, hipMemcpy(points_out, e->d_points, (size_t)total * e->F * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PP_OK;
}
