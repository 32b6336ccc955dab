// Internal declarations shared by the HIP translation units of libpp_hip.so.
// gfx950 (MI355X / CDNA4) only: 64-wide wavefronts are assumed throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include <hip/hip_ext.h>

#include "../../include/pp_hip.h"

#define PP_WAVE 64
// float16 pieces per value of the split-precision GEMM operands (backbone.hip), i.e. in the weight layouts pp_api.hip
// writes ([cin/16][PP_NPIECE][n][16] 16-bit words)
#define PP_NPIECE 2
// zeroed floats in front of every activation buffer (>= the widest layer input, 384 channels):
// the GEMM producers read convolution zero-padding from there instead of masking loaded values
#define PP_ZPAD_FLOATS 512
// fused head map: one 128-byte row per head-map pixel: [box napl*7 | cls napl*ncls | dir napl*2 | 0 pad]
#define PP_HEAD_COLS 32

// ----- kernel launches ----------------------------------------------------
// Every hot-path kernel is launched through PP_LAUNCH.  Normally that is a plain hipLaunchKernelGGL.  While a
// handle collects per-kernel times (pp_set_profiling; plain launches, never inside a graph capture) the launch
// carries a start / stop event pair of its own (hipExtLaunchKernelGGL): the pair brackets the kernel's execution
// on the device -- the same interval rocprofv3's kernel trace reports -- not the gaps between launches.
struct PpProf {
    pp_engine* e;       // handle collecting times on this thread (NULL: none)
    const char* tag;    // name to record ("<kernel symbol>:<layer>"), or NULL: the launch site's own name
};
extern thread_local PpProf g_pp_prof;
bool pp_prof_events(const char* name, hipEvent_t* start, hipEvent_t* stop);   // pp_api.hip
#define PP_LAUNCH(NAME, KERNEL, GRID, BLOCK, SHMEM, STREAM, ...)                                            \
    do {                                                                                                    \
        hipEvent_t pe0_ = nullptr, pe1_ = nullptr;                                                          \
        if (g_pp_prof.e != nullptr && pp_prof_events(NAME, &pe0_, &pe1_))                                   \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, pe0_, pe1_, 0, __VA_ARGS__);          \
        else                                                                                                \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, SHMEM, STREAM, __VA_ARGS__);                            \
    } while (0)

// inclusive prefix sum over the 64 lanes of a wave with DPP adds (row shifts inside the rows of 16, then the two row
// broadcasts): six short VALU operations instead of six ds_bpermute round trips (__shfl_up) -- the scans of the
// single-workgroup stages are dependent chains: their latency is what they cost
// Requirements: all 64 lanes of the wave active at the call (the row shifts read inactive lanes as 0 only through
// bound_ctrl; every caller scans whole waves), and a wave64 GFX9 target: row_bcast:15 / :31 do not exist elsewhere.
// This library is written for gfx950 only -- any other --offload-arch stops here instead of mis-scanning.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "pp_common.h: the DPP wave scans (row_bcast) and the MFMA kernels of this library target gfx950 (MI355X) only"
#endif
__device__ __forceinline__ int wave_inclusive_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);   // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);   // row_bcast:31 into rows 2 and 3
    return v;
}


// ----- numeric guard of the split-precision GEMM path ----------------------------------
// v_max_f32 (fmaxf) returns the OTHER operand when one is a NaN: a ReLU written with it would turn the NaN an
// out-of-range activation produces (two float16 pieces: |x| >= 65520 -> inf - inf) into a clean 0 and the frame into
// silently wrong boxes.  The backbone's ReLUs keep a NaN, so it reaches the head maps, where the post-process sees it
// (bit PP_NDETS_NONFINITE of a frame's detection count -> PP_ERR_NUMERIC).
__device__ __forceinline__ float relu_keep_nan(float x) { return (x < 0.f) ? 0.f : x; }
// BatchNorm statistics partials are centred: (n, s, m2) = (rows, sum, sum of squared deviations about the rows' own
// mean).  Chan et al.'s pairwise merge: (n, s, m2) += (nb, sb, m2b); an empty side (count 0) changes nothing.  The
// deviation of the two means is what a sum of squares about zero would lose to cancellation (|mean| / std large).
__device__ __forceinline__ void bn_chan_merge(float& n, float& s, float& m2, float nb, float sb, float m2b) {
    if (nb <= 0.f) return;
    if (n > 0.f) {
        const float d = sb / nb - s / n;
        m2 = (m2 + m2b) + d * d * (n * nb / (n + nb));
    } else {
        m2 = m2b;
    }
    n += nb;
    s += sb;
}
__device__ __forceinline__ bool pp_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
#define PP_NDETS_NONFINITE (1 << 30)

// ----- voxel grid geometry (float64, as the reference's index math) -----
struct VoxGeom {
    double lo[3];   // range minimum x y z
    double vs[3];   // voxel size x y z
    int grid[3];    // nx ny nz = round((max-min)/vs)
    int ncell;      // nx*ny*nz
};

// ----- one GEMM-shaped layer of the RPN ---------------------------------
enum LayerKind { LAYER_SEP = 0, LAYER_DECONV = 1, LAYER_HEAD = 2 };

struct LayerDesc {
    int kind;
    int cin, cout;        // channels in / out (cout of ONE tap for deconv)
    int stride;           // depthwise stride (sep)
    int k;                // deconv kernel == stride
    int in_h, in_w;       // input map
    int out_h, out_w;     // output map (sep: strided; deconv: in*k; head: in)
    int n_total;          // GEMM N: cout (sep), k*k*cout (deconv), 32 (head, zero padded)
    float* d_dw;          // [9][cin] depthwise taps (sep)
    float* d_wt;          // [n_total][cin] BN-folded, transposed
    float* d_wt16;        // the same weights as three bf16 pieces, [cin/16][3][n_total][16] 16-bit words (or NULL)
    float* d_bias;        // [cout] (sep/deconv: folded BN shift) or [32] (head)
    const float* in;      // input activation  [B, in_h, in_w, cin]
    float* out;           // output base
    int ld_out;           // channels per output pixel row (row stride, floats)
    int co_off;           // channel offset inside the output row (concat placement)
    // heads fused into a deconv's epilogue (head_mode 1: write partial + bias, 2: add partial)
    int head_mode;
    float* d_head_wt;     // [PP_HEAD_COLS][cout] slice of the head kernels, transposed
    float* d_head_bias;   // [PP_HEAD_COLS]
    float* d_head_wt16;   // d_head_wt as three bf16 pieces, [cout/16][3][PP_HEAD_COLS][16] 16-bit words (or NULL)
    // sparse canvas (first layer only): cell -> pillar map [batch][occ_nz][in_h][in_w]; a window position whose
    // cell holds no pillar is read from the zero header instead of the (unwritten) canvas.  NULL: dense input
    const int* d_occ;
    int occ_nz;
    // the same occupancy as a bitmap (PfnParams::occbits), when this pass's PFN launch wrote it: three 16-byte-free
    // lookups per window instead of one per window element and z-cell.  NULL: the cell map is consulted
    const unsigned long long* d_occbits;
    // compact class-logit plane [B * H' * W'][cls_ncol], written by the LAST fused-head deconv (NULL elsewhere)
    float* d_cls_plane;
    int cls_col0, cls_ncol;
    const char* name;
};

// ----- launchers (each in its own .hip file) ----------------------------
// small batches (the latency case) are fed without a copy engine: the first kernel reads the frames' offsets and
// points straight from the caller's page-locked buffer (device-mapped) through this page-locked descriptor and
// leaves the device copies the later kernels use (pts_dst / offsets_dst); feed == NULL: inputs are on the device
struct PpFeed {
    const float* src;        // device address of the caller's page-locked points [sum N, F]
    int pad_[2];
    int offsets[1];          // [batch + 1] follow
};
// (occbits != NULL: the frames' occupancy bitmaps, occ_n 64-bit words each, are cleared by the same launch)
void launch_cell_first(const float* pts, const int* offsets, int batch, int max_n, int F, const VoxGeom& g,
                       int* cell, int* first, int* cellmap, const PpFeed* feed, float* pts_dst, int* offsets_dst,
                       hipStream_t s, unsigned long long* occbits = nullptr, int occ_n = 0);
// returns (through *sorted_in_b) nothing; the host derives the final buffer from voxel_sort_passes()
int voxel_sort_passes(int max_voxels);
bool voxel_first_in_lds(int max_n, int ncell, int max_voxels);   // pass first = NULL to both launchers below
void launch_voxel_frame(const int* offsets, const int* cell, const int* first, int* cellmap, unsigned* keyA,
                        unsigned* idxA, unsigned* keyB, unsigned* idxB, int* pillar_start, int* pillar_cell,
                        int* npillars, int* nvalid, int batch, int max_n, int ncell, int max_voxels, hipStream_t s);
// first[i] = v for i < n (k_voxel_frame's global-memory path: every cell "no point yet" before k_cell_first)
void launch_fill_first(int* first, int v, long long n, hipStream_t s);
// pts_sorted[n0 + j] = pts[n0 + sorted_idx[n0 + j]], j < nvalid[frame]: the pillar-sorted copy the PFN streams
void launch_sort_points(const float* pts, const int* offsets, const unsigned* sorted_idx, const int* nvalid, int batch,
                        int max_n, int F, float* pts_sorted, hipStream_t s);
// pts_sorted: the pillar-sorted copy k_voxel_frame leaves ([sum N][F], frame b's valid points at offsets[b]..)
void launch_voxel_expand(const float* pts_sorted, const int* offsets, const unsigned* sorted_idx, const int* pillar_start,
                         const int* pillar_cell, const int* npillars, int frame, int F, int T, int max_voxels,
                         int ny, int nx, float* voxels, int* coors, int* num_points, hipStream_t s);
void launch_build_cellmap(const int* coors4, int64_t P, int ncell, int ny, int nx, int* cellmap, hipStream_t s);

struct PfnParams {
    // geometry
    int batch, nz, ny, nx, C, F, T, max_voxels;
    float vx, vy, x_off, y_off;
    // weights: w [Fa][C] folded, bias [C] folded
    const float* w;
    const float* bias;
    // cell -> pillar map [batch][nz][ny][nx]
    const int* cellmap;
    // CSR source: pillar-sorted points (frame b: rows offsets[b] + pillar_start[b][p] .. of pts_sorted)
    const float* pts_sorted;
    const int* offsets;
    const int* pillar_start;
    // pillar-centric launch (sparse canvas): linear (z, y, x) cell of every pillar [batch][max_voxels], pillars per frame [batch]
    const int* pillar_cell;
    const int* npillars;
    // ... which also leaves the frame's occupancy bitmap (occ_words(nx) 64-bit words per grid row, bit x + 1 of a row
    // = "a pillar in column x, any z"; cleared by k_cell_first): what the sparse first layer and the one-launch
    // anchor mask read instead of the cell map.  NULL: not written
    unsigned long long* occbits;
    // padded source (compat)
    const float* voxels;
    const int* num_points;
    // outputs
    float* canvas;    // [batch][ny][nx][C]
    int sparse;       // 1: only cells that hold a pillar are written (the first layer consults the cell map)
    int with_distance;  // 1: one more input feature, the point's Euclidean norm (w has F + 6 rows)
    float* feat_out;  // optional [P][C]
    // few frames (the latency case): one extra workgroup per frame of the PFN launch computes the frame's anchor mask
    // (it depends on the voxeliser's cell map only, and nothing before the post-process reads it): NULL = not fused
    const int* am_cells;   // [A][4] static anchor cells
    int64_t am_A;
    float am_threshold;
    uint8_t* am_mask;      // [batch][A]
};
struct PpSwitches;   // pp_switches.h: the process's PP_* switches
struct PlanEnv;      // pp_plan.h: compute units + switches, what the choice of a kernel depends on besides the shapes
bool pfn_can_carry_anchor_mask(const PfnParams& p, bool padded_source, const PpSwitches& sw);   // would launch_pfn run the extra workgroups?
bool pfn_writes_occbits(const PfnParams& p, bool padded_source, const PpSwitches& sw);   // would launch_pfn's kernel set PfnParams::occbits?
int launch_pfn(const PfnParams& p, bool padded_source, const PpSwitches& sw, hipStream_t s);  // returns 0 or PP_ERR_UNSUPPORTED

void launch_anchor_mask(const int* cellmap, int batch, int nz, int ny, int nx, const int* cells, int64_t A,
                        float threshold, int* integ, uint8_t* mask, hipStream_t s);
// 64-bit words per grid row of the occupancy bitmap: bits 0 .. nx + 1 (bit x + 1 = column x; bit 0 = the padding
// column x = -1) plus one spare word, so that a reader may always fetch the word after the one its window starts in
__host__ __device__ static inline int occ_words(int nx) { return (nx + 2 + 63) / 64 + 1; }
// the anchor mask from the occupancy bitmap (nz == 1 grids: a bit is a count): one launch, no integral image
void launch_anchor_mask_bits(const unsigned long long* occbits, int batch, int ny, int nx, const int* cells, int64_t A,
                             float threshold, uint8_t* mask, hipStream_t s);

bool deconv_can_fuse_heads(const LayerDesc& L);
bool layer_writes_cls_plane(const LayerDesc& L, const PlanEnv& env);   // does this layer's kernel leave the compact class-logit plane?
bool sparse_input_supported(const LayerDesc& L, int batch, const PlanEnv& env);   // may L's input be a canvas with unwritten empty cells?
std::string layer_kernel_name(const LayerDesc& L, int batch, const PlanEnv& env);  // template instantiation that runs L at this batch
// the same with the SH argument the tags leave out; reads no device state
std::string layer_plan_name(const LayerDesc& L, int batch, const PlanEnv& env);
// training-mode forward of one separable layer (backbone.hip: k_sep_u<..., TR = 1>; called by train.hip)
struct SepTrainArgs {
    const float* in;             // input map [batch][in_h][in_w][cin] with a PP_ZPAD_FLOATS header in front: NaN-filled when
                                 // `coef` is given (relu(NaN * sc + sh) = 0 is the padding), zero-filled otherwise
    const float4* coef;          // [cin] (sc, sh, ., .) when `in` is a pre-BatchNorm map, NULL when it is an activation
    const float* dw;             // depthwise kernel [3][3][cin]
    const unsigned short* wt16;  // this step's pointwise kernel as two float16 pieces, [cin / 16][2][cout][16]
    float* Z;                    // out: pre-BatchNorm map [rows][cout]
    float* D;                    // out: depthwise output [rows][cin]
    float* stat;                 // out: statistics partials [rows written][2][cout] (one row per workgroup; at most
                                 // ceil(rows / 128) + 7 of them)
    int batch, in_h, in_w, cin, out_h, out_w, cout, stride;
    const char* tag;             // profiler name of the launch ("k_sep_u_tr:<layer>")
};
int launch_sep_train(const SepTrainArgs& t, int cus, hipStream_t s);   // rows of `stat` written, 0: shape not supported
// ... and of a plain product out[rows][N] = in[rows][K] . W (+ bias): the transposed convolutions' forward GEMMs, the heads
struct RowsTrainArgs {
    const float* in;             // [rows][K], rows contiguous (no header needed)
    const unsigned short* wt16;  // W as two float16 pieces, [K / 16][2][N][16]
    const float* bias;           // [N] or NULL
    float* out;                  // [rows][ld_out]
    float* stat;                 // statistics partials [rows written][2][N], or NULL
    long long rows;
    int K, N, ld_out;
    const char* tag;
};
int launch_rows_train(const RowsTrainArgs& t, int cus, hipStream_t s);
int launch_layer(const LayerDesc& L, int batch, float* d_head, hipStream_t s, const PlanEnv& env, int frame0 = 0);  // returns 0 or PP_ERR_UNSUPPORTED
// may L be launched over the frames [frame0, frame0 + batch) of a total_batch-frame batch (k_sep_u's tile sub-ranges)?
bool launch_layer_subrange_ok(const LayerDesc& L, int frame0, int batch, int total_batch, const PlanEnv& env);

struct PostParams {
    int batch;
    int64_t A;
    int pre_max, post_max;
    float score_thr, iou_thr;
    const float* head;     // [batch][H'*W'][PP_HEAD_COLS] fused head map
    const float* cls;      // compact class logits [batch][H'*W'][napl*ncls] (same values as the head map's cls
                           // columns), or NULL: the candidate scan reads the head rows
    int napl;              // anchors per location
    int ncls;              // class logits per anchor (score = max, label = argmax)
    int use_dir;           // 0: no direction head, no flip
    const uint8_t* mask;   // [batch][A]
    const float* anchors;  // [A][7]
    const float* calib;    // [batch][16]  rect @ Trv2c (float32)
    pp_detection* dets;    // [batch][post_max]
    int* n_dets;           // [batch]
    // page-locked host copies the kernel fills itself (or NULL): the kept detections of a frame are a few hundred
    // bytes -- stored straight over the host link they replace two copy nodes (9 us of a replayed step)
    pp_detection* dets_host;
    int* n_dets_host;
    int nms_mode;          // enum pp_nms_mode: which instantiation of the kernel runs
    // pp_set_projection (NULL: off, the other instantiation): p2 [batch][16] float64 row-major; every kept detection's image
    // box (box_project_dev.h) goes to bbox [batch * post_max][4] and, with dets_host, to its page-locked twin
    const double* p2;
    double* bbox;
    double* bbox_host;
    // pp_set_class_nms (enum pp_class_nms).  PP_CLASS_NMS_PER_CLASS: workgroup (b, c) runs the whole pass on class c's score
    // alone and leaves its kept rows in segment (b, c) of the scratch buffers; k_gather_classes then lays the segments end to
    // end into dets / bbox (row stride ncls * post_max), sums the counts into n_dets and fills the page-locked twins
    int class_nms;
    pp_detection* cls_dets;   // [batch][ncls][post_max]
    int* cls_cnt;             // [batch][ncls], each with its own PP_NDETS_NONFINITE flag
    double* cls_bbox;         // [batch][ncls][post_max][4] (with p2)
    // pp_set_soft_nms (read by the PP_NMS_SOFT instantiation only): enum pp_soft_nms_method, sigma of the Gaussian
    // weight, the score under which a re-scored box is dropped.  Nt is iou_thr
    int soft_method;
    float soft_sigma, soft_floor;
};
void launch_postprocess(const PostParams& p, hipStream_t s);

// track.hip: one track table per stream (pp_set_tracking; tracking.py states the rule).  One slot of a stream's table:
struct TrkSlot {
    double x[6];           // x y z vx vy vz
    double p[3];           // p00 p01 p11, shared by the three axes
    double size[3];        // w l h
    double yaw;
    float score;
    int id, label, hits, misses, confirmed;
    int live;              // 0: the slot is free (its other fields are then meaningless)
};
#define PP_TRACK_MASK_ROWS 128     // detection rows per frame the free-row bitmask of k_track_step holds (2 x 64 bits)
// One stream's ego pose on the device (pp_set_track_pose): the [3][4] sensor-to-fixed [R | t], row-major, and
// psi = atan2(R10, R00) from the host -- the kernel only adds and subtracts it
struct TrkPose {
    double m[12];
    double psi;
    int has;               // the queued record: armed for the next step; the previous record: a posed step has run
    int pad;
};
struct TrackParams {
    int batch;                 // streams 0 .. batch - 1 advance by one step
    int rows;                  // row stride of dets (<= PP_TRACK_MASK_ROWS)
    const pp_detection* dets;  // [batch][rows]
    const int* n_dets;         // [batch]; a count with PP_NDETS_NONFINITE leaves its stream untouched
    const pp_track_config* cfg;   // device memory: changing a parameter re-captures nothing
    double* dt;                // [batch] seconds of this step per stream; <= 0: cfg->period.  Consumed (zeroed) by the step,
                               // also for a flagged stream
    TrkSlot* state;            // [B][PP_TRACK_MAX]
    int* next_id;              // [B]
    int* overflow;             // [B]
    TrkPose* pose_q;           // [B] the pose of this step per stream; `has` == 0: none (the step runs exactly as without
                               // ego motion).  Consumed (`has` zeroed) by the step, also for a flagged stream
    TrkPose* pose_prev;        // [B] the pose of the stream's last posed step that ran; rewritten by a posed step
    // page-locked host memory the kernel fills itself (only pp_get_tracks reads them):
    pp_track* out;             // [batch][PP_TRACK_MAX] the live tracks, ascending slot
    int* n_out;                // [batch]
    int* overflow_out;         // [batch]
    // ... and pp_get_tracks_fixed:
    pp_track* out_fixed;       // [batch][PP_TRACK_MAX] the same rows in the fixed frame of the step's pose
    int* n_out_fixed;          // [batch]; -1: the stream's step had no pose
};
void launch_track_step(const TrackParams& p, hipStream_t s);

// loss.hip: training loss at the head maps + gradient with respect to them
struct LossParams {
    int batch;
    int64_t A;             // anchors per frame
    int npx, napl;         // head pixels per frame, anchors per pixel
    int ncls;              // class logits per anchor (num_class; the background column is not encoded)
    const float* head;     // [batch][npx][PP_HEAD_COLS]
    const int* labels;     // [batch][A]  (>0 class, 0 background, -1 ignored)
    const float* reg_targets;  // [batch][A][7]
    const float* anchors;  // [A][7]
    int* npos;             // [batch] scratch: positives per frame
    double* partials;      // [batch * blocks][5] scratch
    float* losses;         // [8] out
    float* head_grad;      // [batch][npx][PP_HEAD_COLS] out, may be NULL
    float alpha, gamma, sigma;
    float code_weight[7];
    float pos_cls_weight, neg_cls_weight;
    float cls_weight, loc_weight, dir_weight;
    int norm_by_num_positives, encode_rad_error_by_sin, use_direction;
};
int loss_blocks(int npx);
int launch_head_loss(const LossParams& p, hipStream_t s);   // 0 or PP_ERR_UNSUPPORTED (anchors per pixel > 3)

// metrics.hip: training metrics at the head map -- accuracy and precision / recall counts of one step
#define PP_METRICS_NTHRESH 7
struct MetricsParams {
    int batch;
    int64_t A;             // anchors per frame (= npx * napl)
    int npx, napl, ncls;
    const float* logits;   // class logit c of anchor r of pixel px of frame b: [(b * npx + px) * row_stride + col_off + r * ncls + c]
    int row_stride, col_off;   // the head map: PP_HEAD_COLS, napl * 7; a plain [batch][A][ncls] array: napl * ncls, 0
    const int* labels;     // [batch][A]  (>0 class, 0 background, -1 ignored)
    int* partials;         // [batch * metrics_blocks(npx)][PP_METRICS_COUNTS] scratch
    long long* counts;     // [PP_METRICS_COUNTS] out (pp_hip.h: acc_hit, n_pos, n_neg, tp[7], fp[7], then zeros)
};
int metrics_blocks(int npx);
int launch_head_metrics(const MetricsParams& p, hipStream_t s);   // 0 or PP_ERR_UNSUPPORTED (as launch_head_loss)

// optim.hip: AdamW update of one flat parameter buffer
void launch_adamw(float* w, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                  float eps, float wd, hipStream_t s);
// ... of the (offset, size) segments seg[2 * i], seg[2 * i + 1] of it only (host array of nseg pairs)
#define PP_ADAMW_SEGS 64      // segments per update launch (the table travels as a kernel argument)
struct AdamwSegs {
    int64_t off[PP_ADAMW_SEGS], size[PP_ADAMW_SEGS];
    int block_start[PP_ADAMW_SEGS + 1];      // a workgroup owns 1 024 consecutive floats of one segment
    int n;
};
// The table of one update launch, shared by k_adamw_seg and k_adamw_seg_clip (grad_clip.hip): the next non-empty
// segments from seg[*done] on, PP_ADAMW_SEGS at most; *done advances past what was taken (empty ones included), src[j]
// (may be NULL) is the index in `seg` of table entry j.  Returns the launch's workgroups.
int adamw_fill_table(AdamwSegs& t, const int64_t* seg, int nseg, int* done, int* src);
void launch_adamw_segments(float* w, const float* g, float* m, float* v, const int64_t* seg, int nseg, float lr_t,
                           float beta1, float beta2, float eps, float wd, hipStream_t s);

// grad_clip.hip: gradient norms per group of segments (float64 sums in a fixed order) and the AdamW update on the
// clipped gradient.  The caller's workspace: the statistics block of pp_hip.h, then the group sums, the partial sums
// and their groups (byte offsets below; max_partials bounds what disjoint segments of n_floats floats can need).
struct GradClipLayout {
    int64_t stats_words, gsum_off, partial_off, pgroup_off, bytes, max_partials;
};
GradClipLayout grad_clip_layout(int64_t n_floats, int n_segments, int n_groups);
int64_t grad_clip_partials(const int64_t* seg, int nseg);      // partial sums these segments produce
// the reduction: one launch per 128 non-empty segments, then one that writes the statistics block for (mode, clip, skip)
void launch_grad_norm(const float* g, const int64_t* seg, int nseg, const int32_t* groups, int ngroups, int mode,
                      float clip, int skip, void* ws, int64_t n_floats, hipStream_t s);
// the update; `ws` (the finished statistics block) may be NULL for PP_CLIP_NONE / PP_CLIP_VALUE without the guard
void launch_adamw_segments_clipped(float* w, const float* g, float* m, float* v, const int64_t* seg, int nseg,
                                   const int32_t* groups, int ngroups, int mode, float clip, int skip, const void* ws,
                                   float lr_t, float beta1, float beta2, float eps, float wd, hipStream_t s);

// rotate_iou.hip: rotated-box overlaps of the AP evaluator
void launch_riou_corners(const float* boxes, int64_t n, float* corners, hipStream_t s);
void launch_riou_pairs(const float* bc, int64_t N, const float* qc, int64_t K, int criterion, float* out, hipStream_t s);
void launch_d3_finish(const double* boxes, int64_t N, const double* qboxes, int64_t K, int criterion,
                      const float* rinc, double* out, hipStream_t s);

// rotate_nms.hip: rotated-box NMS of n boxes dets [n][6] (x, y, x size, y size, angle, score), the m best by score:
// order [m], sorted [m][5], corners [m][9], mask [m][ceil(m / 64)] are scratch; keep [m] and *n_keep the result
void launch_rnms(const float* dets, int n, int m, float thr, int post_max, int* order, float* sorted, float* corners,
                 unsigned long long* mask, int* keep, long long* n_keep, hipStream_t s);

// soft_nms.hip: Soft-NMS of n boxes dets [n][5] (x1, y1, x2, y2, score), the m best by score (m <= PP_SNMS_MAX_BOXES):
// enter [n] and order [m] are scratch (used when m < n); keep [post_max], scores [post_max] and *n_keep the result
void launch_soft_nms(const float* dets, int n, int m, int method, float nt, float sigma, float score_floor, int post_max,
                     int* enter, int* order, int* keep, float* scores, long long* n_keep, hipStream_t s);

// box_project.hip: image boxes of n camera-frame boxes [n][7]; frame_start [frames + 1] is the exclusive prefix of the
// frames' box counts, p2 [frames][16], bbox [n][4]
void launch_box3d_to_bbox(const double* boxes, long long n, const long long* frame_start, int frames, const double* p2,
                          double* bbox, hipStream_t s);

// eval_stats.hip: the AP evaluator's greedy matching and tp / fp / fn / similarity statistics (kitti_eval.py)
struct EvalStatsParams {
    int nframes, K;            // frames; overlap tiers
    int total_gt;              // gt_off[nframes]: row length of `matched`
    const int* gt_off;         // [nframes + 1] first ground truth / detection / DontCare box of each frame
    const int* dt_off;
    const int* dc_off;         // (counting pass only)
    const long long* ov_off;   // [nframes + 1] first overlap of each frame
    const double* overlaps;    // per frame [G][D]
    const double* scores;      // [sum D]
    const int* ign_gt;         // [sum G] 0 counts, 1 neutral, -1 other class
    const int* ign_dt;         // [sum D]
    const double* min_overlaps;   // [K]
    int* matched;              // matching pass out: [K][total_gt] frame-local detection index of a true positive, or -1
    // counting pass
    const double* gt_alpha;    // [sum G]
    const double* dt_alpha;    // [sum D]
    const double* dt_box;      // [sum D][4]
    const double* dc_box;      // [sum C][4]
    const double* thresholds;  // [K][PP_EVAL_NTHRESH]
    const int* nthresh;        // [K] thresholds in use, each <= PP_EVAL_NTHRESH
    int metric, compute_aos;
    double* partial;           // [nframes][K][PP_EVAL_NTHRESH][4] tp, fp, fn, similarity of one frame (slots in use only)
    double* pr;                // out: [K][PP_EVAL_NTHRESH][4]
};
void launch_eval_match(const EvalStatsParams& p, hipStream_t s);
void launch_eval_count(const EvalStatsParams& p, hipStream_t s);
void launch_eval_reduce(const EvalStatsParams& p, hipStream_t s);   // partial -> pr, frames added in a fixed order

// targets.hip: training targets from ground-truth boxes on the device (create_target_np, load_data.py:331-532)
struct TargetParams {
    int batch;
    int64_t A;                 // anchors per frame
    const float4* anchor_near; // [A] nearest standing / lying box of every anchor (xmin, ymin, xmax, ymax)
    const float* anchors;      // [A][7]
    const uint8_t* mask;       // [batch][A] anchors kept per frame, or NULL: every anchor
    const float* gt;           // [sum counts][7] x y z w l h r, the frames' boxes back to back
    const int* gt_cls;         // [sum counts] classes 1..num_class, or NULL: all 1
    const int* gt_cnt;         // [batch] boxes per frame (<= PP_MAX_GT_PER_FRAME)
    unsigned* top;             // [batch][PP_MAX_GT_PER_FRAME] per box: its best overlap over the kept anchors (float bits,
                               // zeroed before the first pass)
    float matched, unmatched;  // thresholds (float32 compares)
    int* labels;               // [batch][A] out
    float* reg_targets;        // [batch][A][7] out
    int* gt_index;             // [batch][A] out or NULL: best box per kept anchor, -1 otherwise
    float* overlap;            // [batch][A] out or NULL: its overlap, -1 for a masked-out anchor
};
void launch_anchor_near(const float* anchors, int64_t A, float4* near, hipStream_t s);
void launch_targets(const TargetParams& p, hipStream_t s);   // pass 1 (per-box maxima) + pass 2 (labels, targets)

// augment.hip: training-time augmentation of the resident frames (augment.py)
typedef pp_aug_frame AugFrame;
struct AugBox {                // per box of a frame, written by k_aug_select for the point pass
    double n[6][3], d[6];      // plane equations of the original 3-D box (outside: p . n + d >= 0)
    double c[3];               // original centre
    double loc[3], cr, sr;     // selected transform (zero when no try passed): shift, cos / sin of the turn
    int valid;
};
struct AugParams {
    int batch, F, T, v2;
    double pc[4];              // pc_range x0 y0 x1 y1
    const int* offsets;        // [batch + 1] resident frame offsets
    const float* pts_in;       // [sum n][F] resident points
    float* pts_out;            // [sum n][F] augmented, shuffled
    const float* gt_in;        // [sum cnt_in][7]
    const int* cls_in;         // [sum cnt_in] or NULL (all 1)
    const uint8_t* valid;      // [sum cnt_in] or NULL (all valid)
    const int* cnt_in;         // [batch]
    const double* draws;       // [sum cnt_in][T][5]
    const int* draw_off;       // [batch] first draw row of each frame, or NULL: its first box's index
    const AugFrame* frames;    // [batch]
    double* frame_cs;          // [batch][2] cos / sin of the frame's global rotation (k_aug_select -> k_aug_points)
    AugBox* boxrec;            // [batch][PP_MAX_GT_PER_FRAME]
    float* box_tmp;            // [batch][PP_MAX_GT_PER_FRAME][7] augmented boxes before compaction
    uint8_t* keep;             // [batch][PP_MAX_GT_PER_FRAME]
    int* sel;                  // [sum cnt_in] selected try (-1: none), or NULL
    float* gt_out;             // [sum cnt_out][7] kept boxes, frames back to back
    int* cls_out;              // [sum cnt_out]
    int* cnt_out;              // [batch]
};
void launch_augment(const AugParams& p, int max_n, hipStream_t s);

// gt_sample.hip: GT-database sampling into the resident frames (gt_sampler.py)
struct GtsPlane { double n[6][3], d[6]; };   // a surviving candidate's 3-D box (outside: p . n + d >= 0)
struct GtsParams {
    int batch, F;
    int max_pc, min_pc;        // sampler_max_point_collision / sampler_min_point_collision
    const int* offsets;        // [batch + 1] resident frame offsets
    const float* pts_in;       // [sum n][F] resident points
    float* pts_out;            // pasted objects' points, then the frame's own, frames back to back
    int* offsets_out;          // [batch + 1]
    const float* gt_in;        // [sum cnt_in][7]
    const int* cls_in;         // [sum cnt_in] or NULL (all 1)
    const uint8_t* valid_in;   // [sum cnt_in] or NULL (all valid)
    const int* cnt_in;         // [batch]
    const pp_gts_cand* cands;  // [batch][PP_GTS_MAX_CAND] the frame's rounds back to back
    const int* cand_counts;    // [batch][PP_GTS_MAX_ROUNDS]
    const float* db_pts;       // the database: points [.][F] centred on their box,
    const int* db_off;         //   [n + 1] point offsets,
    const double* db_box;      //   [n][7] boxes,
    const int* db_cls;         //   [n] classes
    GtsPlane* planes;          // [batch][PP_GTS_MAX_CAND]
    int* status;               // [batch][PP_GTS_MAX_CAND] pp_gts_status; -1 between the kernels: survived the box test
    int* counts;               // [batch][PP_GTS_MAX_CAND] frame points inside the candidate's box
    int* round_used;           // [batch]
    int* acc_n;                // [batch] accepted objects
    int* acc_slot;             // [batch][PP_GTS_MAX_CAND] their slots, in order
    int* acc_pstart;           // [batch][PP_GTS_MAX_CAND + 1] first pasted point of each within the frame
    int* box_off;              // [2][batch + 1] scratch: first box of each frame, in and out
    float* gt_out;             // [sum cnt_out][7] the frame's boxes, then the accepted objects'
    int* cls_out;              // [sum cnt_out]
    uint8_t* valid_out;        // [sum cnt_out]
    int* cnt_out;              // [batch]
};
// select + count + decide; then paste.  max_n: the largest resident frame; max_out_n: an upper bound of the largest
// frame after pasting (both host-known)
void launch_gt_sample(const GtsParams& p, int max_n, int max_out_n, hipStream_t s);

// gt_database.hip: the labelled objects of the resident frames, cut out and centred (gt_database.py)
#define PP_GDB_CHUNK 256       // points per workgroup of the count / gather passes
struct GdbParams {
    int batch, F;
    const int* offsets;        // [batch + 1] resident frame offsets
    const float* pts;          // [sum n][F] resident points (only read)
    const double* boxes;       // [sum G][7] x y z w l h r, the frames' boxes back to back
    const int* box_cnt;        // [batch]
    const int* box_off;        // [batch + 1] first box of each frame
    GtsPlane* planes;          // [sum G]
    int* chunk_cnt;            // [batch][chunk_stride][PP_MAX_GT_PER_FRAME]: members per (chunk, box); after the scan the
    int chunk_stride;          //   chunk's base inside its object.  chunk_stride: chunks of a max_points_per_frame frame
    int* totals;               // [sum G] points per object
    long long* obj_off;        // [sum G + 1] first output row of each object
    float* out;                // [obj_off[sum G]][F]
};
// planes + count + scans (totals, obj_off, chunk bases); then the gather.  max_n: the largest resident frame
void launch_gtdb_count(const GdbParams& p, int total_boxes, int max_n, hipStream_t s);
void launch_gtdb_gather(const GdbParams& p, int max_n, hipStream_t s);

// ingest.hip: live PointCloud2 messages -> the resident float32 points and frame offsets (ingest.py)
struct IngFrame {              // one message of a call, as the kernels see it
    long long byte_off;        // its first byte within the staged bytes
    int width, n_rec;          // records per row; records in all (a frame with tight rows is handed over as one row)
    int point_step, row_step;
    int x_off, y_off, z_off;   // byte offsets of the fields within a record
    int f64, big_endian;       // FLOAT64 fields (else FLOAT32); byte order
    int nchunks;               // ingest_chunks(n_rec)
};
// One feature column (row entry 3 ... F - 1) of one message (pp_ingest_pointcloud2_fields*): the value is
// float32(float64(raw) * scale + bias), raw read at record + off; type 0 reads nothing, the value is float32(bias)
struct IngFeat {
    int off, type;             // byte offset within a record; PointField code 1 INT8 ... 8 FLOAT64, or 0: constant
    double scale, bias;
};
// ingest.hip: raw depth images (sensor_msgs/Image, 16UC1 or 32FC1) -> the same resident points and offsets
struct DepthFrame {            // one image of a call, as the kernels see it
    long long byte_off;        // its first byte within the staged bytes
    int width, n_pix;          // pixels per row (the true width: the deprojection needs row and column); pixels in all
    int row_step;              // bytes per row
    int tight;                 // pixel i sits at i * itemsize (no row padding): no division for its address
    int f32, big_endian;       // 32FC1 metres (else 16UC1 units of depth_scale); byte order
    int nchunks;               // ingest_chunks(n_pix)
    float fx, fy, ppx, ppy;    // pinhole intrinsics
    float depth_scale;         // metres per unit of a 16UC1 pixel
    float z_min, z_max;        // a pixel is valid only when z > z_min && z <= z_max
};
// ingest.hip, a rig call: several sources (cameras) per frame, each under its own selection and transform; a frame's
// points are its sources' kept points in source order, back to back.  The per-source records are IngFrame or DepthFrame.
struct RigSource {             // what a source has of its own besides its IngFrame / DepthFrame
    int frame;                 // the frame it belongs to (non-decreasing over the sources, every frame present)
    int first, decimate;
    int reserved;
    double r[9], r2[9], lift[3];
};
// One call of either feed.  A record is a frame of a plain call (records == batch, src NULL, one selection and one
// transform for all of them: first ... lift) or a source of a rig call (src: the sources' own, and the rig-only outputs).
template <typename Frame>
struct IngestParamsT {
    const uint8_t* raw;        // the records' bytes, staged on the device
    const Frame* frames;       // [records]
    const RigSource* src;      // [records], or NULL: a plain call
    int records, batch, stride;   // stride: chunks of the largest record (row length of the two chunk tables)
    int first, decimate;       // a plain call
    double r[9], r2[9], lift[3];
    int* chunk_cnt;            // [records][stride] finite records (valid pixels) per chunk
    int* chunk_base;           // [records][stride] finite records (valid pixels) of the record in front of the chunk
    int* src_finite;           // [records] out, rig only: finite records (valid pixels) of each source
    int* src_kept;             // [records] out, rig only: points written of each source
    int* out_base;             // [records] out, rig only: kept points of the earlier sources of its frame
    int* finite;               // [batch] out: finite records (valid pixels), a rig's summed over the frame's sources
    int* kept;                 // [batch] out: points written, likewise
    int* offsets;              // [batch + 1] out: the frames' row offsets in `out`
    float* out;                // [sum kept][3 + nfeat]
    long long out_rows;        // rows `out` holds
    const IngFeat* feats;      // [records][nfeat] feature columns behind x y z (PointCloud2 only), or nfeat == 0
    int nfeat;
};
int ingest_chunks(int n);      // chunks of a record of n points or pixels
void launch_ingest(const IngestParamsT<IngFrame>& p, hipStream_t s);
void launch_ingest(const IngestParamsT<DepthFrame>& p, hipStream_t s);

// frustum_crop.hip: the resident frames cropped to the camera frustum (frustum.py), frames compacted in order
struct CropParams {
    const float* in;           // [sum n_b][F] the resident points (device memory, or a zero-copy feed's page-locked block)
    const int* offsets_in;     // [batch + 1] their frame offsets
    const double* planes;      // [batch][6][4] n0 n1 n2 d per face; a point is removed iff ((x n0 + y n1) + z n2) + d >= 0 for one
    int batch, F, stride;      // stride: crop_chunks(largest frame) (row length of the two chunk tables)
    int back;                  // column 0 is negated first (tested and stored negated)
    int* chunk_cnt;            // [batch][stride] kept points per chunk
    int* chunk_base;           // [batch][stride] kept points of the frame in front of the chunk
    int* kept;                 // [batch] out: points kept
    int* offsets_out;          // [batch + 1] out: the frames' row offsets in `out`
    float* out;                // [sum kept][F]
    long long out_rows;        // rows `out` holds
};
int crop_chunks(int n);
int crop_max_features();     // widest row (num_point_features) the kernels move
void launch_frustum_crop(const CropParams& p, hipStream_t s);

// sweeps.hip: the resident frames plus their streams' stored sweeps, carried into the current sensor frame (sweeps.py)
struct SweepXf {               // p_c = M p_s + u of one used sweep, and its time lag
    double m[9], u[3];
    float dt;
    int pad;
};
struct SweepChunk {            // up to SWEEP_CHUNK rows of one segment: the current rows, a used sweep, or the ring push
    const float* src;          // first source row (rows `stride` apart)
    float* dst;                // first destination row (rows back to back)
    int rows;
    int xf;                    // >= 0: index into the transform table; SWEEP_XF_CUR: current rows; SWEEP_XF_PUSH: raw copy
    int stride;
    int pad;
};
constexpr int SWEEP_CHUNK = 256;
constexpr int SWEEP_XF_CUR = -1, SWEEP_XF_PUSH = -2;
struct SweepParams {
    const float* in;           // [sum n_b][F] the resident points (device memory, or a zero-copy feed's page-locked block)
    const int* offsets_in;     // [batch + 1] their frame offsets: DEVICE values, the host holds bounds
    float* out;                // [sum count_b][F] the other input buffer
    int* offsets_out;          // [batch + 1]
    int batch, F, nmax;        // nmax: max_points_per_frame, the cut of an output frame
    int history, capacity, decimate, time_feature;
    double max_age;
    const double* call;        // [batch][13]: the current pose (12), the current stamp
    // the streams' rings, slots = history + 1 per stream
    float* ring;               // [B][slots][capacity][F]
    int* slot_cnt;             // [B][slots] rows stored
    int* slot_valid;           // [B][slots] the slot holds a sweep
    double* slot_pose;         // [B][slots][12]
    double* slot_stamp;        // [B][slots]
    int* head;                 // [B] the slot the next call writes (the oldest sweep's)
    SweepXf* xf;               // [batch][history]
    SweepChunk* segs;          // [batch][history + 2] the frames' segments, as chunks of any length (plan scratch)
    int* seg_chunk0;           // [batch][history + 2] first chunk of each segment
    int* frame_chunks;         // [batch + 1] chunks per frame -> their exclusive scan
    SweepChunk* chunks;        // [chunk_cap] the move launch's table
    int* nchunks;              // [1] entries written
    int chunk_cap;
    int chunk_bound;           // the host's bound on *nchunks: the move launch's grid
    int *count, *used, *truncated, *push_truncated;   // [batch] pp_sweeps_info
};
int sweep_chunks(int n);       // chunks of a segment of n rows
void launch_sweeps(const SweepParams& p, hipStream_t s);

// costmap.hip: the resident points, the last pass's detections or the streams' tracks -> one int8 grid per frame
// (pp_set_costmap; costmap.py states the rule).  One footprint of a frame's table, with a conservative cell box:
struct CmFootprint {
    double ox, oy, c, s, hx, hy;
    int cost;
    int ix0, ix1, iy0, iy1;        // no cell outside the box has its centre in the rectangle (an empty box: ix0 > ix1)
    int pad;
};
#define PP_CM_TRACK_ROWS (PP_TRACK_MAX * (1 + PP_COSTMAP_MAX_STEPS))   // footprints of a stream's tracks at most
struct CostmapParams {
    pp_costmap_config cfg;
    int batch, F;
    int pitch;                     // cells of a row in words / grid / tap: width rounded up to 4
    int max_n;                     // the host's bound on the rows of a frame
    const float* points;           // the resident rows [.][F]
    const int* offsets;            // [batch + 1] device values
    const pp_detection* dets;      // objects = detections: [batch][det_rows]
    const int* n_dets;             // [batch], PP_NDETS_NONFINITE: the frame takes no objects
    int det_rows;
    const TrkSlot* slots;          // objects = tracks: [B][PP_TRACK_MAX]
    CmFootprint* table;            // [batch][table_rows], the frame's footprints compacted in source order
    int table_rows;
    int* n_fp;                     // [batch] footprints written
    int* flagged;                  // [batch] 1: the frame's detections were flagged non-finite
    int* in_grid;                  // [batch] points inside the grid (cleared with the words)
    unsigned* words;               // [batch][height * pitch]: bits 0..30 the count, bit 31 observed without a count
    int8_t* grid;                  // [batch][height * pitch]
    int* tap;                      // [batch][height * pitch] the counts
    const unsigned long long* mask;    // the object mask's words [batch][mask_stride], or NULL: no row is masked
    int mask_stride;
    const unsigned long long* gnd;     // the ground stage's GROUND and OBSTACLE words [batch][cls_stride] each, or both NULL:
    const unsigned long long* obs;     // the fixed z band decides
    int cls_stride;
};
void launch_costmap(const CostmapParams& p, hipStream_t s);

// occupancy.hip: the resident points under a pose per stream -> the stream's rolling log-odds window and its int8 grid
// (pp_set_occupancy; occupancy.py states the rule).  What one stream of a call needs, read from a device buffer:
struct OccCall {
    double r0[3], tx;              // row 0 of the pose [R | t]
    double r1[3], ty;              // row 1
    int ox, oy;                    // the new window's origin, global cell indices
    int sdx, sdy;                  // a cell of the new window was cell (ix + sdx, iy + sdy) of the old one
    int fresh;                     // 1: nothing of an old window is kept (none yet, a reset, a jump past the window)
    int src;                       // which of the two state copies holds the old window; the new one goes to 1 - src
    int pad[2];
};
#define PP_OCC_HIT 1u              // mark bits of an end cell of a frame
#define PP_OCC_GROUND 2u
#define PP_OCC_MASKED 4u           // ... of a row in the hit band that the object mask names: the cell's ray, and no hit
#define PP_OCC_INFO 8              // int32 per stream: hits, ground, ignored, cells_hit, cells_free, listed cells, masked rows, 1 spare
struct OccParams {
    pp_occupancy_config cfg;
    int batch, F;
    int pitch;                     // cells of a row in every buffer below: width rounded up to 4
    int max_n;                     // the host's bound on the rows of a frame
    int list_cap;                  // entries of a stream's list
    const float* points;           // the resident rows [.][F]
    const int* offsets;            // [batch + 1] device values
    const OccCall* call;           // [batch]
    unsigned* marks;               // [batch][height * pitch] the end cells' bits, cleared before the launches
    unsigned char* passed;         // [batch][height * pitch] 1: a ray crossed the cell; cleared likewise
    int* list;                     // [batch][list_cap]: the cells that took an endpoint, each once, in no fixed order
    int* info;                     // [batch][PP_OCC_INFO], cleared before the launches
    int16_t* logodds[2];           // [B][height * pitch] each: the two state copies
    int8_t* grid[2];               // [B][height * pitch] each; -1 is also the state's "not known"
    const int8_t* table;           // [l_max - l_min + 1]
    const unsigned long long* mask;    // the object mask's words [batch][mask_stride], or NULL: no row is masked
    int mask_stride;
    const unsigned long long* gnd;     // the ground stage's GROUND and OBSTACLE words [batch][cls_stride] each, or both NULL:
    const unsigned long long* obs;     // the fixed z band decides
    int cls_stride;
};
void launch_occupancy(const OccParams& p, hipStream_t s);

// inflate.hip: int8 OccupancyGrids -> the grids with every obstacle grown by the robot's radius and a falling cost beyond
// it (pp_set_inflation, pp_inflate_grids; inflation.py states the rule)
struct InflParams {
    int batch, width, height;
    int R;                         // the inflation radius in cells, <= PP_INFLATE_MAX_RADIUS
    int lethal, unknown_min;       // pp_inflation_config's lethal_threshold, unknown_min_cost
    int in_pitch, out_pitch;       // cells of a row of `in`, and of `out` and `dist2`
    size_t in_stride, out_stride;  // cells from one grid to the next
    const int8_t* in[2];           // [batch][height * in_pitch]; read, never written
    const OccCall* occ_call;       // NULL: every grid is in[0]'s.  Else [batch], the records of the occupancy update that
                                   // wrote the grids: stream b's lies in in[1 - occ_call[b].src]
    const int8_t* table;           // [R * R + 1] the cost by squared cell distance
    int8_t* out;                   // [batch][height * out_pitch]
    uint16_t* dist2;               // the same shape, or NULL: the squared distance, R * R + 1 where nothing is in reach
    int* counts;                   // [batch][2]: obstacle cells, cells with out != in; cleared before the launch
};
void launch_inflate(const InflParams& p, hipStream_t s);

// navfn.hip: int8 OccupancyGrids and one goal cell each -> the cost-to-go field and the path from a start cell
// (pp_set_navfn, pp_navfn_grids; navfn.py states the rule)
struct NavCall {                   // what travels from the host per grid and call
    int gx, gy, sx, sy;            // the goal and the start, cells
    int flags;                     // NAV_HAS_START; NAV_KNOWN (clear: the grid reads all unknown, whatever it holds)
};
constexpr int NAV_HAS_START = 1, NAV_KNOWN = 2;
// per grid, field-major int [NAV_STATE][state_stride]: the three `changed` slots rotate by round index
enum { NAV_CHANGED = 0, NAV_ROUNDS = 3, NAV_REACHED = 4, NAV_GOAL_STATE = 5, NAV_PATH_STATE = 6, NAV_PATH_LEN = 7, NAV_STATE = 8 };
struct NavParams {
    int batch, width, height;
    int pitch;                     // cells of a row of `grid`, `cost` and both `pot`
    size_t stride;                 // cells from one grid to the next in all of them
    int lethal, neutral, factor, allow_unknown, unknown_cost, conn, max_path;     // pp_navfn_config
    const int8_t* grid;            // [batch][height * pitch]; read, never written
    const NavCall* call;           // [batch]
    uint16_t* cost;                // [batch][height * pitch], 0: blocked
    unsigned* pot[2];              // the same shape: round r reads pot[r & 1] and writes pot[(r + 1) & 1]
    int* state;                    // [NAV_STATE][state_stride]
    int state_stride;
    int* paths;                    // [batch][max_path][2]
};
void launch_navfn_init(const NavParams& p, hipStream_t s);
void launch_navfn_relax(const NavParams& p, int round, hipStream_t s);       // `round` counts from 0 behind the init
void launch_navfn_finish(const NavParams& p, int rounds, hipStream_t s);     // after `rounds` rounds; NAV_REACHED cleared before it
int navfn_tiles(int width, int height, int* tiles_x);                        // workgroups of a round per grid

// local_plan.hip: the inflated grid, the field and one pose and window per grid -> the (v, w) command whose rollout scores
// least (pp_set_local_plan, pp_local_plan_grids; local_planner.py states the rule)
struct LocalCall {                 // what travels from the host per grid and call: 8 int32
    int X, Y, h;                   // the pose: sub-cells and a heading tick (taken & 4095)
    int v0, dv, w0, dw;            // the window: sample s = i * nw + j has sv = v0 + i * dv, sw = w0 + j * dw
    int flags;                     // LOC_NO_GOAL: the field has no goal, whatever `nav_state` says (pp_local_plan_grids)
};
constexpr int LOC_NO_GOAL = 1;
constexpr int LOC_BLOCK = 256;     // samples of a workgroup of the rollout
constexpr int LOC_MAX_CHUNKS = PP_LOCAL_MAX_SAMPLES / LOC_BLOCK;
// per grid, field-major int [LOC_STATE][state_stride]: the four reason counts are cleared before the rollout and added to by
// it; the others are written by finish.  The first PP_LOCAL_RESULT fields are a grid's result words in their order.
enum { LOC_CMD_STATE = 0, LOC_BEST = 1, LOC_SV = 2, LOC_SW = 3, LOC_N_OK = 4, LOC_N_OUTSIDE = 5, LOC_N_COLLISION = 6,
       LOC_N_UNREACHED = 7, LOC_STATE = 8 };
struct LocalParams {
    int batch, width, height;
    int pitch;                     // cells of a row of `grid` and `pot`
    size_t stride;                 // cells from one grid to the next in both
    int lethal, allow_unknown, unknown_cost;       // of the pp_navfn_config the field was made with
    int nv, nw, steps, lookahead, pot_w, occ_w, speed_w, turn_w;     // pp_local_plan_config
    const int8_t* grid;            // [batch][height * pitch]; read, never written
    const unsigned* pot;           // the same shape; read, never written
    const NavCall* nav_call;       // [batch] or NULL: NAV_KNOWN clear reads the grid all unknown
    const int* nav_state;          // [NAV_STATE][nav_state_stride] or NULL: NAV_GOAL_STATE != 0 is "no goal"
    int nav_state_stride;
    const LocalCall* call;         // [batch]
    const unsigned* trig;          // [PP_LOCAL_HEADINGS]: C[h] as int16 in the low half, S[h] in the high half
    unsigned long long* partial;   // [batch][LOC_MAX_CHUNKS]: a workgroup's least key (with a footprint: the least key of a
                                   // chunk of LOC_BLOCK samples, all ones before the rollout, whose workgroups lower it)
    int* state;                    // [LOC_STATE][state_stride]
    int state_stride;
    unsigned long long* score;     // [batch]
    int* traj;                     // [batch][steps + 1][3]
    unsigned long long* keys;      // [batch][nv * nw], or NULL: not stored
    // the movers (pp_local_plan_movers_async, pp_local_plan_grids_movers); NULL: none, and the kernels' instantiations
    // without them run, which read nothing below
    const int* movers;             // [batch][PP_LOCAL_MAX_MOVERS][6]: mx, my, mvx, mvy, r_hard, r_soft
    int* mover_info;               // [PP_LOCAL_MOVER_INFO][state_stride], as LOC_M_* names the fields
    int horizon, mover_w;          // pp_local_mover_config
    // the footprint (pp_set_local_footprint, pp_local_plan_grids_footprint); NULL: a point, and the kernels'
    // instantiations without it run, which read nothing below
    const unsigned* probes;        // [n_probes]: fx as int16 in the low half, fy in the high half; one table for every grid
    int n_probes, foot_lethal;     // 1 .. PP_LOCAL_MAX_PROBES; pp_local_footprint_config
    int* foot_info;                // [PP_LOCAL_FOOT_INFO][state_stride], as LOC_F_* names the fields
};
// n_movers (-1: the stream has had no posed step; rolled as 0) and n_skipped are written by k_local_movers or the host,
// n_dynamic is cleared before the rollout and added to by it, near is written by finish
enum { LOC_M_COUNT = 0, LOC_M_SKIPPED = 1, LOC_M_DYNAMIC = 2, LOC_M_NEAR = 3 };
// n_footprint is cleared before the rollout and added to by it; the others are written by finish
enum { LOC_F_COUNT = 0, LOC_F_FOOTPRINT = 1, LOC_F_START = 2, LOC_F_RESERVED = 3 };
// The footprint rollout gives every sample a group of LOC_FOOT_GROUP lanes of one wave, lane j of which takes the probes
// q = j (mod LOC_FOOT_GROUP); a workgroup then rolls LOC_BLOCK / LOC_FOOT_GROUP samples.  Chosen by measurement among 1,
// 8, 16 and 64.
constexpr int LOC_FOOT_GROUP = 64;
void launch_local_rollout(const LocalParams& p, hipStream_t s);     // the reason counts of `state` cleared before it
void launch_local_finish(const LocalParams& p, hipStream_t s);
struct LocalFrame {                // what travels from the host per grid and pp_local_plan_movers_async: 4 doubles
    double ox, oy, res, dt;        // the metres of cell [0, 0]'s corner and of a cell, the seconds of a step
};
struct LocalMoverParams {
    int batch;
    int fixed;                     // 1: the slots are carried into the fixed frame with pose_prev (the occupancy source)
    int confirmed_only;
    double pad_hard, pad_soft;
    const TrkSlot* slots;          // [B][PP_TRACK_MAX]
    const TrkPose* pose_prev;      // [B]
    const LocalFrame* frame;       // [batch]
    int* movers;                   // [batch][PP_LOCAL_MAX_MOVERS][6]; zeros behind a grid's movers
    int* mover_info;               // [PP_LOCAL_MOVER_INFO][info_stride]: writes LOC_M_COUNT and LOC_M_SKIPPED
    int info_stride;
};
void launch_local_movers(const LocalMoverParams& p, hipStream_t s);

// scan_match.hip: the resident points under a prior pose per stream, matched against the stream's log-odds window
// (pp_set_scan_match, pp_scan_match_grids; scan_match.py states the rule)
struct ScanCall {                  // what travels from the host per stream and call: 6 doubles, 4 int32
    double r0[3], r1[3];           // rows 0 and 1 of the prior's rotation
    int sx, sy;                    // the sensor in sub-cells of the stream's window (0 where flags are set)
    int flags;                     // PP_SCAN_NO_MAP | PP_SCAN_OUTSIDE: nothing is scored
    int src;                       // which of the two log-odds copies holds the stream's map
};
constexpr int SCAN_TILE = 64;      // translation candidates of a workgroup of k_scan_scores: one per lane of a wave
constexpr int SCAN_INFO = 4;       // int32 per stream in front of the marks: rows used, rows ignored, scan cells, spare
struct ScanParams {
    pp_occupancy_config occ;       // resolution, z_min, z_max, max_range, width, height
    pp_scan_match_config cfg;
    int batch, F;
    int pitch;                     // cells of a row of the log-odds
    size_t map_stride;             // cells from one stream's log-odds to the next
    int max_n;                     // the host's bound on the rows of a frame
    int list_cap;                  // entries of a stream's list
    int mark_words;                // 32-bit words of a stream's marks: a bit per cell of width * height
    int n_trans, tiles;            // (2 nx + 1)(2 ny + 1), and the workgroups of a heading that cover them
    const float* points;           // the resident rows [.][F]
    const int* offsets;            // [batch + 1] device values
    const ScanCall* call;          // [batch]
    const unsigned* trig;          // [PP_LOCAL_HEADINGS]: C[h] as int16 in the low half, S[h] in the high half
    const int16_t* logodds[2];     // [.][map_stride] each; stream b's lies in logodds[call[b].src]; 0 where not known
    int* info;                     // [batch][SCAN_INFO], cleared with the marks before the launches
    unsigned* marks;               // [batch][mark_words], cleared before the launches
    int2* list;                    // [batch][list_cap]: (ux, uy) of every scan cell, each once, in no fixed order
    int* scores;                   // [batch][candidates]
    unsigned long long* partial;   // [batch][(2 nt + 1) * tiles]: a workgroup's least key
    int* words;                    // [batch][PP_SCAN_RESULT]
    const unsigned long long* mask;    // the object mask's words [batch][mask_stride], or NULL: no row is masked
    int mask_stride;
    const unsigned long long* gnd;     // the ground stage's GROUND and OBSTACLE words [batch][cls_stride] each, or both NULL:
    const unsigned long long* obs;     // the fixed z band decides
    int cls_stride;
};
void launch_scan_match(const ScanParams& p, hipStream_t s);         // info and marks cleared before it

// object_mask.hip: per resident row, "this return lies in the BEV rectangle of an object" (pp_set_object_mask,
// pp_object_mask_points; object_mask.py states the rule).  One footprint of a frame's table, with a conservative float32
// box for the rows' pretest: 64 bytes, read by every lane of a wave at one LDS address (a broadcast)
struct OmFootprint {
    double ox, oy, c, s, hx, hy;
    float xlo, xhi, ylo, yhi;      // no row outside the box lies in the rectangle (an empty box: xlo > xhi)
};
struct OmCall {                    // what travels from the host per stream and call: 14 doubles, 2 int32
    double m[12];                  // the pose [R | t] the slots' copies are carried into
    double psi;                    // atan2(R10, R00), from the host
    double dt;                     // seconds the copies are predicted by
    int has_pose, has_dt;
};
enum { OM_DETECTIONS = 1, OM_TRACKS = 2, OM_GIVEN = 3 };      // OmParams::objects (1, 2: pp_object_mask_config's)
struct OmParams {
    pp_object_mask_config cfg;     // (OM_GIVEN reads pad alone)
    int objects;
    int batch, F;
    int max_n;                     // the host's bound on the rows of a frame
    const float* points;           // the resident rows [.][F]
    const int* offsets;            // [batch + 1] device values
    const pp_detection* dets;      // OM_DETECTIONS: [batch][det_rows]
    const int* n_dets;             // [batch], PP_NDETS_NONFINITE: the frame takes no objects
    int det_rows;
    const TrkSlot* slots;          // OM_TRACKS: [B][PP_TRACK_MAX], read and never written
    const TrkPose* pose_prev;      // [B] the tracker's record of the stream's last posed step
    const OmCall* call;            // [batch], or NULL: the slots as they stand
    const double* given;           // OM_GIVEN: [.][5] x y w l yaw, frame b's rows from given_off[b]
    const int* given_off;          // [batch + 1]
    OmFootprint* table;            // [batch][PP_OBJMASK_MAX_FOOTPRINTS], compacted in source order
    int* info;                     // [batch][PP_OBJMASK_INFO]
    unsigned long long* words;     // [batch][stride]; every run writes words 0 .. 4 * ceil(max_n / 256) - 1 of a frame
    int stride;
};
void launch_object_mask(const OmParams& p, hipStream_t s);

// ground.hip: per resident frame one plane z = a x + b y + c by RANSAC, per row a class from its vertical residual
// (pp_set_ground, pp_ground_points; ground.py states the rule and the order of every operation).  One hypothesis of a
// frame's table: 32 bytes, read by every lane of a wave at one LDS address (a broadcast)
struct GrHyp {
    double a, b, c;
    int valid, pad;                // pad: the record's k
};
struct GrParams {
    pp_ground_config cfg;
    int batch, F;
    int max_n;                     // the host's bound on the rows of a frame
    int K;                         // cfg.hypotheses
    const float* points;           // the resident rows [.][F]
    const int* offsets;            // [batch + 1] device values
    const unsigned* triples;       // [batch][K][3]
    GrHyp* hyp;                    // [batch][K]
    GrHyp* chyp;                   // [batch][K]: the valid records of a frame in order of k, back to back, k in `pad`; info[4] of them
    int* counts;                   // [batch][K]
    long long* sums;               // [batch][PP_GROUND_SUMS]
    double* plane;                 // [batch][3]: the winner's (or the fallback) plane after the pick, the final one after the refit
    int* info;                     // [batch][PP_GROUND_INFO]
    unsigned long long* gnd;       // [batch][stride]; every run writes words 0 .. 4 * ceil(max_n / 256) - 1 of a frame
    unsigned long long* obs;       // [batch][stride]
    int stride;
};
void launch_ground(const GrParams& p, hipStream_t s);
int ground_launches(const GrParams& p);      // the launches launch_ground queues

// frontier.hip: int8 OccupancyGrids -> the clusters of their frontier cells, ranked (pp_set_frontier, pp_frontier_grids;
// frontier.py states the rule)
struct FrontierCall {              // what travels from the host per grid and call: 4 int32
    int rx, ry;                    // the reference cell (read while use_field is 0)
    int flags;                     // FRONTIER_KNOWN (clear: the grid reads all unknown, whatever it holds)
    int pad;
};
constexpr int FRONTIER_KNOWN = 1;
// per grid int [FR_INFO_WORDS]: the first PP_FRONTIER_INFO are a grid's info words in their order; FR_CELLS, FR_CLUSTERS
// and FR_OVERRUN are cleared before the launches and added to by them, the others are written by select
enum { FR_CELLS = 0, FR_CLUSTERS = 1, FR_SMALL = 2, FR_UNREACHED = 3, FR_KEPT = 4, FR_RETURNED = 5, FR_OVERRUN = 6, FR_INFO_WORDS = 8 };
struct FrontierParams {
    int batch, width, height;
    int pitch;                     // cells of a row of `grid`
    size_t stride;                 // cells from one grid to the next in `grid`
    int free_max, conn, min_size, max_frontiers, rank, use_field;     // pp_frontier_config
    const int8_t* grid;            // [batch][height * pitch]; read, never written
    const FrontierCall* call;      // [batch]
    const unsigned* pot;           // use_field: [batch][height * pot_pitch], read by select only; else NULL
    int pot_pitch;
    size_t pot_stride;
    // rows of `width` cells, width * height cells from one grid to the next, in everything below
    unsigned* labels;              // [batch][height * width]: the parent of a frontier cell (its root behind stats), NONE elsewhere
    unsigned* count;               // the same shape: n at a root
    unsigned long long* sums;      // [batch][height * width][2]: sx, sy at a root
    unsigned long long* rep;       // [batch][height * width]: the least representative key at a root
    unsigned* roots;               // [batch][height * width]: the roots, each once, in no fixed order (FR_CLUSTERS of them)
    int* info;                     // [batch][FR_INFO_WORDS]
    int* words;                    // [batch][PP_FRONTIER_MAX][8]
};
void launch_frontier(const FrontierParams& p, hipStream_t s);           // mark, label, stats, rep, select; info cleared before it
void launch_frontier_select(const FrontierParams& p, hipStream_t s);    // the ranking alone, on another field

// weight_publish.hip: the trainer's flat parameter / state buffers -> the detector's weight arrays, on the device
enum PubKind {
    PUB_PFN_W,       // out [FA][cout] = params[src] * scale[c]
    PUB_SHIFT,       // out [n] = beta - mean * scale
    PUB_COPY,        // out [n] = params[src]
    PUB_SEP_WT,      // out [cout][cin] = params[src] ([cin][cout]) * scale[co]
    PUB_DEC_WT,      // out [n_total][cin] = params[src] * scale[n % cout]
    PUB_HEAD_WT,     // out [PP_HEAD_COLS][cout] = columns co_off .. co_off + cout of the head matrix
    PUB_HEAD_BIAS,   // out [PP_HEAD_COLS]
    PUB_SPLIT,       // out16 [cin / 16][PP_NPIECE][n_total][16] = float16 pieces of wt [n_total][cin]
    PUB_SPLIT_HEAD   // ... of a head slice, its channels in the deconv kernels' accumulator-register order
};
struct PubTask {
    int kind;
    int n;                      // threads: output elements (fold kinds), 16-channel groups (split kinds)
    int block0;                 // first workgroup of the task within its launch
    int cin, cout, n_total;
    int co_off;                 // PUB_HEAD_WT
    int flag;                   // split kinds: the range flag the task raises
    long long src;              // offsets (floats) into the parameter buffer ...
    long long gamma, beta;
    long long mean, var;        // ... and into the state buffer
    float* out;
    const float* wt;            // split kinds: the folded float32 array (written by the fold launch in front)
    unsigned short* out16;
};
struct PubHead {                // the three head kernels [CC][n*] and biases in the parameter buffer
    long long box_k, box_b, cls_k, cls_b, dir_k, dir_b;
    int nb, nc, nd;
};
int publish_blocks(int n);     // workgroups of a task of n threads
void launch_publish_fold(const PubTask* tasks, int ntasks, int blocks, const PubHead& hd, const float* params,
                         const float* state, hipStream_t s);
void launch_publish_split(const PubTask* tasks, int ntasks, int blocks, int* flags, hipStream_t s);
