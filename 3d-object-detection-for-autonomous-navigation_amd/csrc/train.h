// Training step (train.hip): shapes, the flat parameter layout and the device buffers api_train.hip hands over.
#pragma once

#include <string>
#include <utility>
#include <vector>

#include "pp_common.h"
#include "pp_switches.h"

struct TrainEntry {
    std::string name;    // Keras tensor name (weights.py), e.g. "rpn/block2/3/pointwise_kernel"
    int64_t offset;      // floats from the start of the parameter (or state) buffer
    int64_t size;
    int is_state;        // 1: BatchNorm moving statistic (not trained; its own buffer)
};

struct TrainShape {
    int nx, ny, nz, C, F, FA, T, max_voxels, with_dist;
    float vx, vy, x_off, y_off;
    int head_h, head_w, napl, ncls, use_dir, CC;
    std::vector<LayerDesc> layers;   // the engine's layer table (shapes only are read)
};

// One trainable layer of the plan (train_plan): the separable layers and transposed convolutions in table order -- the
// numbering of pp_train_fetch_decisions.  Tensor offsets are floats into the params / grads buffers (moving statistics:
// the state buffer), resolved once from the layout.
struct TrainLayer {
    int kind;                 // LAYER_SEP or LAYER_DECONV
    int block, index;         // block (0-based) and index in the block (separable layers)
    int layer;                // index in TrainShape::layers
    int64_t dw, pw;           // depthwise and pointwise kernels (transposed convolution: pw = its kernel; dw unused)
    int64_t gamma, beta, mean, var;
    int src;                  // the layer whose output this one reads (-1: the canvas); its input gradient goes to that
                              // layer's dA (the canvas's: dcanvas)
    bool src_z;               // src's output is its pre-BatchNorm map Z read through its coef table (src keeps no A)
    bool keeps_a;             // the activation A is a tensor (the layer in front of a transposed convolution)
    bool accumulate;          // transposed convolution: its input gradient is added to src's dA (the next block's first
                              // layer wrote it first)
    int cat_off;              // transposed convolution: its channels in the concatenation
    long pw16_off;            // offset (16-bit words) of its split forward kernel in TrainCtx::pw16
    std::string fused_tag, fwd_tag, pair_tag;   // profiler names: k_sep_u_tr:block1.0, k_tr_gemm2:fwd.block1.0, ...
    std::string dgrad_tag, wgrad_tag;           // ... the input- / weight-gradient product alone (frozen layers and
                                                // layers with nothing trainable upstream): k_tr_gemm2:dgrad.block2.0
    // freeze (train_plan_freeze): a frozen layer's BatchNorm runs on its moving statistics, and none of its tensors gets
    // a gradient; the gradient still passes through it to trainable layers upstream
    bool frozen = false;
    bool needs_dx = true;     // a trainable unit lies upstream of this layer's input: its input gradient is wanted
    bool needs_bwd = true;    // frozen == false or needs_dx: the layer has a backward step at all
};

// Built once per handle from the shape and the engine's maximum batch: the layout, the layers, and the buffer sizes
// the step's rules need.  `unsupported`: the step refuses the configuration (pp_train_layout still works).
struct TrainPlan {
    std::vector<TrainEntry> layout;
    int64_t n_params = 0, n_state = 0;
    std::vector<TrainLayer> layers;
    int64_t pfn_w = 0, pfn_gamma = 0, pfn_beta = 0, pfn_mean = 0, pfn_var = 0;
    int64_t box_k = 0, box_b = 0, cls_k = 0, cls_b = 0, dir_k = 0, dir_b = 0;   // without a direction head: dir = box
    bool unsupported = false;
    // freeze units (train_plan_freeze): "pfn", "rpn/block<b>/<j>", "rpn/deconv<b>", "rpn/conv_box", "rpn/conv_cls",
    // "rpn/conv_dir_cls"; frozen[u] per unit, in that order (the graph key of pp_train_step)
    std::vector<std::string> units;
    std::vector<unsigned char> frozen;
    bool any_frozen = false;
    bool pfn_frozen = false;
    bool head_frozen[3] = {false, false, false};        // box, cls, dir
    bool heads_wgrad = true;  // some head is trainable
    bool heads_dgrad = true;  // some layer in front of the heads has a backward step (dcat is wanted)
    std::vector<std::pair<int64_t, int64_t>> frozen_params;   // (offset, size) ranges of frozen parameters, merged
    bool fused = false;       // the fused forward kernels are available (the split-weight table holds every layer)
    long pw16_words = 0;
    size_t max_z = 1, max_d = 1, part_floats = 0;
    long stat_part_floats = 1;
    // a fused or product forward of `rows` x `n` leaves its statistics partials in TrainCtx::stat_part
    bool stat_room(long rows, long n) const { return ((rows + 127) / 128 + 8) * (2 * n + 1) <= stat_part_floats; }
};

struct TrainLayerBuf {   // per plan layer
    float* D;       // depthwise output [rows][cin] (separable layers)
    float* Z;       // pre-BatchNorm GEMM output [rows][cout] / [pixels][k*k*cout]
    float* A;       // activation [rows][cout] where TrainLayer::keeps_a (in-block readers evaluate relu(bn(Z)) from Z and
                    // coef); NULL otherwise
    float* dA;      // gradient of A (separable layers)
    float* stats;   // [cout][2] batch mean, 1/sqrt(var + eps)
    float* sums;    // [2][cout] scratch of the reductions
    float4* coef;   // [cout] (sc, sh, inv, -mean * inv): act = z * sc + sh, zhat = z * inv + nmi (k_tr_bn_finalize)
};

struct TrainCtx {
    hipStream_t stream;
    // what the step's choices depend on besides the shapes, from the handle's PlanEnv: the compute units (persistent
    // grids of the fused forward launches) and the PP_TRAIN_* switches (pp_switches.h)
    int cus = 256;
    TrainSwitches sw;
    // voxeliser products of the resident frames
    const float* pts_sorted;
    const int* offsets;
    const int* pillar_start;
    const int* pillar_cell;
    const int* npillars;
    const int* cellmap;
    // PFN
    float* pfn_feat;     // [B * max_voxels][C]
    int* pfn_arg;        // [B * max_voxels][C]
    float* pfn_stats;    // [C][2]
    float* pfn_sums;     // [2][C]
    float* pfn_nrows;    // [1] rows of the padded PFN tensor (pillars of the batch * T), computed on the device
    int* pfn_prefix;     // [B + 1] exclusive prefix of the frames' pillar counts
    float4* pfn_rec;     // [B * max_voxels][3] pillar records (row range, slot, canvas row | mean, centre): written by k_tr_pfn_lin
    float* canvas;       // [B][ny][nx][C]
    float* dcanvas;
    // RPN
    std::vector<TrainLayerBuf> lbuf;   // per TrainPlan::layers entry
    float* cat;          // [B * H' * W'][CC]
    float* dcat;
    float* head;         // [B * H' * W'][32] (the loss kernel's layout)
    float* dhead;
    float* head_w;       // [CC][32] packed head kernels
    float* head_b;       // [32]
    float* dhead_w;
    float* dhead_b;      // [2][32] scratch (row 0 = the bias gradient)
    float* dZ;           // scratch [max rows * cout]
    float* dD;           // scratch [max rows * cin]
    float* part;         // partial sums of the persistent reductions
    float* stat_part;    // BatchNorm statistics partials of the forward products: [row tiles][2][GEMM columns]
                         // (TrainPlan::stat_part_floats)
    float* gemm_part;    // split-K partial tiles
    long gemm_part_floats;
    // fused training forward of the separable layers (k_sep_u<..., TR = 1>): every pointwise kernel of the step as two
    // float16 pieces, [cin / 16][2][cout][16] per layer (k_tr_split_pw, once per step).  The maps those launches read
    // (canvas, Z of in-block layers, A of block-final ones) carry a NaN header in front.
    unsigned short* pw16;
    unsigned short* head_w16;   // the packed head matrix [CC][32] in the same form
    // pp_set_train_metrics: launched right behind the loss on the step's head map and labels (NULL: off, nothing added)
    const MetricsParams* metrics = nullptr;
};

TrainPlan train_plan(const TrainShape& s, int max_batch);
// Freeze the named units (none: train everything).  PP_ERR_ARG for an unknown or repeated name, or when nothing would be
// left to train; the plan is unchanged then.
int train_plan_freeze(TrainPlan& plan, const std::vector<std::string>& units);
// forward (training mode) + loss + backward for `batch` resident, voxelised frames; grads overwritten, state updated
int train_step(const TrainCtx& cx, const TrainShape& s, const TrainPlan& plan, const float* params, float* grads,
               float* state, int batch, const LossParams& loss, int phase = 3);

// parity tap (pp_train_fetch_decisions): mask[i] = 1 where the backward pass lets the gradient through element i of
// Z[n] ([rows][C]; the test the BatchNorm-backward kernels make: fmaf(z, sc, sh) > 0)
void launch_relu_mask(const float* Z, const float4* coef, long n, int C, unsigned char* mask, hipStream_t s);
