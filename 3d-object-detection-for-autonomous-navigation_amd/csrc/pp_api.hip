// C-ABI of libpp_hip.so (include/pp_hip.h): engine lifetime, weight folding, device workspaces, feeds and uploads,
// the inference pipeline, the stage calls and the measurement hooks -- and the resident frames' state transitions the
// other host units (pp_engine.h) go through.  Host side only; the kernels live in voxelize.hip / pfn.hip /
// anchor_mask.hip / backbone.hip / postprocess.hip.  Everything runs on one HIP stream owned by the handle.
#include <mutex>
#include <stdarg.h>

#include "pp_engine.h"

// The switch table (pp_switches.h): the one place in csrc/ that reads the environment.  Each switch parses as it always
// has (INTEGRATION.md section 5 states the values).
PpSwitches pp_parse_switches() {
    PpSwitches v;
    if (const char* e = getenv("PP_GEMM_PREC")) v.gemm_f32 = e[0] == 'f';
    if (const char* e = getenv("PP_SEP_KERNEL")) v.sep_ws = e[0] == 'w';
    if (const char* e = getenv("PP_SEP_NT")) v.sep_nt = atoi(e);
    if (const char* e = getenv("PP_SEP_K4")) v.sep_k4 = atoi(e);
    if (const char* e = getenv("PP_DECONV_K4")) v.deconv_k4 = atoi(e);
    if (const char* e = getenv("PP_PFN_KERNEL")) v.pfn_first_generation = e[0] == '1';
    if (const char* e = getenv("PP_DENSE_CANVAS")) v.dense_canvas = e[0] == '1';
    if (const char* e = getenv("PP_NO_GRAPH")) v.no_graph = e[0] == '1';
    v.no_head_fusion = getenv("PP_NO_HEAD_FUSION") != nullptr;
    TrainSwitches& t = v.train;
    if (const char* e = getenv("PP_TRAIN_FUSED_MIN")) t.fused_min = atol(e);
    if (const char* e = getenv("PP_TRAIN_GEMM")) t.split_gemm = e[0] != 'f';
    if (const char* e = getenv("PP_TRAIN_FIN_THR")) {
        long a = 0, b = 0;
        if (sscanf(e, "%ld,%ld", &a, &b) == 2 && a > 0 && b > 0) { t.fin256 = a; t.fin64 = b; }
    }
    if (const char* e = getenv("PP_TRAIN_ARENA_FLOATS")) t.arena_floats = std::max(0l, atol(e));
    return v;
}
const PpSwitches& pp_switches() {
    static const PpSwitches sw = pp_parse_switches();
    return sw;
}

static std::string g_create_error;

thread_local PpProf g_pp_prof = {nullptr, nullptr};

int fail(pp_engine* e, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (e) e->err = buf; else g_create_error = buf;
    return code;
}

int check_device(const char* who, int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, PP_ERR_HIP, "%s: no HIP device available (this library has no CPU fallback)", who);
    if (device < 0 || device >= ndev) return fail(nullptr, PP_ERR_ARG, "%s: device %d not in [0,%d)", who, device, ndev);
    return PP_OK;
}

int prof_event(pp_engine* e) {
    if (e->ev_used == (int)e->events.size()) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return -1;
        e->events.push_back(ev);
    }
    return e->ev_used++;
}

bool pp_prof_events(const char* name, hipEvent_t* start, hipEvent_t* stop) {
    pp_engine* e = g_pp_prof.e;
    if (e == nullptr || e->prof <= 0) return false;
    const int e0 = prof_event(e), e1 = prof_event(e);
    if (e0 < 0 || e1 < 0) return false;
    e->ktimes.push_back({g_pp_prof.tag ? g_pp_prof.tag : name, e0});
    *start = e->events[e0];
    *stop = e->events[e1];
    return true;
}

namespace {

// process-wide upload stream of a device (created on first use, lives as long as the process)
hipStream_t device_copy_stream(int device) {
    static std::mutex mu;
    static std::map<int, hipStream_t> streams;
    std::lock_guard<std::mutex> lock(mu);
    auto it = streams.find(device);
    if (it != streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    streams[device] = s;
    return s;
}

int bits_ok(const pp_config& c) {
    for (int j = 0; j < 3; ++j)
        if (!(c.voxel_size[j] > 0.0) || !(c.pc_range[3 + j] > c.pc_range[j])) return 0;
    return 1;
}

const char* kBn[4] = {"gamma", "beta", "moving_mean", "moving_variance"};

const std::vector<float>* getw(pp_engine* e, const std::string& name, std::initializer_list<int64_t> shape) {
    auto it = e->hw.find(name);
    if (it == e->hw.end()) { e->err = "missing weight tensor '" + name + "'"; return nullptr; }
    const auto& sh = e->hshape[name];
    std::vector<int64_t> want(shape);
    if (sh != want) {
        std::string s = "weight '" + name + "' has shape [";
        for (auto v : sh) s += std::to_string(v) + ",";
        s += "] expected [";
        for (auto v : want) s += std::to_string(v) + ",";
        s += "]";
        e->err = s;
        return nullptr;
    }
    return &it->second;
}

// BatchNorm inference folded to y = x*scale + shift (eps 1e-3: model/pointpillars.py:109; Keras default for the RPN)
bool bn_fold(pp_engine* e, const std::string& prefix, int c, std::vector<float>& scale, std::vector<float>& shift) {
    const std::vector<float>* p[4];
    for (int i = 0; i < 4; ++i) {
        p[i] = getw(e, prefix + "/" + kBn[i], {c});
        if (!p[i]) return false;
    }
    scale.resize(c);
    shift.resize(c);
    for (int i = 0; i < c; ++i) {
        const float inv = (*p[0])[i] / sqrtf((*p[3])[i] + 1e-3f);
        scale[i] = inv;
        shift[i] = (*p[1])[i] - (*p[2])[i] * inv;
    }
    return true;
}

int upload(pp_engine* e, float** d, const std::vector<float>& h) {
    void* q = nullptr;
    HIPCHK(e, hipMalloc(&q, (h.size() ? h.size() : 1) * sizeof(float)));
    e->wallocs.push_back(q);   // released by the next pp_finalize_weights / pp_destroy
    *d = (float*)q;
    HIPCHK(e, hipMemcpy(*d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return PP_OK;
}

// Split-precision operand for the float16 matrix pipe: every float32 weight w becomes two float16 pieces hi + mid
// (round-to-nearest-even each), laid out [cin / 16][piece][n_total][16] so that one K-chunk's tile of one piece is
// contiguous (what k_sep_u / the deconv kernels stage into LDS).  Returned as raw 16-bit words packed in floats.
std::vector<float> split_weights_f16x2(const std::vector<float>& wt, int n_total, int cin) {
    std::vector<uint16_t> out((size_t)n_total * cin * PP_NPIECE);
    for (int n = 0; n < n_total; ++n)
        for (int c = 0; c < cin; ++c) {
            const float w = wt[(size_t)n * cin + c];
            const _Float16 hf = (_Float16)w;
            const _Float16 mf = (_Float16)(w - (float)hf);
            uint16_t pcs[PP_NPIECE];
            memcpy(&pcs[0], &hf, 2);
            memcpy(&pcs[1], &mf, 2);
            const int kc = c / 16, cc = c % 16;
            for (int p = 0; p < PP_NPIECE; ++p) out[(((size_t)kc * PP_NPIECE + p) * n_total + n) * 16 + cc] = pcs[p];
        }
    std::vector<float> packed(out.size() / 2);
    memcpy(packed.data(), out.data(), out.size() * 2);
    return packed;
}

// May these BN-folded weights go to the two-float16-piece operand layout?  A piece is a float16: |w| must stay below
// its largest finite value (with headroom for the rounding of hi); a layer that fails runs on the float32 matrix
// instruction instead (its d_wt16 stays NULL and the launchers pick the PREC = 0 instantiations).  Small weights need
// no guard: below 2^-3 the mid piece is a float16 subnormal, so a weight carries an ABSOLUTE error of at most 2^-25,
// which is what bounds the error of a dot product whose other terms are O(1).
static bool f16_pair_range_ok(const std::vector<float>& wt) {
    for (float w : wt)
        if (!(fabsf(w) < 32768.f)) return false;      // also catches NaN / inf
    return true;
}

// canvas -> host (debug taps).  With the sparse canvas the cells without a pillar were never written: they are
// zeroed here from the cell map, so the caller sees the dense pseudo-image of the reference.
static int fetch_canvas(pp_engine* e, float* canvas, int batch, int set) {
    const size_t plane = (size_t)e->ny * e->nx;
    HIPCHK(e, hipMemcpyAsync(canvas, e->d_canvas, (size_t)batch * plane * e->C * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (!e->sparse_canvas) return PP_OK;
    std::vector<int> cm((size_t)batch * e->nz * plane);
    HIPCHK(e, hipMemcpy(cm.data(), e->vox[set].cellmap, cm.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b)
        for (size_t c = 0; c < plane; ++c) {
            bool occ = false;
            for (int z = 0; z < e->nz; ++z) occ = occ || cm[((size_t)b * e->nz + z) * plane + c] >= 0;
            if (!occ) memset(canvas + ((size_t)b * plane + c) * e->C, 0, (size_t)e->C * sizeof(float));
        }
    return PP_OK;
}

}  // namespace

// ---- stage pipelines (all enqueue on e->stream) ----
static const unsigned* sorted_idx(pp_engine* e) {
    return (voxel_sort_passes(e->cfg.max_voxels) % 2 == 0) ? e->d_idxA : e->d_idxB;
}

int run_voxelize(pp_engine* e, int batch, int max_n, hipStream_t vs) {
    if (vs == nullptr) {
        vs = e->stream;
        // the voxeliser's scratch (cells, keys, indices) exists once: a launch here must not overtake one that
        // pp_upload_points_async queued on the copy stream
        if (e->prevox_issued) { HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_up, 0)); e->prevox_issued = false; }
        e->main_vox_pending = true;
    }
    const bool lds_first = voxel_first_in_lds(max_n, e->ncell, e->cfg.max_voxels);
    int* d_first = lds_first ? nullptr : e->d_first;
    if (!lds_first) {
        ProfScope ps(e, "k_fill_first");   // (0x7f7f7f7f: the bytes the memset of rounds 1-4 wrote)
        launch_fill_first(e->d_first, 0x7f7f7f7f, (long long)batch * e->ncell, vs);
    }
    {
        ProfScope ps(e, "k_cell_first");   // also clears the cell map
        launch_cell_first(e->d_points, e->d_offsets, batch, max_n, e->F, e->geom, e->d_cell, d_first, e->d_cellmap,
                          e->zc ? e->d_feed[e->in_buf] : nullptr, e->d_points, e->d_offsets, vs,
                          e->sparse_canvas ? e->d_occbits : nullptr, e->ny * occ_words(e->nx));
        e->vox[e->in_buf].occ_cleared = e->sparse_canvas;
    }
    {
        ProfScope ps(e, "k_voxel_frame");
        launch_voxel_frame(e->d_offsets, e->d_cell, d_first, e->d_cellmap, e->d_keyA, e->d_idxA, e->d_keyB,
                           e->d_idxB, e->d_pstart, e->d_pcell, e->d_npillars, e->d_nvalid, batch, max_n, e->ncell,
                           e->cfg.max_voxels, vs);
    }
    {
        ProfScope ps(e, "k_sort_points");
        launch_sort_points(e->d_points, e->d_offsets, sorted_idx(e), e->d_nvalid, batch, max_n, e->F,
                           e->d_points_sorted, vs);
    }
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// largest batch whose anchor masks ride in the PFN launch.  Few frames only: the 32 KB LDS image the extra workgroups
// declare caps EVERY workgroup of the launch at 5 per CU, and a full chip of PFN workgroups lives on occupancy (B = 64:
// 73 -> 99 us with the masks inside, against 14 us for the three mask kernels by themselves); on one frame the launch
// is 14.7 us instead of 12.2 + 8.8.
static constexpr int kAnchorMaskInPfnMaxBatch = 8;

static int run_pfn(pp_engine* e, int batch, bool padded, float* feat_out, bool with_mask = false) {
    PfnParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.nz = e->nz; p.ny = e->ny; p.nx = e->nx; p.C = e->C; p.F = e->F; p.T = e->T;
    p.max_voxels = e->cfg.max_voxels;
    p.vx = (float)e->cfg.voxel_size[0];
    p.vy = (float)e->cfg.voxel_size[1];
    // Python-float64 arithmetic, then a float32 constant (model/pointpillars.py:121-124)
    p.x_off = (float)(e->cfg.voxel_size[0] / 2 + e->cfg.pc_range[0]);
    p.y_off = (float)(e->cfg.voxel_size[1] / 2 + e->cfg.pc_range[1]);
    p.w = e->d_pfn_w; p.bias = e->d_pfn_b; p.cellmap = e->d_cellmap;
    p.pts_sorted = e->d_points_sorted; p.offsets = e->d_offsets; p.pillar_start = e->d_pstart;
    p.pillar_cell = e->d_pcell; p.npillars = e->d_npillars;
    p.voxels = e->d_voxels; p.num_points = e->d_numpts;
    p.canvas = e->d_canvas; p.feat_out = feat_out;
    p.sparse = e->sparse_canvas ? 1 : 0;
    p.with_distance = e->with_dist ? 1 : 0;
    // the bitmap is only as good as its clearing: the fused path's k_cell_first does it (run_voxelize); the stage entry
    // points build the cell map from the caller's coordinates and keep the cell-map lookups
    p.occbits = (e->sparse_canvas && !padded && e->vox[e->in_buf].occ_cleared) ? e->d_occbits : nullptr;
    const PpSwitches& sw = e->plan_env.sw;
    e->occbits_live = p.occbits != nullptr && pfn_writes_occbits(p, padded, sw);
    if (!e->occbits_live) p.occbits = nullptr;
    e->vox[e->in_buf].occ_cleared = false;
    e->mask_in_pfn = false;
    if (with_mask && batch <= kAnchorMaskInPfnMaxBatch && pfn_can_carry_anchor_mask(p, padded, sw)) {
        // the anchor mask (needs the cell map only, read by the post-process only) rides in this launch
        p.am_cells = e->d_cells; p.am_A = e->A; p.am_threshold = e->cfg.anchor_area_threshold; p.am_mask = e->d_mask;
        e->mask_in_pfn = true;
    }
    ProfScope ps(e, nullptr);   // under the name of the kernel launch_pfn chooses (k_pfn_canvas or k_pfn_canvas2)
    int st = launch_pfn(p, padded, sw, e->stream);
    if (st) return fail(e, st, "PFN: unsupported C=%d / F=%d", e->C, e->F);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

static int run_anchor_mask(pp_engine* e, int batch) {
    ProfScope ps(e, nullptr);   // three kernels, each under its own name
    if (e->occbits_live && e->nz == 1) {   // one z-cell: a bit of the occupancy bitmap is the pillar count
        launch_anchor_mask_bits(e->d_occbits, batch, e->ny, e->nx, e->d_cells, e->A, e->cfg.anchor_area_threshold, e->d_mask,
                                e->stream);
        HIPCHK(e, hipGetLastError());
        return PP_OK;
    }
    launch_anchor_mask(e->d_cellmap, batch, e->nz, e->ny, e->nx, e->d_cells, e->A, e->cfg.anchor_area_threshold,
                       e->d_integ, e->d_mask, e->stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

static void refresh_tags(pp_engine* e, int batch) {
    if (e->tag_batch == batch) return;
    for (size_t i = 0; i < e->layers.size(); ++i)
        e->layer_tags[i] = layer_kernel_name(e->layers[i], batch, e->plan_env) + ":" + e->layers[i].name;
    e->tag_batch = batch;
}

static int run_backbone(pp_engine* e, int batch) {
    refresh_tags(e, batch);
    e->cls_plane_live = false;
    for (const LayerDesc& L : e->layers) if (layer_writes_cls_plane(L, e->plan_env)) e->cls_plane_live = true;
    // Frame sub-ranges for the layers whose maps do not fit the last-level cache (round 4).  A run of consecutive
    // separable layers of a block is walked sub-batch by sub-batch -- L1(s0) L2(s0) L3(s0), L1(s1) ... -- so that what a
    // layer reads is what the layer before has just written for the same frames and still sits in the 256 MB cache:
    // on the KITTI-shaped B = 32 maps (439 MB in block1, 219 MB in block2) a layer's loads are a third of its time, on
    // cfg-A's 84-168 MB maps they are free already.  Same kernels, same buffers, same pixel
    // numbering: a launch walks a sub-range of the batch's tiles (launch_layer's frame0).  The budget (input + output map
    // of a launch) is the handle's cache_budget_mb: pp_set_cache_budget, default 256 = the whole cache for ONE handle in
    // flight; callers that keep several handles in flight set 0 -- their working sets evict each other and the extra
    // launches only cost (measured: DESIGN section 4.6).
    const int sub_on = e->cache_budget_mb > 0 ? 1 : 0;
    const long sub_mb = e->cache_budget_mb;
    size_t i = 0;
    while (i < e->layers.size()) {
        // the run [i, j) of separable layers, and the sub-batch it is walked in (1 = the whole batch)
        size_t j = i;
        int sub = batch;
        if (sub_on && e->layers[i].kind == LAYER_SEP) {
            // The two activation buffers ping-pong, so layers i+1, i+3, ... write the buffer that holds the run's input:
            // walked sub-range by sub-range, L(i+1) of frames [f0, f0 + nb) writes [f0, f0 + nb) * its output bytes per
            // frame while L(i) has yet to read frames f0 + nb.. of that buffer at its input bytes per frame.  A layer that
            // writes more per frame than the run's first layer reads (a stride-1 block that widens the channels, or stride 2
            // with cout > 4 cin) ends the run before it.  (The other buffer holds nothing that a later sub-range reads: each
            // of its readers reads what the layer before wrote for the same frames; the layers after the first share one
            // output shape, so the run's last output is not overwritten either.)
            const LayerDesc& l0 = e->layers[i];
            // (floats per frame of the run's input: its producer, a separable layer, writes rows of ld_out = cout = cin)
            const size_t in0 = (size_t)l0.in_h * l0.in_w * l0.cin;
            while (j < e->layers.size() && e->layers[j].kind == LAYER_SEP) {
                const LayerDesc& l = e->layers[j];
                if (j > i && l.out == l0.in && (size_t)l.out_h * l.out_w * l.ld_out > in0) break;
                ++j;
            }
            double per_frame = 0.0;          // bytes of the largest (input + output) map pair of the run, per frame
            for (size_t k = i; k < j; ++k) {
                const LayerDesc& l = e->layers[k];
                const double in_b = (k == 0 && l.d_occ != nullptr) ? 0.0 : 4.0 * l.in_h * l.in_w * l.cin;   // (the sparse canvas is not read as a map)
                per_frame = std::max(per_frame, in_b + 4.0 * l.out_h * l.out_w * l.cout);
            }
            const double budget = (double)sub_mb * 1048576.0;
            while (sub > 1 && per_frame * sub > budget && sub % 2 == 0) sub /= 2;
            // every launch must stay a full-chip k_sep_u launch whose sub-range starts on a tile boundary
            for (bool ok = false; sub < batch && !ok; ) {
                ok = true;
                for (size_t k = i; k < j && ok; ++k)
                    for (int f0 = 0; f0 < batch && ok; f0 += sub)
                        ok = launch_layer_subrange_ok(e->layers[k], f0, std::min(sub, batch - f0), batch, e->plan_env) &&
                             (long long)sub * e->layers[k].out_h * e->layers[k].out_w >= 1024ll * 128;
                if (!ok) sub *= 2;
            }
            if (sub >= batch) sub = batch;
        } else {
            j = i + 1;
        }
        for (int f0 = 0; f0 < batch; f0 += sub) {
            const int nb = std::min(sub, batch - f0);
            for (size_t k = i; k < j; ++k) {
                LayerDesc L = e->layers[k];
                // sparse first layer: the occupancy bitmap when this pass's PFN launch left one, else the cell map
                if (k == 0 && L.d_occ != nullptr) { L.d_occ = e->d_cellmap; L.d_occbits = e->occbits_live ? e->d_occbits : nullptr; }
                ProfScope ps(e, e->layer_tags[k].c_str());
                int st = launch_layer(L, nb, e->d_head, e->stream, e->plan_env, f0);
                if (st) return fail(e, st, "layer %s: unsupported shape (cin=%d cout=%d)", L.name, L.cin, L.cout);
            }
        }
        i = j;
    }
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// to_host: the kernel also fills the page-locked result buffers (the fused path: no copy nodes behind it)
static int run_post(pp_engine* e, int batch, bool to_host = false) {
    PostParams p;
    p.batch = batch; p.A = e->A; p.pre_max = e->cfg.nms_pre_max_size; p.post_max = e->cfg.nms_post_max_size;
    p.score_thr = e->cfg.nms_score_threshold; p.iou_thr = e->cfg.nms_iou_threshold;
    p.head = e->d_head; p.cls = e->cls_plane_live ? e->d_cls : nullptr; p.napl = e->napl; p.ncls = e->ncls; p.use_dir = e->use_dir ? 1 : 0; p.mask = e->d_mask; p.anchors = e->d_anchors;
    p.calib = e->d_calib; p.dets = e->d_dets; p.n_dets = e->d_ndets;
    p.dets_host = to_host ? e->h_dets : nullptr; p.n_dets_host = to_host ? e->h_ndets : nullptr;
    const PostRule& r = e->rule;
    const bool proj = r.proj != 0;
    if (proj && batch > e->proj.batch)
        return fail(e, PP_ERR_STATE, "pp_set_projection gave matrices for %d frames; this pass has %d", e->proj.batch, batch);
    p.nms_mode = r.nms_mode; p.soft_method = r.soft_method; p.soft_sigma = r.soft_sigma; p.soft_floor = r.soft_floor;
    p.class_nms = r.class_nms; p.cls_dets = e->d_cls_dets; p.cls_cnt = e->d_cls_cnt;
    p.p2 = proj ? e->proj.d_p2 : nullptr; p.bbox = proj ? e->proj.d_bbox : nullptr; p.cls_bbox = proj ? e->proj.d_cls_bbox : nullptr;
    p.bbox_host = (proj && to_host) ? e->proj.h_bbox : nullptr;
    ProfScope ps(e, nullptr);      // the launch sites' own names: k_postprocess and, per-class mode, k_gather_classes
    launch_postprocess(p, e->stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// The stage entry points (pp_points_to_voxel, pp_anchor_mask, pp_forward_voxels, pp_predict) reuse the fused
// path's device buffers (points, cell map, canvas, head map, mask, detections): after one of them the resident
// frames and the last results of the fused path are gone, and the calls that would read them say so.
static void stage_call_done(pp_engine* e) {
    e->cur_batch = 0;
    ++e->resident_gen;
    e->cur_max_n = 0;
    e->cur_total = 0;
    e->results_batch = 0;
    e->results_rows = 0;
    e->proj.results = 0;
}

int check_batch(pp_engine* e, int batch) {
    if (batch < 1 || batch > e->B) return fail(e, PP_ERR_ARG, "batch %d outside [1, max_batch=%d]", batch, e->B);
    return PP_OK;
}

// the voxeliser products the d_* members name: set i (follows in_buf)
static void use_vox_set(pp_engine* e, int i) {
    const pp_engine::VoxSet& v = e->vox[i];
    e->d_points_sorted = v.points_sorted; e->d_cellmap = v.cellmap; e->d_pstart = v.pstart; e->d_pcell = v.pcell;
    e->d_npillars = v.npillars; e->d_nvalid = v.nvalid; e->d_occbits = v.occbits;
}

// ---- the resident frames' state: every feed, and every call that replaces the frames, goes through these ----

// Orders `s` behind the frames' upload (and voxelisation) on the copy stream, once per upload.
int wait_for_upload(pp_engine* e, hipStream_t s) {
    if (e->up_pending || e->prevox_issued) {
        HIPCHK(e, hipStreamWaitEvent(s, e->ev_up, 0));
        e->up_pending = false;
        e->prevox_issued = false;
    }
    return PP_OK;
}

// Orders the main stream behind what a call has queued on `up` (nothing to do when that is the main stream).
int copies_done(pp_engine* e, hipStream_t up) {
    if (up == e->stream) return PP_OK;
    HIPCHK(e, hipEventRecord(e->ev_tgt, up));
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_tgt, 0));
    return PP_OK;
}

// The next upload goes to the other input buffer: d_points / d_offsets and the voxeliser products follow it.
int flip_input(pp_engine* e) {
    const int nb = e->in_buf ^ 1;
    e->in_buf = nb;
    e->d_points = e->d_points_buf[nb];
    e->d_offsets = e->d_offsets_buf[nb];
    use_vox_set(e, nb);
    e->vox_ahead = false;
    return nb;
}

// What the host knows of the resident frames: their offsets `off` [batch + 1], or (`exact` false) prefix sums of per-frame bounds
void set_resident(pp_engine* e, int batch, const int* off, int max_n, bool exact) {
    e->cur_batch = batch;
    ++e->resident_gen;
    e->cur_max_n = max_n;
    e->cur_total = off[batch];
    e->h_cur_off.assign(off, off + batch + 1);
    e->off_host_exact = exact;
}

int require_host_exact(pp_engine* e, const char* who) {
    if (e->off_host_exact) return PP_OK;
    return fail(e, PP_ERR_STATE, "%s: the resident frames were sampled inside a training step or ingested from camera messages, their sizes are device values (upload frames first)", who);
}

// The resident points as a kernel queued on `s` reads them (*src): behind their upload; a zero-copy feed where it lies, in
// the caller's page-locked memory, after its offsets have been copied to d_offsets.  `materialise`: the caller writes a
// new cloud into d_points behind this, so the feed counts as replaced by device copies from here on.
int resident_points(pp_engine* e, int batch, hipStream_t s, bool materialise, const float** src) {
    if (int st = wait_for_upload(e, s)) return st;
    *src = e->d_points;
    if (e->zc) {
        const PpFeed* f = e->h_feed[e->in_buf];
        HIPCHK(e, hipMemcpyAsync(e->d_offsets, f->offsets, (size_t)(batch + 1) * sizeof(int), hipMemcpyHostToDevice, s));
        *src = f->src;
    }
    if (materialise) { e->zc = false; e->vox_ahead = false; }
    return PP_OK;
}

int ensure_spare_pts(pp_engine* e) { return e->spare_pts ? PP_OK : dalloc(e, &e->spare_pts, (size_t)e->B * e->NMAX * e->F); }

// frame offsets as every feed takes them; *max_n: the largest frame
static int check_offsets(pp_engine* e, const int32_t* off, int batch, int* max_n) {
    if (!off) return fail(e, PP_ERR_ARG, "frame_offsets is NULL");
    if (off[0] != 0) return fail(e, PP_ERR_ARG, "frame_offsets[0] must be 0");
    *max_n = 0;
    for (int b = 0; b < batch; ++b) {
        const int n = off[b + 1] - off[b];
        if (n < 0) return fail(e, PP_ERR_ARG, "frame_offsets not monotone at frame %d", b);
        if (n > e->NMAX) return fail(e, PP_ERR_ARG, "frame %d has %d points > max_points_per_frame=%d", b, n, e->NMAX);
        *max_n = std::max(*max_n, n);
    }
    return PP_OK;
}

// Validates the frame offsets, flips to the other input buffer and queues the offsets' copy on `stream`
// (the main stream, or the copy stream for the asynchronous upload -- which first waits until the pass that
// last read that buffer has finished).
static int set_offsets(pp_engine* e, const int32_t* off, int batch, hipStream_t stream) {
    int max_n = 0;
    if (int st = check_offsets(e, off, batch, &max_n)) return st;
    e->zc = false;                                     // inputs arrive by copy: the first kernel reads device memory
    int slot;
    HIPCHK(e, e->ring.take(&slot));
    memcpy(e->h_off.at(slot), off, (size_t)(batch + 1) * sizeof(int));
    set_resident(e, batch, off, max_n, true);
    if (int st = flip_for_write(e, stream)) return st;
    HIPCHK(e, e->h_off.send(slot, e->d_offsets, (size_t)batch + 1, stream));
    HIPCHK(e, e->ring.sent(slot, stream));
    return PP_OK;
}

// The tail of an asynchronous upload: voxelises the frames just queued on the copy stream right there, behind their
// copy and beside the pass in flight, and records ev_up for the next reader (wait_for_upload).  No voxeliser while
// per-launch times are collected (their events belong to the main stream's pass) and none on a handle that trains
// (pp_train_step voxelises inside its own graphs).
int finish_async_upload(pp_engine* e, int batch) {
    if (e->prof <= 0 && e->train == nullptr) {
        // The voxeliser's scratch (cells, keys, sorted indices) exists once per handle: a voxeliser queued on the main
        // stream -- the pass in flight, if it was fed by zero-copy / pp_upload_points / pp_upload_points_device -- must
        // be through before this one overwrites it.  Only after such a pass: copy feed after copy feed adds no wait.
        if (e->main_vox_pending) {
            HIPCHK(e, hipEventRecord(e->ev_vox_main, e->stream));
            HIPCHK(e, hipStreamWaitEvent(e->copy_stream, e->ev_vox_main, 0));
            e->main_vox_pending = false;
        }
        if (int st = run_voxelize(e, batch, e->cur_max_n, e->copy_stream)) return st;
        e->vox_ahead = true;
        e->prevox_issued = true;
    }
    HIPCHK(e, hipEventRecord(e->ev_up, e->copy_stream));
    e->up_pending = true;
    return PP_OK;
}

// fused head map [pixels][PP_HEAD_COLS] <-> the reference's three NHWC head tensors
static int fetch_heads(pp_engine* e, int batch, float* box, float* cls, float* dir) {
    const size_t px = (size_t)batch * e->head_h * e->head_w;
    const int nb = e->napl * 7, nc = e->napl * e->ncls, nd = e->use_dir ? e->napl * 2 : 0;
    std::vector<float> h(px * PP_HEAD_COLS);
    HIPCHK(e, hipMemcpyAsync(h.data(), e->d_head, h.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (size_t p = 0; p < px; ++p) {
        const float* r = h.data() + p * PP_HEAD_COLS;
        if (box) memcpy(box + p * nb, r, nb * sizeof(float));
        if (cls) memcpy(cls + p * nc, r + nb, nc * sizeof(float));
        if (dir && nd) memcpy(dir + p * nd, r + nb + nc, nd * sizeof(float));
    }
    return PP_OK;
}

static int upload_heads(pp_engine* e, int batch, const float* box, const float* cls, const float* dir) {
    const size_t px = (size_t)batch * e->head_h * e->head_w;
    const int nb = e->napl * 7, nc = e->napl * e->ncls, nd = e->use_dir ? e->napl * 2 : 0;
    std::vector<float> h(px * PP_HEAD_COLS, 0.f);
    for (size_t p = 0; p < px; ++p) {
        float* r = h.data() + p * PP_HEAD_COLS;
        memcpy(r, box + p * nb, nb * sizeof(float));
        memcpy(r + nb, cls + p * nc, nc * sizeof(float));
        if (nd) memcpy(r + nb + nc, dir + p * nd, nd * sizeof(float));
    }
    HIPCHK(e, hipMemcpyAsync(e->d_head, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));   // h is a local
    e->cls_plane_live = false;                    // the compact plane no longer mirrors the head map
    return PP_OK;
}

static void calib_matrix(const float* rect, const float* trv, float* M) {
    // r_rect @ velo2cam in float32 (libraries/eval_helper_functions.py:732)
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = 0.f;
            for (int k = 0; k < 4; ++k) s += rect[i * 4 + k] * trv[k * 4 + j];
            M[i * 4 + j] = s;
        }
}

extern "C" {

int pp_abi_version(void) { return PP_ABI_VERSION; }

const char* pp_last_error(pp_handle h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int pp_create(const pp_config* cfg, int device, pp_handle* out) {
    if (!cfg || !out) return fail(nullptr, PP_ERR_ARG, "pp_create: NULL argument");
    *out = nullptr;
    if (!bits_ok(*cfg)) return fail(nullptr, PP_ERR_ARG, "pp_create: bad range / voxel size");
    if (cfg->max_points < 1 || cfg->max_voxels < 1 || cfg->max_batch < 1 || cfg->max_points_per_frame < 1)
        return fail(nullptr, PP_ERR_ARG, "pp_create: max_points / max_voxels / max_batch / max_points_per_frame must be >= 1");
    if (cfg->num_point_features != 3 && cfg->num_point_features != 4)
        return fail(nullptr, PP_ERR_UNSUPPORTED, "pp_create: num_point_features must be 3 or 4");
    if (cfg->num_class < 1) return fail(nullptr, PP_ERR_ARG, "pp_create: num_class must be >= 1");
    if (cfg->num_anchor_per_loc < 1 ||
        cfg->num_anchor_per_loc * (7 + cfg->num_class + (cfg->use_direction_classifier ? 2 : 0)) > PP_HEAD_COLS)
        return fail(nullptr, PP_ERR_UNSUPPORTED, "pp_create: num_anchor_per_loc * (7 + num_class + 2) must fit the %d-column head row", PP_HEAD_COLS);
    if (cfg->nms_post_max_size < 1 || cfg->nms_pre_max_size < 1)
        return fail(nullptr, PP_ERR_ARG, "pp_create: nms sizes must be >= 1");
    if (int st = check_device("pp_create", device)) return st;
    pp_engine* e = new pp_engine();
    e->cfg = *cfg;
    e->device = device;
    hipError_t st = hipSetDevice(device);
    if (st == hipSuccess) st = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
    if (st != hipSuccess) {
        fail(nullptr, PP_ERR_HIP, "pp_create: %s", hipGetErrorString(st));
        delete e;
        return PP_ERR_HIP;
    }
    {
        e->plan_env.sw = pp_switches();
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && ncu > 0)
            e->plan_env.cus = ncu;
    }
    for (int j = 0; j < 3; ++j) {
        e->geom.lo[j] = cfg->pc_range[j];
        e->geom.vs[j] = cfg->voxel_size[j];
        e->geom.grid[j] = (int)nearbyint((cfg->pc_range[3 + j] - cfg->pc_range[j]) / cfg->voxel_size[j]);
    }
    e->nx = e->geom.grid[0]; e->ny = e->geom.grid[1]; e->nz = e->geom.grid[2];
    e->ncell = e->nx * e->ny * e->nz;
    e->geom.ncell = e->ncell;
    e->C = cfg->pfn_filters; e->F = cfg->num_point_features; e->T = cfg->max_points;
    e->ncls = cfg->num_class; e->use_dir = cfg->use_direction_classifier != 0; e->with_dist = cfg->with_distance != 0;
    e->FA = e->F + 5 + (e->with_dist ? 1 : 0);
    e->B = cfg->max_batch; e->NMAX = cfg->max_points_per_frame;
    e->napl = cfg->num_anchor_per_loc;
    const int osf = cfg->layer_strides[0] / cfg->upsample_strides[0];
    if (osf < 1 || e->nx < 1 || e->ny < 1 || e->nz < 1) {
        fail(nullptr, PP_ERR_ARG, "pp_create: degenerate grid");
        delete e;
        return PP_ERR_ARG;
    }
    e->head_h = e->ny / osf; e->head_w = e->nx / osf;
    e->A = (int64_t)e->head_h * e->head_w * e->napl;
    e->CC = cfg->num_upsample_filters[0] + cfg->num_upsample_filters[1] + cfg->num_upsample_filters[2];

    // layer table + map sizes
    int st2 = PP_OK;
    {
        int h = e->ny, w = e->nx, cin = e->C;
        size_t act_max = 1;
        int co_off = 0;
        static const char* sep_names[3][8] = {
            {"block1.0", "block1.1", "block1.2", "block1.3", "block1.4", "block1.5", "block1.6", "block1.7"},
            {"block2.0", "block2.1", "block2.2", "block2.3", "block2.4", "block2.5", "block2.6", "block2.7"},
            {"block3.0", "block3.1", "block3.2", "block3.3", "block3.4", "block3.5", "block3.6", "block3.7"}};
        static const char* dec_names[3] = {"deconv1", "deconv2", "deconv3"};
        for (int b = 0; b < 3 && st2 == PP_OK; ++b) {
            if (cfg->layer_nums[b] < 0 || cfg->layer_nums[b] > 7) { st2 = fail(nullptr, PP_ERR_UNSUPPORTED, "layer_nums[%d] must be 0..7", b); break; }
            for (int j = 0; j <= cfg->layer_nums[b]; ++j) {
                LayerDesc L;
                memset(&L, 0, sizeof(L));
                L.kind = LAYER_SEP; L.cin = cin; L.cout = cfg->num_filters[b];
                L.stride = (j == 0) ? cfg->layer_strides[b] : 1;
                L.in_h = h; L.in_w = w;
                L.out_h = (h + 2 - 3) / L.stride + 1; L.out_w = (w + 2 - 3) / L.stride + 1;
                L.n_total = L.cout; L.ld_out = L.cout; L.co_off = 0; L.name = sep_names[b][j];
                e->layers.push_back(L);
                h = L.out_h; w = L.out_w; cin = L.cout;
                act_max = std::max(act_max, (size_t)e->B * h * w * cin);
            }
            LayerDesc D;
            memset(&D, 0, sizeof(D));
            D.kind = LAYER_DECONV; D.cin = cin; D.cout = cfg->num_upsample_filters[b]; D.k = cfg->upsample_strides[b];
            D.in_h = h; D.in_w = w; D.out_h = h * D.k; D.out_w = w * D.k;
            D.n_total = D.k * D.k * D.cout; D.ld_out = e->CC; D.co_off = co_off; D.name = dec_names[b];
            if (D.out_h != e->head_h || D.out_w != e->head_w)
                st2 = fail(nullptr, PP_ERR_SHAPE, "deconv%d output %dx%d != head map %dx%d", b + 1, D.out_h, D.out_w, e->head_h, e->head_w);
            co_off += D.cout;
            e->layers.push_back(D);
        }
        if (st2 == PP_OK) {
            e->fuse_heads = true;
            for (const LayerDesc& L : e->layers)
                if (L.kind == LAYER_DECONV && !deconv_can_fuse_heads(L)) e->fuse_heads = false;
            if (e->plan_env.sw.no_head_fusion) e->fuse_heads = false;   // PP_NO_HEAD_FUSION: A/B switch for measurements
        }
        if (st2 == PP_OK && e->fuse_heads) {
            int nd = 0;
            for (LayerDesc& L : e->layers)
                if (L.kind == LAYER_DECONV) L.head_mode = (nd++ == 0) ? 1 : 2;
        }
        if (st2 == PP_OK && !e->fuse_heads) {
            LayerDesc H;
            memset(&H, 0, sizeof(H));
            H.kind = LAYER_HEAD; H.cin = e->CC; H.cout = 32; H.in_h = e->head_h; H.in_w = e->head_w;
            H.out_h = e->head_h; H.out_w = e->head_w; H.n_total = 32; H.name = "heads";
            e->layers.push_back(H);
        }
        if (st2 == PP_OK) {
            pp_engine* q = e;
            const size_t BN = (size_t)e->B * e->NMAX;
            const size_t BMV = (size_t)e->B * cfg->max_voxels;
            const size_t HW = (size_t)e->head_h * e->head_w;
            auto A1 = [&](int s) { if (st2 == PP_OK) st2 = s; };
            A1(dalloc(q, &e->d_points_buf[0], BN * e->F));
            A1(dalloc(q, &e->d_points_buf[1], BN * e->F));
            A1(dalloc(q, &e->d_offsets_buf[0], (size_t)e->B + 1));
            A1(dalloc(q, &e->d_offsets_buf[1], (size_t)e->B + 1));
            e->d_points = e->d_points_buf[0];
            e->d_offsets = e->d_offsets_buf[0];
            A1(dalloc(q, &e->d_cell, BN));
            A1(dalloc(q, &e->d_first, (size_t)e->B * e->ncell));
            A1(dalloc(q, &e->d_keyA, BN)); A1(dalloc(q, &e->d_idxA, BN));
            A1(dalloc(q, &e->d_keyB, BN)); A1(dalloc(q, &e->d_idxB, BN));
            for (pp_engine::VoxSet& v : e->vox) {   // the voxeliser's products, twice (see pp_engine::vox)
                A1(dalloc(q, &v.points_sorted, BN * e->F));
                A1(dalloc(q, &v.cellmap, (size_t)e->B * e->ncell));
                A1(dalloc(q, &v.pstart, (size_t)e->B * (cfg->max_voxels + 1)));
                A1(dalloc(q, &v.pcell, BMV));
                A1(dalloc(q, &v.npillars, (size_t)e->B));
                A1(dalloc(q, &v.nvalid, (size_t)e->B));
                A1(dalloc(q, &v.occbits, (size_t)e->B * e->ny * occ_words(e->nx)));
            }
            use_vox_set(e, 0);
            // activation buffers carry a zeroed PP_ZPAD_FLOATS header (see backbone.hip producers)
            auto APAD = [&](float** p, size_t count) {
                float* raw = nullptr;
                A1(dalloc(q, &raw, count + PP_ZPAD_FLOATS));
                if (st2 == PP_OK && hipMemset(raw, 0, PP_ZPAD_FLOATS * sizeof(float)) != hipSuccess) st2 = PP_ERR_HIP;
                *p = raw ? raw + PP_ZPAD_FLOATS : nullptr;
            };
            APAD(&e->d_canvas, (size_t)e->B * e->ny * e->nx * e->C);
            APAD(&e->d_act[0], act_max);
            APAD(&e->d_act[1], act_max);
            if (!e->fuse_heads) APAD(&e->d_concat, (size_t)e->B * HW * e->CC);
            A1(dalloc(q, &e->d_head, (size_t)e->B * HW * PP_HEAD_COLS));
            A1(dalloc(q, &e->d_cls, (size_t)e->B * HW * e->napl * e->ncls));
            A1(dalloc(q, &e->d_integ, (size_t)e->B * e->ny * e->nx));
            A1(dalloc(q, &e->d_mask, (size_t)e->B * e->A));
            A1(dalloc(q, &e->d_anchors, (size_t)e->A * 7));
            A1(dalloc(q, &e->d_cells, (size_t)e->A * 4));
            A1(dalloc(q, &e->d_anchor_near, (size_t)e->A));
            A1(dalloc(q, &e->tgt.gt.boxes, (size_t)e->B * PP_MAX_GT_PER_FRAME * 7));
            A1(dalloc(q, &e->tgt.gt.cls, (size_t)e->B * PP_MAX_GT_PER_FRAME));
            A1(dalloc(q, &e->tgt.gt.cnt, (size_t)e->B));
            A1(dalloc(q, &e->tgt.top, (size_t)e->B * PP_MAX_GT_PER_FRAME));
            A1(dalloc(q, &e->tgt.mask, (size_t)e->B * e->A));
            A1(dalloc(q, &e->d_calib, (size_t)e->B * 16));
            // result rows per frame: num_class * nms_post_max_size (the per-class mode's; the joint mode uses the first nms_post_max_size * B)
            A1(dalloc(q, &e->d_dets, (size_t)e->B * e->ncls * cfg->nms_post_max_size));
            A1(dalloc(q, &e->d_cls_dets, (size_t)e->B * e->ncls * cfg->nms_post_max_size));
            A1(dalloc(q, &e->d_cls_cnt, (size_t)e->B * e->ncls));
            A1(dalloc(q, &e->d_ndets, (size_t)e->B));
            if (st2 == PP_OK && hipHostMalloc((void**)&e->h_dets, (size_t)e->B * e->ncls * cfg->nms_post_max_size * sizeof(pp_detection)) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && hipHostMalloc((void**)&e->h_ndets, (size_t)e->B * sizeof(int)) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && (hipEventCreate(&e->t0) != hipSuccess || hipEventCreate(&e->t1) != hipSuccess)) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && e->h_off.alloc(e->ring, (size_t)e->B + 1) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && hipEventCreateWithFlags(&e->ev_main, hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            for (int i = 0; i < 2 && st2 == PP_OK; ++i) {
                void* dp = nullptr;
                if (hipHostMalloc((void**)&e->h_feed[i], sizeof(PpFeed) + (size_t)(e->B + 1) * sizeof(int)) != hipSuccess ||
                    hipHostGetDevicePointer(&dp, e->h_feed[i], 0) != hipSuccess) st2 = PP_ERR_HIP;
                e->d_feed[i] = (const PpFeed*)dp;
            }
            if (st2 == PP_OK && hipEventCreateWithFlags(&e->ev_up, hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && hipEventCreateWithFlags(&e->ev_vox_main, hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK && hipEventCreateWithFlags(&e->ev_tgt, hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            for (int i = 0; i < 2 && st2 == PP_OK; ++i)
                if (hipEventCreateWithFlags(&e->ev_read[i], hipEventDisableTiming) != hipSuccess) st2 = PP_ERR_HIP;
            if (st2 == PP_OK) {
                // one upload stream per device, shared by every handle: the host link is one resource, and the
                // runtime multiplexes streams onto a handful of hardware queues (GPU_MAX_HW_QUEUES, default 4) --
                // a private copy stream per handle made the handles' compute streams share queues and serialise
                e->copy_stream = device_copy_stream(device);
                if (e->copy_stream == nullptr) st2 = PP_ERR_HIP;
            }
            if (st2 == PP_OK) {
                // identity calibration until pp_set_calib
                std::vector<float> I((size_t)e->B * 16, 0.f);
                for (int b = 0; b < e->B; ++b) for (int d = 0; d < 4; ++d) I[(size_t)b * 16 + d * 5] = 1.f;
                if (hipMemcpy(e->d_calib, I.data(), I.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) st2 = PP_ERR_HIP;
            }
            if (st2 != PP_OK && g_create_error.empty()) g_create_error = e->err.empty() ? "pp_create: allocation failed" : e->err;
            if (st2 != PP_OK && !e->err.empty()) g_create_error = e->err;
        }
        // wire activation buffers: ping-pong inside the blocks, deconvs into the concat buffer
        if (st2 == PP_OK) {
            e->layer_tags.assign(e->layers.size(), std::string());
            const float* cur = e->d_canvas;
            int pp = 0;
            if (e->fuse_heads) {   // the last branch finishes the head sums
                LayerDesc* last = nullptr;
                for (LayerDesc& L : e->layers) if (L.kind == LAYER_DECONV) last = &L;
                if (last && last->head_mode == 2) {
                    last->d_cls_plane = e->d_cls;
                    last->cls_col0 = e->napl * 7;
                    last->cls_ncol = e->napl * e->ncls;
                }
            }
            for (LayerDesc& L : e->layers) {
                if (L.kind == LAYER_SEP) { L.in = cur; L.out = e->d_act[pp]; cur = L.out; pp ^= 1; }
                else if (L.kind == LAYER_DECONV) { L.in = cur; L.out = e->fuse_heads ? nullptr : e->d_concat; }
                else { L.in = e->d_concat; L.out = nullptr; }
            }
        }
    }
    if (st2 != PP_OK) { pp_destroy(e); return st2; }
    *out = e;
    return PP_OK;
}

static void graph_invalidate(pp_engine* e);

int pp_destroy(pp_handle e) {
    if (!e) return PP_OK;
    (void)hipSetDevice(e->device);
    if (e->copy_stream) (void)hipStreamSynchronize(e->copy_stream);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    graph_invalidate(e);
    for (void* p : e->allocs) (void)hipFree(p);
    for (void* p : e->wallocs) (void)hipFree(p);
    // what lives outside `allocs`: the loaded database, the grow-only buffers, page-locked memory, events
    for (void* p : {(void*)e->db.pts, (void*)e->db.off, (void*)e->db.box, (void*)e->db.cls, (void*)e->ing.raw, (void*)e->ing.chunks,
                    (void*)e->gdb.out, (void*)e->d_voxels, (void*)e->d_numpts, (void*)e->d_coors, (void*)e->d_feat})
        if (p) (void)hipFree(p);
    if (e->train) for (auto& tg : e->train->graph) { destroy_exec(&tg.exec); destroy_exec(&tg.exec_bwd); }
    delete e->train;
    e->ring.release();      // with the riders' arrays (before the stages reset the structs those live in)
    track_release(e);
    sweeps_release(e);
    costmap_release(e);
    occupancy_release(e);
    inflate_release(e);
    local_plan_release(e);
    scan_match_release(e);
    object_mask_release(e);
    ground_release(e);
    frontier_release(e);
    navfn_release(e);
    for (void* p : {(void*)e->h_feed[0], (void*)e->h_feed[1], (void*)e->h_train_losses, (void*)e->h_dets, (void*)e->h_ndets, (void*)e->proj.h_bbox, (void*)e->metrics.h_counts})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t ev : {e->ev_in, e->ev_main, e->ev_up, e->ev_vox_main, e->ev_tgt,
                          e->ev_read[0], e->ev_read[1], e->t0, e->t1})
        if (ev) (void)hipEventDestroy(ev);
    for (hipEvent_t ev : e->events) (void)hipEventDestroy(ev);
    if (e->stream) (void)hipStreamDestroy(e->stream);
    delete e;
    return PP_OK;
}

int pp_set_weight(pp_handle e, const char* name, const float* data, const int64_t* shape, int32_t ndim) {
    if (!e) return PP_ERR_ARG;
    if (!name || !data || !shape || ndim < 1 || ndim > 4) return fail(e, PP_ERR_ARG, "pp_set_weight: bad argument");
    size_t n = 1;
    std::vector<int64_t> sh(shape, shape + ndim);
    for (auto v : sh) { if (v < 1) return fail(e, PP_ERR_SHAPE, "pp_set_weight(%s): non-positive dim", name); n *= (size_t)v; }
    e->hw[name].assign(data, data + n);
    e->hshape[name] = sh;
    e->weights_ready = false;
    return PP_OK;
}

int pp_finalize_weights(pp_handle e) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    graph_invalidate(e);          // waits for the stream; the captured graphs hold the old weight pointers
    e->weights_ready = false;
    for (void* p : e->wallocs) (void)hipFree(p);   // the previous weight set (the stream is idle)
    e->wallocs.clear();
    e->pub.live = false;          // ... a published one included
    std::vector<float> sc, sh;
    // PFN: dense [Fa,C] * scale, bias = shift
    {
        const auto* k = getw(e, "pfn/dense/kernel", {e->FA, e->C});
        if (!k || !bn_fold(e, "pfn/bn", e->C, sc, sh)) return PP_ERR_SHAPE;
        std::vector<float> w((size_t)e->FA * e->C);
        for (int f = 0; f < e->FA; ++f)
            for (int c = 0; c < e->C; ++c) w[(size_t)f * e->C + c] = (*k)[(size_t)f * e->C + c] * sc[c];
        int st = upload(e, &e->d_pfn_w, w); if (st) return st;
        st = upload(e, &e->d_pfn_b, sh); if (st) return st;
    }
    // the three head kernels as one [PP_HEAD_COLS][CC] matrix (rows: box | cls | dir | zero pad) + bias
    std::vector<float> headw((size_t)PP_HEAD_COLS * e->CC, 0.f), headb(PP_HEAD_COLS, 0.f);
    {
        const int nb = e->napl * 7, nc = e->napl * e->ncls, nd = e->use_dir ? e->napl * 2 : 0, CC = e->CC;
        const auto* kb = getw(e, "rpn/conv_box/kernel", {1, 1, CC, nb});
        const auto* bb = getw(e, "rpn/conv_box/bias", {nb});
        const auto* kc = getw(e, "rpn/conv_cls/kernel", {1, 1, CC, nc});
        const auto* bc = getw(e, "rpn/conv_cls/bias", {nc});
        if (!kb || !bb || !kc || !bc) return PP_ERR_SHAPE;
        for (int ci = 0; ci < CC; ++ci) {
            for (int o = 0; o < nb; ++o) headw[(size_t)o * CC + ci] = (*kb)[(size_t)ci * nb + o];
            for (int o = 0; o < nc; ++o) headw[(size_t)(nb + o) * CC + ci] = (*kc)[(size_t)ci * nc + o];
        }
        for (int o = 0; o < nb; ++o) headb[o] = (*bb)[o];
        for (int o = 0; o < nc; ++o) headb[nb + o] = (*bc)[o];
        if (e->use_dir) {   // model/voxelnet.py:690: the direction head exists only with use_direction_classifier
            const auto* kd = getw(e, "rpn/conv_dir_cls/kernel", {1, 1, CC, nd});
            const auto* bd = getw(e, "rpn/conv_dir_cls/bias", {nd});
            if (!kd || !bd) return PP_ERR_SHAPE;
            for (int ci = 0; ci < CC; ++ci)
                for (int o = 0; o < nd; ++o) headw[(size_t)(nb + nc + o) * CC + ci] = (*kd)[(size_t)ci * nd + o];
            for (int o = 0; o < nd; ++o) headb[nb + nc + o] = (*bd)[o];
        }
    }
    int bi = 0, li = 0;
    e->f32_fallback_layers = 0;
    for (LayerDesc& L : e->layers) {
        if (L.kind == LAYER_SEP) {
            const std::string pre = "rpn/block" + std::to_string(bi + 1) + "/" + std::to_string(li);
            const auto* dw = getw(e, pre + "/depthwise_kernel", {3, 3, L.cin, 1});
            const auto* pw = getw(e, pre + "/pointwise_kernel", {1, 1, L.cin, L.cout});
            if (!dw || !pw || !bn_fold(e, pre + "/bn", L.cout, sc, sh)) return PP_ERR_SHAPE;
            std::vector<float> wt((size_t)L.cout * L.cin);
            for (int ci = 0; ci < L.cin; ++ci)
                for (int co = 0; co < L.cout; ++co) wt[(size_t)co * L.cin + ci] = (*pw)[(size_t)ci * L.cout + co] * sc[co];
            int st = upload(e, &L.d_dw, *dw); if (st) return st;
            st = upload(e, &L.d_wt, wt); if (st) return st;
            L.d_wt16 = nullptr;
            if (!e->force_f32 && L.cin % 16 == 0 && f16_pair_range_ok(wt)) { st = upload(e, &L.d_wt16, split_weights_f16x2(wt, L.n_total, L.cin)); if (st) return st; }
            else ++e->f32_fallback_layers;
            st = upload(e, &L.d_bias, sh); if (st) return st;
            ++li;
        } else if (L.kind == LAYER_DECONV) {
            const std::string pre = "rpn/deconv" + std::to_string(bi + 1);
            const auto* k = getw(e, pre + "/kernel", {L.k, L.k, L.cout, L.cin});
            if (!k || !bn_fold(e, pre + "/bn", L.cout, sc, sh)) return PP_ERR_SHAPE;
            std::vector<float> wt(k->size());
            for (size_t n = 0; n < (size_t)L.n_total; ++n) {
                const int co = (int)(n % L.cout);
                for (int ci = 0; ci < L.cin; ++ci) wt[n * L.cin + ci] = (*k)[n * L.cin + ci] * sc[co];
            }
            int st = upload(e, &L.d_wt, wt); if (st) return st;
            L.d_wt16 = nullptr;
            L.d_head_wt16 = nullptr;
            if (!e->force_f32 && L.cin % 16 == 0 && f16_pair_range_ok(wt)) { st = upload(e, &L.d_wt16, split_weights_f16x2(wt, L.n_total, L.cin)); if (st) return st; }
            else ++e->f32_fallback_layers;
            st = upload(e, &L.d_bias, sh); if (st) return st;
            if (L.head_mode != 0) {   // this branch's [PP_HEAD_COLS][cout] slice of the head matrix
                std::vector<float> hw((size_t)PP_HEAD_COLS * L.cout);
                for (int o = 0; o < PP_HEAD_COLS; ++o)
                    for (int c = 0; c < L.cout; ++c) hw[(size_t)o * L.cout + c] = headw[(size_t)o * e->CC + L.co_off + c];
                st = upload(e, &L.d_head_wt, hw); if (st) return st;
                if (!e->force_f32 && L.cout % 32 == 0 && f16_pair_range_ok(hw)) {
                    // k_deconv_u feeds the head GEMM from its accumulator registers: slot (h, j) of 16-channel group
                    // (n, g) holds channel n*32 + (j&3) + 8*(2g + (j>>2)) + 4h (the 32x32 MFMA result layout); the
                    // head kernels get the same order of k
                    std::vector<float> hwp(hw.size());
                    for (int o = 0; o < PP_HEAD_COLS; ++o)
                        for (int c = 0; c < L.cout; ++c) {
                            const int n = c / 32, g = (c % 32) / 16, sl = c % 16, hh = sl / 8, j = sl % 8;
                            const int src = n * 32 + (j & 3) + 8 * (2 * g + (j >> 2)) + 4 * hh;
                            hwp[(size_t)o * L.cout + c] = hw[(size_t)o * L.cout + src];
                        }
                    st = upload(e, &L.d_head_wt16, split_weights_f16x2(hwp, PP_HEAD_COLS, L.cout)); if (st) return st;
                }
                st = upload(e, &L.d_head_bias, headb); if (st) return st;
            }
            ++bi; li = 0;
        } else {
            int st = upload(e, &L.d_wt, headw); if (st) return st;
            st = upload(e, &L.d_bias, headb); if (st) return st;
        }
    }
    decide_sparse_canvas(e);
    e->tag_batch = -1;            // which kernel runs a layer may depend on its weights (float16 range fallback)
    e->weights_ready = true;
    return PP_OK;
}

}  // extern "C"
// sparse canvas: on a large, mostly empty BEV grid (KITTI-shaped: 214 k cells, <= 12 k pillars) writing and
// re-reading the zeros of the pseudo-image is most of the PFN's and the first layer's traffic.  The PFN then
// writes only the cells that hold a pillar and the first layer looks every window position up in the cell
// map.  Needs the kernels that know the lookup (sparse_input_supported); PP_DENSE_CANVAS=1 turns it off.
void decide_sparse_canvas(pp_engine* e) {
    const long long cells = (long long)e->ny * e->nx;
    LayerDesc& L0 = e->layers[0];
    e->sparse_canvas = !e->plan_env.sw.dense_canvas && cells >= 32768 && 4ll * e->cfg.max_voxels <= cells &&
                       L0.in == e->d_canvas && sparse_input_supported(L0, e->B, e->plan_env);
    L0.d_occ = e->sparse_canvas ? e->d_cellmap : nullptr;
    L0.occ_nz = e->nz;
}
extern "C" {

int pp_set_anchors(pp_handle e, const float* anchors, const int32_t* cells, int64_t num_anchors) {
    if (e) graph_invalidate(e);
    if (!e) return PP_ERR_ARG;
    if (!anchors || !cells) return fail(e, PP_ERR_ARG, "pp_set_anchors: NULL argument");
    if (num_anchors != e->A) return fail(e, PP_ERR_SHAPE, "pp_set_anchors: got %lld anchors, config needs %lld", (long long)num_anchors, (long long)e->A);
    for (int64_t a = 0; a < num_anchors; ++a) {
        const int32_t* c = cells + a * 4;
        if (c[0] < 0 || c[1] < 0 || c[2] >= e->nx || c[3] >= e->ny || c[0] >= e->nx || c[1] >= e->ny || c[2] < 0 || c[3] < 0)
            return fail(e, PP_ERR_ARG, "pp_set_anchors: anchor %lld cells out of the %dx%d grid", (long long)a, e->nx, e->ny);
    }
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipMemcpy(e->d_anchors, anchors, (size_t)num_anchors * 7 * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->d_cells, cells, (size_t)num_anchors * 4 * sizeof(int), hipMemcpyHostToDevice));
    launch_anchor_near(e->d_anchors, num_anchors, e->d_anchor_near, e->stream);
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipStreamSynchronize(e->stream));
    e->anchors_ready = true;
    return PP_OK;
}

int pp_upload_points(pp_handle e, const float* points, const int32_t* frame_offsets, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    st = set_offsets(e, frame_offsets, batch, e->stream); if (st) return st;
    e->up_pending = false;
    const size_t n = (size_t)frame_offsets[batch];
    if (n && !points) return fail(e, PP_ERR_ARG, "pp_upload_points: points is NULL");
    if (n) HIPCHK(e, hipMemcpyAsync(e->d_points, points, n * e->F * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));  // the host buffers may be pageable / reused by the caller
    return PP_OK;
}

// largest batch fed zero-copy (pp_upload_points_async)
static constexpr int ZC_MAX_BATCH = 4;
// live pp_host_alloc blocks (base -> bytes) whose device mapping is the identity; pp_host_free removes its entry
// BEFORE the memory goes back to the runtime, so a later lookup of a recycled address cannot hit
static std::mutex g_pinned_mu;
static std::map<uintptr_t, size_t> g_pinned;
static bool pinned_block_holds(const void* p, size_t bytes) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    auto it = g_pinned.upper_bound(a);
    if (it == g_pinned.begin()) return false;
    --it;
    return a >= it->first && a + bytes <= it->first + it->second;
}

// Small batch, page-locked points: nothing is copied and no HIP call is made besides one event query -- the
// descriptor of the other input buffer gets the points' device address and the offsets, and the next pass's first
// kernel reads both over the host link (a 16 K-point frame is 196 KB: ~4 us of it) while it writes the device copies.
static int feed_zero_copy(pp_engine* e, const float* points_pinned, const int32_t* off, int batch) {
    int max_n = 0;
    if (int st = check_offsets(e, off, batch, &max_n)) return st;
    const void* dev = nullptr;
    if (off[batch] > 0) {
        // Device address of the caller's buffer.  No address is remembered per handle (a freed buffer's address can
        // come back as pageable memory): a range inside a LIVE pp_host_alloc block is its own device address
        // (hipHostMalloc under unified addressing) -- one lookup in the library's registry, which pp_host_free
        // updates -- and anything else is asked of the runtime on every call (pageable memory fails there and the
        // caller falls back to the copy path).
        const size_t bytes = (size_t)off[batch] * e->F * sizeof(float);
        if (pinned_block_holds(points_pinned, bytes)) dev = points_pinned;
        else {
            void* dp = nullptr;
            if (hipHostGetDevicePointer(&dp, (void*)points_pinned, 0) != hipSuccess || dp == nullptr) {
                (void)hipGetLastError();
                return PP_ERR_UNSUPPORTED;
            }
            dev = dp;
        }
    }
    const int nb = flip_input(e);
    // the pass that last read this buffer's descriptor (two uploads ago) must be through
    HIPCHK(e, hipEventSynchronize(e->ev_read[nb]));
    PpFeed* f = e->h_feed[nb];
    f->src = (const float*)dev;
    memcpy(f->offsets, off, (size_t)(batch + 1) * sizeof(int));
    __atomic_thread_fence(__ATOMIC_RELEASE);
    set_resident(e, batch, off, max_n, true);
    e->up_pending = false;
    e->zc = true;
    return PP_OK;
}

int pp_upload_points_async(pp_handle e, const float* points_pinned, const int32_t* frame_offsets, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    if (frame_offsets && batch >= 1 && frame_offsets[batch] > 0 && !points_pinned)
        return fail(e, PP_ERR_ARG, "pp_upload_points_async: points is NULL");
    if (frame_offsets && batch >= 1 && batch <= ZC_MAX_BATCH) {
        st = feed_zero_copy(e, points_pinned, frame_offsets, batch);
        if (st != PP_ERR_UNSUPPORTED) return st;      // (not device-mapped memory: the copy below still works)
    }
    // on the copy stream, into the input buffer the running pass is not reading: no wait here, and the DMA runs
    // beside this handle's own kernels; pp_detect_async orders itself behind ev_up
    st = set_offsets(e, frame_offsets, batch, e->copy_stream); if (st) return st;
    const size_t n = (size_t)frame_offsets[batch];
    if (n) HIPCHK(e, hipMemcpyAsync(e->d_points, points_pinned, n * e->F * sizeof(float), hipMemcpyHostToDevice, e->copy_stream));
    return finish_async_upload(e, batch);
}

int pp_host_alloc(int64_t bytes, void** out) {
    if (!out || bytes < 0) return fail(nullptr, PP_ERR_ARG, "pp_host_alloc: bad argument");
    *out = nullptr;
    if (hipHostMalloc(out, (size_t)(bytes ? bytes : 1)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(nullptr, PP_ERR_HIP, "pp_host_alloc: hipHostMalloc(%lld) failed", (long long)bytes);
    }
    void* dp = nullptr;   // registered for the zero-copy feed only when the device sees the block at the same address
    if (hipHostGetDevicePointer(&dp, *out, 0) == hipSuccess && dp == *out) {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned[(uintptr_t)*out] = (size_t)(bytes ? bytes : 1);
    } else {
        (void)hipGetLastError();
    }
    return PP_OK;
}

int pp_host_free(void* p) {
    if (p) {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        g_pinned.erase((uintptr_t)p);
    }
    if (p && hipHostFree(p) != hipSuccess) return fail(nullptr, PP_ERR_HIP, "pp_host_free: hipHostFree failed");
    return PP_OK;
}

int pp_upload_points_device(pp_handle e, const void* points_dev, const int32_t* frame_offsets, int32_t batch,
                            void* producer_stream) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    st = set_offsets(e, frame_offsets, batch, e->stream); if (st) return st;
    e->up_pending = false;
    const size_t n = (size_t)frame_offsets[batch];
    if (n && !points_dev) return fail(e, PP_ERR_ARG, "pp_upload_points_device: points is NULL");
    if (producer_stream != nullptr) {
        // the copy must not start before the work queued on the producer's stream has written the points
        HIPCHK(e, hipEventRecord(e->ev_in, (hipStream_t)producer_stream));
        HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_in, 0));
    }
    if (n) HIPCHK(e, hipMemcpyAsync(e->d_points, points_dev, n * e->F * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return PP_OK;
}
int pp_current_batch(pp_handle e, int32_t* uploaded, int32_t* results) {
    if (!e) return PP_ERR_ARG;
    if (uploaded) *uploaded = e->cur_batch;
    if (results) *results = e->results_batch;
    return PP_OK;
}

int pp_set_calib(pp_handle e, const float* rect, const float* trv2c, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    if (!rect || !trv2c) return fail(e, PP_ERR_ARG, "pp_set_calib: NULL argument");
    std::vector<float> M((size_t)batch * 16);
    for (int b = 0; b < batch; ++b) calib_matrix(rect + (size_t)b * 16, trv2c + (size_t)b * 16, M.data() + (size_t)b * 16);
    HIPCHK(e, hipMemcpy(e->d_calib, M.data(), M.size() * sizeof(float), hipMemcpyHostToDevice));
    return PP_OK;
}

static void graph_invalidate(pp_engine* e) {
    // a replay of one of these graphs may still be running on the stream: its kernarg / node storage must
    // outlive it
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    for (auto& g : e->graphs) {
        destroy_exec(&g.exec);
        g = pp_engine::GraphSlot();
    }
}

// The only launch parameters that depend on the frames' point counts are k_cell_first's grid and the
// LDS-vs-global choice of the voxeliser, both functions of max(points per frame): a graph is keyed by that
// maximum rounded up to 4096 (the kernels bound-check every frame against its own count), so batches of
// similar size share one graph.
}  // extern "C"
int graph_bucket(const pp_engine* e, int max_n) {
    int b = ((max_n + 4095) / 4096) * 4096;
    if (b < 4096) b = 4096;
    return b < e->cfg.max_points_per_frame ? b : e->cfg.max_points_per_frame;
}

void drop_detect_graphs(pp_engine* e) { graph_invalidate(e); }

// the whole fused pipeline of one batch, enqueued on e->stream (plain launches or under stream capture)
static int enqueue_detect(pp_engine* e, int B, int max_n) {
    int st;
    if (!e->vox_ahead && (st = run_voxelize(e, B, max_n))) return st;
    if ((st = run_pfn(e, B, false, nullptr, true))) return st;
    if (!e->mask_in_pfn && (st = run_anchor_mask(e, B))) return st;
    if ((st = run_backbone(e, B))) return st;
    // the post-process stores its few kept detections per frame straight into the page-locked result buffers
    if ((st = run_post(e, B, true))) return st;
    return e->rule.track ? run_track(e, B) : PP_OK;
}

// The soft parameters count only while the soft rule runs: in the other modes the key carries fixed values, so changing
// sigma there costs neither a capture nor an LRU slot.
static DetectKey detect_key(const pp_engine* e, int B, int bucket) {
    DetectKey k;
    k.batch = B; k.bucket = bucket; k.buf = e->in_buf; k.zc = e->zc ? 1 : 0; k.vox = e->vox_ahead ? 1 : 0;
    k.rule = e->rule;
    if (k.rule.nms_mode != PP_NMS_SOFT) { k.rule.soft_method = 0; k.rule.soft_sigma = k.rule.soft_floor = 0.f; }
    return k;
}

bool capture_exec(pp_engine* e, const std::function<int()>& enqueue, hipGraphExec_t* out, int* enqueue_status) {
    *out = nullptr;
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(e->stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    const int st = ok ? enqueue() : PP_ERR_HIP;
    if (ok && hipStreamEndCapture(e->stream, &g) != hipSuccess) { ok = false; g = nullptr; }
    ok = ok && st == PP_OK && g != nullptr && hipGraphInstantiate(out, g, nullptr, nullptr, 0) == hipSuccess;
    if (g) (void)hipGraphDestroy(g);
    if (!ok) { *out = nullptr; (void)hipGetLastError(); }
    if (enqueue_status) *enqueue_status = st;
    return ok;
}

extern "C" {

int pp_detect_async(pp_handle e) {
    if (!e) return PP_ERR_ARG;
    if (!e->weights_ready) return fail(e, PP_ERR_STATE, "pp_detect_async: weights not finalised");
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_detect_async: anchors not set");
    if (e->cur_batch < 1) return fail(e, PP_ERR_STATE, "pp_detect_async: no frames uploaded");
    if (int st = track_check_pass(e)) return st;
    (void)hipSetDevice(e->device);
    const int B = e->cur_batch;
    prof_reset(e);
    // the frames were uploaded (and voxelised) on the copy stream (outside any capture: the event is not part of the graph)
    if (int st = wait_for_upload(e, e->stream)) return st;
    // (a graph replay voxelises without passing run_voxelize.  A second pass over the same upload -- Engine.detect's
    // float32 retry -- either voxelises here again, flagged the same way, or, vox_ahead, reads only the products of
    // set in_buf, which no later copy-stream voxeliser writes before ev_read[in_buf])
    if (!e->vox_ahead) e->main_vox_pending = true;
    // ~35 launches per batch replay as ONE graph launch: every kernel argument is a device pointer or a
    // per-(batch, max points) constant, so the captured graph is reusable until either changes (profiling
    // needs the per-launch events and uses plain launches)
    bool launched = false;
    if (e->prof <= 0 && e->graph_state == 0 && graphs_enabled(e)) {
        const DetectKey key = detect_key(e, B, graph_bucket(e, e->cur_max_n));
        pp_engine::GraphSlot* slot = nullptr;
        pp_engine::GraphSlot* lru = &e->graphs[0];
        for (auto& g : e->graphs) {
            if (g.exec && g.key == key) slot = &g;
            if (g.used < lru->used) lru = &g;
        }
        if (slot == nullptr) {
            slot = lru;
            if (slot->exec) {
                // LRU eviction: the evicted graph may still be replaying (pp_detect_async does not wait)
                HIPCHK(e, hipStreamSynchronize(e->stream));
                destroy_exec(&slot->exec);
            }
            *slot = pp_engine::GraphSlot();
            if (capture_exec(e, [&] { return enqueue_detect(e, B, key.bucket); }, &slot->exec, nullptr)) slot->key = key;
            else e->graph_state = -1;          // fall back to plain launches for the life of the handle
        }
        if (slot->exec != nullptr) {
            slot->used = ++e->graph_tick;
            HIPCHK(e, hipGraphLaunch(slot->exec, e->stream));
            launched = true;
        }
    }
    if (!launched)
        if (int st = enqueue_detect(e, B, e->cur_max_n)) return st;
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    e->results_batch = B;
    e->results_gen = e->resident_gen;
    e->results_buf = e->in_buf;
    e->proj.results = e->rule.proj ? B : 0;
    e->results_rows = det_rows(e);
    e->trk.results = e->rule.track ? B : 0;
    e->trk.from_pass = true;
    return PP_OK;
}

int pp_sync(pp_handle e) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

// k_postprocess flags a frame whose head maps hold a non-finite value in bit PP_NDETS_NONFINITE of its count
}  // extern "C"
int check_numeric(pp_engine* e, const int* n_dets, int B, const char* who) {
    int bad = 0, first = -1;
    for (int b = 0; b < B; ++b)
        if (n_dets[b] & PP_NDETS_NONFINITE) { if (first < 0) first = b; ++bad; }
    if (!bad) return PP_OK;
    return fail(e, PP_ERR_NUMERIC, "%s: non-finite head outputs in %d of %d frames (first: frame %d); %s", who, bad, B, first,
                e->force_f32 ? "the network overflows float32 on these inputs"
                             : "an activation left the range of the float16 operand pieces (|x| < 65504): "
                               "pp_set_gemm_precision(h, PP_PREC_F32) and run the frames again");
}
extern "C" {

int pp_set_gemm_precision(pp_handle e, int32_t precision) {
    if (!e) return PP_ERR_ARG;
    if (precision != PP_PREC_SPLIT_F16 && precision != PP_PREC_F32) return fail(e, PP_ERR_ARG, "pp_set_gemm_precision: unknown precision %d", precision);
    const bool f32 = precision == PP_PREC_F32;
    if (f32 == e->force_f32) return PP_OK;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_gemm_precision: a training step is in flight");
    e->force_f32 = f32;
    if (!e->weights_ready) return PP_OK;
    if (e->pub.live) return publish_reapply(e);   // published weights: re-derived from their folded arrays, on the device
    return pp_finalize_weights(e);       // waits for the stream, drops the graphs, rebuilds the device weights
}

int pp_set_cache_budget(pp_handle e, int32_t megabytes) {
    if (!e) return PP_ERR_ARG;
    if (megabytes < 0) return fail(e, PP_ERR_ARG, "pp_set_cache_budget: negative budget");
    if (megabytes == e->cache_budget_mb) return PP_OK;
    (void)hipSetDevice(e->device);
    graph_invalidate(e);          // the captured passes hold the old launch plan
    e->cache_budget_mb = megabytes;
    return PP_OK;
}

int pp_get_gemm_precision(pp_handle e, int32_t* precision) {
    if (!e || !precision) return PP_ERR_ARG;
    *precision = e->force_f32 ? PP_PREC_F32 : PP_PREC_SPLIT_F16;
    return PP_OK;
}

int pp_get_detections(pp_handle e, pp_detection* dets, int32_t* n_dets) {
    if (!e) return PP_ERR_ARG;
    if (!dets || !n_dets) return fail(e, PP_ERR_ARG, "pp_get_detections: NULL argument");
    const int B = e->results_batch;
    if (B < 1) return fail(e, PP_ERR_STATE, "pp_get_detections: no pp_detect_async results on this handle (or a stage call has reused the buffers)");
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));   // immediate after pp_sync; never hands out a half-written buffer
    // the kept detections of every frame, zeros behind them (the kernel writes only what it keeps)
    if (e->results_rows != det_rows(e))
        return fail(e, PP_ERR_STATE, "pp_get_detections: the last pass ran in the other class mode (pp_set_class_nms): run a new one");
    const size_t pm = (size_t)e->results_rows;    // row stride of that pass: nms_post_max_size, or num_class times that
    if (int st = check_numeric(e, e->h_ndets, B, "pp_get_detections")) return st;
    for (int b = 0; b < B; ++b) {
        size_t n = (size_t)std::max(0, std::min(e->h_ndets[b], (int)pm));
        memcpy(dets + (size_t)b * pm, e->h_dets + (size_t)b * pm, n * sizeof(pp_detection));
        memset(dets + (size_t)b * pm + n, 0, (pm - n) * sizeof(pp_detection));
    }
    memcpy(n_dets, e->h_ndets, (size_t)B * sizeof(int));
    return PP_OK;
}

int pp_detect(pp_handle e, const float* points, const int32_t* frame_offsets, int32_t batch, const float* rect,
              const float* trv2c, pp_detection* dets, int32_t* n_dets) {
    int st;
    if ((st = pp_upload_points(e, points, frame_offsets, batch))) return st;
    if (rect && trv2c && (st = pp_set_calib(e, rect, trv2c, batch))) return st;
    if ((st = pp_detect_async(e))) return st;
    if ((st = pp_sync(e))) return st;
    return pp_get_detections(e, dets, n_dets);
}

int pp_points_to_voxel(pp_handle e, const float* points, int64_t n, float* voxels, int32_t* coors,
                       int32_t* num_points, int32_t* n_pillars) {
    if (!e) return PP_ERR_ARG;
    if (!voxels || !coors || !num_points || !n_pillars) return fail(e, PP_ERR_ARG, "pp_points_to_voxel: NULL output");
    if (n < 0 || n > e->NMAX) return fail(e, PP_ERR_ARG, "pp_points_to_voxel: n=%lld outside [0, max_points_per_frame=%d]", (long long)n, e->NMAX);
    (void)hipSetDevice(e->device);
    const int32_t off[2] = {0, (int32_t)n};
    int st = pp_upload_points(e, points, off, 1); if (st) return st;
    prof_reset(e);
    if ((st = run_voxelize(e, 1, (int)n))) return st;
    const size_t MV = (size_t)e->cfg.max_voxels;
    if ((st = dgrow(e, &e->d_voxels, &e->cap_voxels, MV * e->T * e->F))) return st;
    if ((st = dgrow(e, &e->d_numpts, &e->cap_numpts, MV))) return st;
    if ((st = dgrow(e, &e->d_coors, &e->cap_coors, MV * 4))) return st;
    launch_voxel_expand(e->d_points_sorted, e->d_offsets, sorted_idx(e), e->d_pstart, e->d_pcell, e->d_npillars, 0, e->F,
                        e->T, e->cfg.max_voxels, e->ny, e->nx, e->d_voxels, e->d_coors, e->d_numpts, e->stream);
    HIPCHK(e, hipGetLastError());
    int P = 0;
    HIPCHK(e, hipMemcpyAsync(&P, e->d_npillars, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (P < 0 || P > e->cfg.max_voxels) return fail(e, PP_ERR_HIP, "pp_points_to_voxel: device returned %d pillars", P);
    *n_pillars = P;
    if (P) {
        HIPCHK(e, hipMemcpy(voxels, e->d_voxels, (size_t)P * e->T * e->F * sizeof(float), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(coors, e->d_coors, (size_t)P * 3 * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(num_points, e->d_numpts, (size_t)P * sizeof(int), hipMemcpyDeviceToHost));
    }
    stage_call_done(e);
    return PP_OK;
}

static int upload_coors(pp_engine* e, const int32_t* coors, int64_t P, int32_t batch, const char* who) {
    for (int64_t p = 0; p < P; ++p) {
        const int32_t* c = coors + p * 4;
        if (c[0] < 0 || c[0] >= batch || c[1] < 0 || c[1] >= e->nz || c[2] < 0 || c[2] >= e->ny || c[3] < 0 || c[3] >= e->nx)
            return fail(e, PP_ERR_ARG, "%s: coors[%lld] = (%d,%d,%d,%d) outside batch=%d / grid z%d y%d x%d", who,
                        (long long)p, c[0], c[1], c[2], c[3], batch, e->nz, e->ny, e->nx);
    }
    int st = dgrow(e, &e->d_coors, &e->cap_coors, (size_t)P * 4); if (st) return st;
    if (P) HIPCHK(e, hipMemcpyAsync(e->d_coors, coors, (size_t)P * 4 * sizeof(int), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemsetAsync(e->d_cellmap, 0xff, (size_t)batch * e->ncell * sizeof(int), e->stream));
    launch_build_cellmap(e->d_coors, P, e->ncell, e->ny, e->nx, e->d_cellmap, e->stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

int pp_anchor_mask(pp_handle e, const int32_t* coors, int64_t num_pillars, int32_t batch, uint8_t* mask) {
    if (!e) return PP_ERR_ARG;
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_anchor_mask: anchors not set");
    if ((num_pillars && !coors) || !mask || num_pillars < 0) return fail(e, PP_ERR_ARG, "pp_anchor_mask: bad argument");
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    if ((st = upload_coors(e, coors, num_pillars, batch, "pp_anchor_mask"))) return st;
    prof_reset(e);
    // the cell map was built from the caller's coordinates; an occupancy bitmap is what the last pass's PFN launch left
    e->occbits_live = false;
    if ((st = run_anchor_mask(e, batch))) return st;
    HIPCHK(e, hipMemcpyAsync(mask, e->d_mask, (size_t)batch * e->A, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    stage_call_done(e);
    return PP_OK;
}

int pp_forward_voxels(pp_handle e, const float* voxels, const int32_t* num_points, const int32_t* coors,
                      int64_t P, int32_t batch, float* box_preds, float* cls_preds, float* dir_cls_preds,
                      float* pillar_features, float* canvas) {
    if (!e) return PP_ERR_ARG;
    if (!e->weights_ready) return fail(e, PP_ERR_STATE, "pp_forward_voxels: weights not finalised");
    if (P < 0 || (P && (!voxels || !num_points || !coors)) || !box_preds || !cls_preds || (e->use_dir && !dir_cls_preds))
        return fail(e, PP_ERR_ARG, "pp_forward_voxels: NULL argument");
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    for (int64_t p = 0; p < P; ++p)
        if (num_points[p] < 1 || num_points[p] > e->T)
            return fail(e, PP_ERR_ARG, "pp_forward_voxels: num_points[%lld]=%d outside [1,%d]", (long long)p, num_points[p], e->T);
    if ((st = upload_coors(e, coors, P, batch, "pp_forward_voxels"))) return st;
    if ((st = dgrow(e, &e->d_voxels, &e->cap_voxels, (size_t)P * e->T * e->F))) return st;
    if ((st = dgrow(e, &e->d_numpts, &e->cap_numpts, (size_t)P))) return st;
    if (pillar_features && (st = dgrow(e, &e->d_feat, &e->cap_feat, (size_t)P * e->C))) return st;
    if (P) {
        HIPCHK(e, hipMemcpyAsync(e->d_voxels, voxels, (size_t)P * e->T * e->F * sizeof(float), hipMemcpyHostToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->d_numpts, num_points, (size_t)P * sizeof(int), hipMemcpyHostToDevice, e->stream));
    }
    prof_reset(e);
    if ((st = run_pfn(e, batch, true, pillar_features ? e->d_feat : nullptr))) return st;
    if ((st = run_backbone(e, batch))) return st;
    if ((st = fetch_heads(e, batch, box_preds, cls_preds, dir_cls_preds))) return st;
    if (pillar_features && P)
        HIPCHK(e, hipMemcpyAsync(pillar_features, e->d_feat, (size_t)P * e->C * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (canvas && (st = fetch_canvas(e, canvas, batch, e->in_buf))) return st;
    stage_call_done(e);
    return PP_OK;
}

int pp_predict(pp_handle e, const float* box_preds, const float* cls_preds, const float* dir_cls_preds,
               const uint8_t* anchors_mask, const float* rect, const float* trv2c, int32_t batch,
               pp_detection* dets, int32_t* n_dets) {
    if (!e) return PP_ERR_ARG;
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_predict: anchors not set");
    if (!box_preds || !cls_preds || (e->use_dir && !dir_cls_preds) || !anchors_mask || !rect || !trv2c || !dets || !n_dets)
        return fail(e, PP_ERR_ARG, "pp_predict: NULL argument");
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    if ((st = pp_set_calib(e, rect, trv2c, batch))) return st;
    if ((st = upload_heads(e, batch, box_preds, cls_preds, dir_cls_preds))) return st;
    HIPCHK(e, hipMemcpyAsync(e->d_mask, anchors_mask, (size_t)batch * e->A, hipMemcpyHostToDevice, e->stream));
    prof_reset(e);
    if ((st = run_post(e, batch))) return st;
    const size_t rows = (size_t)det_rows(e);
    HIPCHK(e, hipMemcpyAsync(dets, e->d_dets, (size_t)batch * rows * sizeof(pp_detection), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(n_dets, e->d_ndets, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    if (e->rule.proj)
        HIPCHK(e, hipMemcpyAsync(e->proj.h_bbox, e->proj.d_bbox, (size_t)batch * rows * 4 * sizeof(double), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    stage_call_done(e);
    if (e->rule.proj) {      // pp_get_bboxes reads the counts beside the boxes (flags included: it reports PP_ERR_NUMERIC too)
        memcpy(e->h_ndets, n_dets, (size_t)batch * sizeof(int));
        e->proj.results = batch;
        e->results_rows = (int)rows;
    }
    // non-finite predictions: the reference's predict() would hand NaN boxes on (np.argpartition over NaN scores);
    // this one says so instead (documented deviation)
    if ((st = check_numeric(e, n_dets, batch, "pp_predict"))) {
        for (int b = 0; b < batch; ++b) n_dets[b] = 0;
        return st;
    }
    return PP_OK;
}

int pp_fetch_intermediates(pp_handle e, int32_t* n_pillars, int32_t* coors, int32_t* num_points,
                           uint8_t* anchors_mask, float* box_preds, float* cls_preds, float* dir_cls_preds,
                           float* canvas) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    const int B = e->results_batch;
    if (B < 1) return fail(e, PP_ERR_STATE, "pp_fetch_intermediates: no fused-path pass to tap (run pp_detect / pp_detect_async first)");
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const int MV = e->cfg.max_voxels;
    std::vector<int> np(B);
    const pp_engine::VoxSet& vs = e->vox[e->results_buf];      // the set that pass read (a later upload has flipped the d_* members)
    HIPCHK(e, hipMemcpy(np.data(), vs.npillars, B * sizeof(int), hipMemcpyDeviceToHost));
    if (n_pillars) memcpy(n_pillars, np.data(), B * sizeof(int));
    if (coors || num_points) {
        std::vector<int> pcell((size_t)B * MV), pstart((size_t)B * (MV + 1));
        HIPCHK(e, hipMemcpy(pcell.data(), vs.pcell, pcell.size() * sizeof(int), hipMemcpyDeviceToHost));
        HIPCHK(e, hipMemcpy(pstart.data(), vs.pstart, pstart.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < B; ++b)
            for (int p = 0; p < np[b]; ++p) {
                const size_t r = (size_t)b * MV + p;
                if (coors) {
                    const int c = pcell[r];
                    coors[r * 3 + 0] = c / (e->nx * e->ny);
                    coors[r * 3 + 1] = (c / e->nx) % e->ny;
                    coors[r * 3 + 2] = c % e->nx;
                }
                if (num_points) {
                    const int cnt = pstart[(size_t)b * (MV + 1) + p + 1] - pstart[(size_t)b * (MV + 1) + p];
                    num_points[r] = cnt < e->T ? cnt : e->T;
                }
            }
    }
    if (anchors_mask) HIPCHK(e, hipMemcpy(anchors_mask, e->d_mask, (size_t)B * e->A, hipMemcpyDeviceToHost));
    if (box_preds || cls_preds || dir_cls_preds) {
        int st = fetch_heads(e, B, box_preds, cls_preds, dir_cls_preds);
        if (st) return st;
    }
    if (canvas) { int stc = fetch_canvas(e, canvas, B, e->results_buf); if (stc) return stc; }
    return PP_OK;
}

int pp_set_profiling(pp_handle e, int32_t level) {
    if (!e) return PP_ERR_ARG;
    e->prof = level > 0 ? 1 : 0;
    return PP_OK;
}

int pp_get_kernel_times(pp_handle e, int32_t capacity, const char** names, float* ms, int32_t* count) {
    if (!e) return PP_ERR_ARG;
    if (!count) return fail(e, PP_ERR_ARG, "pp_get_kernel_times: NULL count");
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    const int n = (int)e->ktimes.size();
    *count = n;
    for (int i = 0; i < n && i < capacity; ++i) {
        float t = 0.f;
        HIPCHK(e, hipEventElapsedTime(&t, e->events[e->ktimes[i].ev], e->events[e->ktimes[i].ev + 1]));
        if (names) names[i] = e->ktimes[i].name;
        if (ms) ms[i] = t;
    }
    return PP_OK;
}

int pp_timer_start(pp_handle e) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipEventRecord(e->t0, e->stream));
    return PP_OK;
}

int pp_timer_stop(pp_handle e, float* elapsed_ms) {
    if (!e) return PP_ERR_ARG;
    if (!elapsed_ms) return fail(e, PP_ERR_ARG, "pp_timer_stop: NULL argument");
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipEventRecord(e->t1, e->stream));
    HIPCHK(e, hipEventSynchronize(e->t1));
    HIPCHK(e, hipEventElapsedTime(elapsed_ms, e->t0, e->t1));
    return PP_OK;
}

int pp_layer_count(pp_handle e, int32_t* count) {
    if (!e || !count) return PP_ERR_ARG;
    *count = (int32_t)e->layers.size();
    return PP_OK;
}

const char* pp_layer_tag(pp_handle e, int32_t layer) {
    if (!e || layer < 0 || layer >= (int)e->layer_tags.size()) return "";
    refresh_tags(e, e->cur_batch > 0 ? e->cur_batch : e->B);
    return e->layer_tags[layer].c_str();
}

int pp_plan_layer_name(const pp_layer_plan_desc* layer, int32_t batch, int32_t compute_units, char* name, int32_t name_capacity) {
    if (!layer || !name || name_capacity < 1 || batch < 1 || compute_units < 1) return PP_ERR_ARG;
    if (layer->kind != LAYER_SEP && layer->kind != LAYER_DECONV && layer->kind != LAYER_HEAD) return PP_ERR_ARG;
    static float pieces;                 // what the planner asks of the weight pointers is only whether they are NULL
    static int cells;
    LayerDesc L;
    memset(&L, 0, sizeof(L));
    L.kind = layer->kind; L.cin = layer->cin; L.cout = layer->cout; L.n_total = layer->n_total;
    L.stride = layer->stride; L.k = layer->k;
    L.in_h = layer->in_h; L.in_w = layer->in_w; L.out_h = layer->out_h; L.out_w = layer->out_w;
    L.head_mode = layer->head_mode;
    L.d_wt16 = layer->has_wt16 ? &pieces : nullptr;
    L.d_head_wt16 = layer->has_head_wt16 ? &pieces : nullptr;
    L.d_occ = layer->sparse_input ? &cells : nullptr;
    PlanEnv env;
    env.cus = compute_units;
    env.sw = pp_switches();
    const std::string n = layer_plan_name(L, batch, env);
    if ((int)n.size() + 1 > name_capacity) return PP_ERR_ARG;
    memcpy(name, n.c_str(), n.size() + 1);
    return PP_OK;
}

int pp_bench_layer(pp_handle e, int32_t layer, int32_t batch, int32_t reps, int32_t ablate, float* avg_ms) {
    if (!e) return PP_ERR_ARG;
    if (!avg_ms || reps < 1 || layer < 0 || layer >= (int)e->layers.size()) return fail(e, PP_ERR_ARG, "pp_bench_layer: bad argument");
    if (ablate != 0) return fail(e, PP_ERR_ARG, "pp_bench_layer: ablate must be 0 (the kernel ablation bits were removed)");
    if (!e->weights_ready) return fail(e, PP_ERR_STATE, "pp_bench_layer: weights not finalised");
    (void)hipSetDevice(e->device);
    int st = check_batch(e, batch); if (st) return st;
    const LayerDesc& L = e->layers[layer];
    for (int i = 0; i < 2; ++i)
        if ((st = launch_layer(L, batch, e->d_head, e->stream, e->plan_env))) return fail(e, st, "pp_bench_layer: unsupported layer");
    HIPCHK(e, hipEventRecord(e->t0, e->stream));
    for (int i = 0; i < reps; ++i) launch_layer(L, batch, e->d_head, e->stream, e->plan_env);
    HIPCHK(e, hipEventRecord(e->t1, e->stream));
    HIPCHK(e, hipEventSynchronize(e->t1));
    HIPCHK(e, hipGetLastError());
    float ms = 0.f;
    HIPCHK(e, hipEventElapsedTime(&ms, e->t0, e->t1));
    *avg_ms = ms / reps;
    return PP_OK;
}

int pp_stream(pp_handle e, void** stream) {
    if (!e) return PP_ERR_ARG;
    if (!stream) return fail(e, PP_ERR_ARG, "pp_stream: stream is NULL");
    *stream = (void*)e->stream;
    return PP_OK;
}

int pp_device_mem_free(pp_handle e, int64_t* free_bytes) {
    if (!e || !free_bytes) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    size_t fr = 0, tot = 0;
    HIPCHK(e, hipMemGetInfo(&fr, &tot));
    *free_bytes = (int64_t)fr;
    return PP_OK;
}

// measurement helper: device-to-device copy rate on the handle's stream (the bench states the HBM figure it
// measured in the run beside the spec constant its roofline fractions use)
int pp_device_copy_bench(pp_handle e, int64_t bytes, int32_t reps, float* gbytes_per_s) {
    if (!e || !gbytes_per_s || bytes <= 0 || reps <= 0) return fail(e, PP_ERR_ARG, "pp_device_copy_bench: bad argument");
    (void)hipSetDevice(e->device);
    void *src = nullptr, *dst = nullptr;
    if (hipMalloc(&src, (size_t)bytes) != hipSuccess || hipMalloc(&dst, (size_t)bytes) != hipSuccess) {
        if (src) (void)hipFree(src);
        (void)hipGetLastError();
        return fail(e, PP_ERR_HIP, "pp_device_copy_bench: hipMalloc(2 x %lld) failed", (long long)bytes);
    }
    int st = PP_OK;
    float ms = 0.f;
    if (hipMemsetAsync(src, 1, (size_t)bytes, e->stream) != hipSuccess ||
        hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, e->stream) != hipSuccess ||     // warm-up
        hipEventRecord(e->t0, e->stream) != hipSuccess) st = PP_ERR_HIP;
    for (int i = 0; i < reps && st == PP_OK; ++i)
        if (hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDeviceToDevice, e->stream) != hipSuccess) st = PP_ERR_HIP;
    if (st == PP_OK && (hipEventRecord(e->t1, e->stream) != hipSuccess || hipEventSynchronize(e->t1) != hipSuccess ||
                        hipEventElapsedTime(&ms, e->t0, e->t1) != hipSuccess)) st = PP_ERR_HIP;
    (void)hipStreamSynchronize(e->stream);
    (void)hipFree(src);
    (void)hipFree(dst);
    if (st != PP_OK) { (void)hipGetLastError(); return fail(e, st, "pp_device_copy_bench: copy failed"); }
    *gbytes_per_s = (float)(2.0 * (double)bytes * reps / (ms * 1e-3) / 1e9);   // read + write
    return PP_OK;
}

int pp_device_info(pp_handle e, char* name, int32_t name_capacity, int32_t* compute_units, int64_t* hbm_bytes) {
    if (!e) return PP_ERR_ARG;
    hipDeviceProp_t prop;
    HIPCHK(e, hipGetDeviceProperties(&prop, e->device));
    if (name && name_capacity > 0) {
        snprintf(name, (size_t)name_capacity, "%s (%s)", prop.name, prop.gcnArchName);
    }
    if (compute_units) *compute_units = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return PP_OK;
}

}  // extern "C"
