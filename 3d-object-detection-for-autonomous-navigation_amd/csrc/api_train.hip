// C-ABI, training: the head loss (loss.hip), the training step (train.hip) with its graph cache
// and its fused variants (targets, augmentation, GT sampling: api_dataprep.hip's enqueue_*), the AdamW update (optim.hip),
// gradient clipping and the non-finite guard in front of it (grad_clip.hip).
#include "pp_engine.h"

int ensure_loss_buffers(pp_engine* e) {
    pp_engine::Loss& l = e->loss;
    if (l.head_grad) return PP_OK;
    const size_t B = (size_t)e->B, npx = (size_t)e->head_h * e->head_w;
    DevAlloc A{e};
    A(&l.labels, B * e->A); A(&l.regt, B * e->A * 7); A(&l.npos, B); A(&l.partials, B * loss_blocks((int)npx) * 5);
    A(&l.out, (size_t)8); A(&l.head_grad, B * npx * PP_HEAD_COLS);      // (head_grad last: it is the group's ready flag)
    return A.st;
}

namespace {

void fill_loss_params(pp_engine* e, const pp_loss_config* lc, int batch, LossParams& p) {
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.A = e->A; p.npx = e->head_h * e->head_w; p.napl = e->napl; p.ncls = e->ncls;
    p.head = e->d_head; p.labels = e->loss.labels; p.reg_targets = e->loss.regt; p.anchors = e->d_anchors;
    p.npos = e->loss.npos; p.partials = e->loss.partials; p.losses = e->loss.out;
    p.alpha = lc->alpha; p.gamma = lc->gamma; p.sigma = lc->sigma;
    for (int i = 0; i < 7; ++i) p.code_weight[i] = lc->code_weight[i];
    p.pos_cls_weight = lc->pos_class_weight; p.neg_cls_weight = lc->neg_class_weight;
    p.cls_weight = lc->classification_weight; p.loc_weight = lc->localization_weight; p.dir_weight = lc->direction_loss_weight;
    p.norm_by_num_positives = lc->norm_by_num_positives; p.encode_rad_error_by_sin = lc->encode_rad_error_by_sin;
    p.use_direction = lc->use_direction_classifier;
}

int train_state(pp_engine* e) {
    if (e->train) return PP_OK;
    auto* t = new pp_engine::TrainState();
    TrainShape& s = t->shape;
    s.nx = e->nx; s.ny = e->ny; s.nz = e->nz; s.C = e->C; s.F = e->F; s.FA = e->FA; s.T = e->T;
    s.max_voxels = e->cfg.max_voxels; s.with_dist = e->with_dist ? 1 : 0;
    s.vx = (float)e->cfg.voxel_size[0]; s.vy = (float)e->cfg.voxel_size[1];
    s.x_off = (float)(e->cfg.voxel_size[0] / 2 + e->cfg.pc_range[0]);
    s.y_off = (float)(e->cfg.voxel_size[1] / 2 + e->cfg.pc_range[1]);
    s.head_h = e->head_h; s.head_w = e->head_w; s.napl = e->napl; s.ncls = e->ncls; s.use_dir = e->use_dir ? 1 : 0;
    s.CC = e->CC;
    s.layers = e->layers;
    t->plan = train_plan(s, e->B);
    e->train = t;
    return PP_OK;
}

int train_buffers(pp_engine* e) {
    pp_engine::TrainState* t = e->train;
    if (t->buffers) return PP_OK;
    const TrainShape& s = t->shape;
    TrainCtx& cx = t->cx;
    const size_t B = (size_t)e->B, HW = (size_t)s.head_h * s.head_w;
    int st = PP_OK;
    auto A1 = [&](int r) { if (st == PP_OK) st = r; };
    A1(dalloc(e, &cx.pfn_feat, B * s.max_voxels * s.C));
    A1(dalloc(e, &cx.pfn_arg, B * s.max_voxels * s.C));
    A1(dalloc(e, &cx.pfn_stats, (size_t)2 * s.C));
    A1(dalloc(e, &cx.pfn_sums, (size_t)2 * s.C));
    A1(dalloc(e, &cx.pfn_nrows, (size_t)1));
    A1(dalloc(e, &cx.pfn_prefix, B + 1));
    A1(dalloc(e, &cx.pfn_rec, B * s.max_voxels * 3));
    // maps the fused forward kernel reads through a 3x3 window carry a PP_ZPAD_FLOATS header in front, the padding of
    // the convolution: NaN-filled for the pre-BatchNorm maps (relu(NaN * sc + sh) evaluates to 0 on the vector unit,
    // launch_sep_train), zero-filled for the tensors read as they are (canvas, block-final activations)
    auto dalloc_hdr = [&](float** p, size_t count, int fill = 0xff) -> int {
        float* raw = nullptr;
        int r = dalloc(e, &raw, count + PP_ZPAD_FLOATS);
        if (r == PP_OK && hipMemset(raw, fill, PP_ZPAD_FLOATS * sizeof(float)) != hipSuccess) r = PP_ERR_HIP;
        *p = raw ? raw + PP_ZPAD_FLOATS : nullptr;
        return r;
    };
    A1(dalloc_hdr(&cx.canvas, B * s.ny * s.nx * s.C, 0));
    A1(dalloc(e, &cx.dcanvas, B * s.ny * s.nx * s.C));
    const TrainPlan& plan = t->plan;
    cx.lbuf.assign(plan.layers.size(), TrainLayerBuf{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr});
    for (size_t j = 0; j < plan.layers.size(); ++j) {
        const LayerDesc& l = s.layers[plan.layers[j].layer];
        TrainLayerBuf& tb = cx.lbuf[j];
        if (l.kind == LAYER_SEP) {
            const size_t rows = B * l.out_h * l.out_w;
            A1(dalloc(e, &tb.D, rows * l.cin)); A1(dalloc_hdr(&tb.Z, rows * l.cout));
            if (plan.layers[j].keeps_a) A1(dalloc_hdr(&tb.A, rows * l.cout, 0));
            A1(dalloc(e, &tb.dA, rows * l.cout));
        } else {
            A1(dalloc(e, &tb.Z, B * l.in_h * l.in_w * l.k * l.k * l.cout));
        }
        A1(dalloc(e, &tb.stats, (size_t)2 * l.cout)); A1(dalloc(e, &tb.sums, (size_t)2 * l.cout));
        A1(dalloc(e, &tb.coef, (size_t)l.cout));
    }
    A1(dalloc(e, &cx.cat, B * HW * s.CC)); A1(dalloc(e, &cx.dcat, B * HW * s.CC));
    A1(dalloc(e, &cx.head_w, (size_t)s.CC * PP_HEAD_COLS)); A1(dalloc(e, &cx.head_b, (size_t)PP_HEAD_COLS));
    A1(dalloc(e, &cx.dhead_w, (size_t)s.CC * PP_HEAD_COLS)); A1(dalloc(e, &cx.dhead_b, (size_t)2 * PP_HEAD_COLS));
    A1(dalloc(e, &cx.dZ, plan.max_z)); A1(dalloc(e, &cx.dD, plan.max_d));
    A1(dalloc(e, &cx.part, plan.part_floats));
    A1(dalloc(e, &cx.stat_part, (size_t)plan.stat_part_floats));
    A1(dalloc(e, &cx.pw16, (size_t)std::max<long>(plan.pw16_words, 8)));
    A1(dalloc(e, &cx.head_w16, (size_t)2 * s.CC * PP_HEAD_COLS));
    // split-K partial tiles + the regions of the step's deferred reductions (every weight gradient keeps its
    // partials until the end of the step): 64 MB at the reference's batch, 16 MB more per frame beyond 4
    // (round 4: capped -- the deferred regions are bounded by the SHAPES, not the batch: a weight-gradient product keeps at
    // most ~1 024 partial tiles of 64 x 64 floats, a depthwise layer 512 rows of 11 * cin, about two dozen of each per
    // step; an engine created for 512 frames used to take 8.6 GB here.  Past the cap the products split less and the
    // depthwise backward falls back to the shared scratch, train.hip)
    cx.gemm_part_floats = std::min<long>(std::max<long>(16l << 20, (long)B * (4l << 20)), 192l << 20);
    A1(dalloc(e, &cx.gemm_part, (size_t)cx.gemm_part_floats));
    // PP_TRAIN_ARENA_FLOATS=n: the step uses at most n floats of it (tests: the arena-exhausted branches of train.hip).
    // Where partial rows live and how many K slices a product gets change; what is computed does not.
    cx.cus = e->plan_env.cus;
    cx.sw = e->plan_env.sw.train;
    if (const long cap = cx.sw.arena_floats) cx.gemm_part_floats = std::min(cx.gemm_part_floats, cap);
    if (st == PP_OK) st = ensure_loss_buffers(e);
    if (st == PP_OK) t->buffers = true;
    return st;
}

TrainKey train_key(const pp_engine* e, int batch, int bucket, const void* params, const void* grads, const void* state,
                   const pp_loss_config* lc) {
    TrainKey k;
    k.batch = batch; k.bucket = bucket; k.zc = e->zc ? 1 : 0;
    k.params = params; k.grads = grads; k.state = state; k.loss = *lc;
    k.frozen = e->train->plan.frozen;
    k.metrics = e->metrics.on;
    return k;
}

// pp_train_step_async and pp_train_step_gt_async: `targets` fills loss.labels / loss.regt between the two halves of
// the step (plain stream work between the two graph replays, or between the two eager halves)
int train_step_launch(pp_engine* e, const float* params_dev, float* grads_dev, float* state_dev, int32_t batch,
                      const pp_loss_config* lc, const std::function<int()>& targets,
                      const std::function<int()>& pre = nullptr) {
    if (!params_dev || !grads_dev || !state_dev || !lc)
        return fail(e, PP_ERR_ARG, "pp_train_step: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_train_step_async: the step before has not been waited for");
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_train_step: anchors not set");
    if (e->cur_batch < 1 || e->cur_batch != batch)
        return fail(e, PP_ERR_STATE, "pp_train_step: %d frames are resident, batch is %d (upload the frames first)", e->cur_batch, batch);
    if ((lc->use_direction_classifier != 0) != e->use_dir)
        return fail(e, PP_ERR_ARG, "pp_train_step: loss config and engine disagree on use_direction_classifier");
    if (!(lc->sigma > 0.f)) return fail(e, PP_ERR_ARG, "pp_train_step: sigma must be positive");
    (void)hipSetDevice(e->device);
    int st = train_state(e); if (st) return st;
    if ((st = train_buffers(e))) return st;
    if ((st = wait_for_upload(e, e->stream))) return st;   // (also a handle that served pp_detect_async passes before it trained)
    prof_reset(e);
    if (pre && (st = pre())) return st;   // plain launches ahead of the forward half (the augmentation)
    e->main_vox_pending = true;    // the step voxelises on the main stream (inside its graph, too)
    pp_engine::TrainState* t = e->train;
    TrainCtx& cx = t->cx;
    cx.stream = e->stream;
    cx.pts_sorted = e->d_points_sorted; cx.offsets = e->d_offsets; cx.pillar_start = e->d_pstart; cx.pillar_cell = e->d_pcell;
    cx.npillars = e->d_npillars; cx.cellmap = e->d_cellmap;
    cx.head = e->d_head; cx.dhead = e->loss.head_grad;
    LossParams lp;
    fill_loss_params(e, lc, batch, lp);
    cx.metrics = nullptr;
    if (e->metrics.on) {      // counted inside the second half, right behind the loss (pp_set_train_metrics)
        if ((st = ensure_metrics(e))) return st;
        fill_metrics_params(e, batch, e->metrics.step);
        cx.metrics = &e->metrics.step;
    }
    // the step in two halves: 1 = voxelise + forward, 2 = loss + backward
    auto enqueue = [&](int max_n, int phase) -> int {
        if (phase & 1) {
            int r = run_voxelize(e, batch, max_n);
            if (r) return r;
        }
        return train_step(cx, t->shape, t->plan, params_dev, grads_dev, state_dev, batch, lp, phase);
    };
    bool launched = false;
    if (e->prof <= 0 && t->graph_state == 0 && graphs_enabled(e)) {
        const int bucket = graph_bucket(e, e->cur_max_n);
        pp_engine::TrainState::Graph& tg = t->graph[e->in_buf & 1];
        const TrainKey key = train_key(e, batch, bucket, params_dev, grads_dev, state_dev, lc);
        if (!(tg.exec != nullptr && tg.exec_bwd != nullptr && tg.key == key)) {
            if (tg.exec || tg.exec_bwd) {
                HIPCHK(e, hipStreamSynchronize(e->stream));
                destroy_exec(&tg.exec); destroy_exec(&tg.exec_bwd);
            }
            bool ok = true;
            for (int phase = 1; phase <= 2 && ok; ++phase) {
                ok = capture_exec(e, [&] { return enqueue(bucket, phase); }, phase == 1 ? &tg.exec : &tg.exec_bwd, &st);
                if (st == PP_ERR_UNSUPPORTED) {      // no capture failure: graph_state stays, a forward half already built goes
                    destroy_exec(&tg.exec);
                    return fail(e, st, "pp_train_step: configuration not supported by the training kernels");
                }
            }
            if (ok) {
                tg.key = key;
                ++t->n_captures;
            } else {
                destroy_exec(&tg.exec); destroy_exec(&tg.exec_bwd);
                t->graph_state = -1;
            }
        }
        if (tg.exec != nullptr && tg.exec_bwd != nullptr) {
            HIPCHK(e, hipGraphLaunch(tg.exec, e->stream));
            if ((st = targets())) return st;
            HIPCHK(e, hipGraphLaunch(tg.exec_bwd, e->stream));
            ++t->n_replays;
            launched = true;
            st = PP_OK;
        }
    }
    if (!launched) {
        ProfScope ps(e, nullptr);
        st = enqueue(e->cur_max_n, 1);
        if (st == PP_OK) st = targets();
        if (st == PP_OK) st = enqueue(e->cur_max_n, 2);
    }
    if (st) return fail(e, st, "pp_train_step: configuration not supported by the training kernels");
    HIPCHK(e, hipGetLastError());
    if (!e->h_train_losses && hipHostMalloc((void**)&e->h_train_losses, 8 * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(e, PP_ERR_HIP, "pp_train_step: hipHostMalloc failed");
    }
    HIPCHK(e, hipMemcpyAsync(e->h_train_losses, e->loss.out, 8 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (e->metrics.on)
        HIPCHK(e, hipMemcpyAsync(e->metrics.h_counts, e->metrics.counts, PP_METRICS_COUNTS * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
    e->metrics.step_counted = e->metrics.on;
    // this input buffer (and its zero-copy descriptor) is free again once the step is through: the NEXT batch may be
    // uploaded into the other one while this step runs (pp_upload_points_async between _async and _wait)
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    e->results_batch = 0;          // the head map now holds training-mode outputs, not detections
    e->cls_plane_live = false;
    e->train_pending = true;
    t->last_batch = batch;
    return PP_OK;
}

// the synchronous pp_train_step*: launch, then wait for the losses
template <typename Launch>
int step_and_wait(pp_engine* e, const char* who, float* losses, Launch launch) {
    if (!e) return PP_ERR_ARG;
    if (!losses) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    const int st = launch();
    return st ? st : pp_train_step_wait(e, losses);
}

// pp_grad_norm_device / pp_adamw_step_clipped_device: everything the kernels index with is checked here
int check_clip_table(const char* who, int64_t n, const int64_t* segments, int32_t n_segments, const int32_t* groups,
                     int32_t n_groups, const void* workspace, bool reduce) {
    if (n < 0 || n_segments < 0 || n_groups < 1 || (n_segments > 0 && !segments))
        return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    if (!groups && n_groups != 1) return fail(nullptr, PP_ERR_ARG, "%s: groups is NULL but n_groups is %d", who, n_groups);
    for (int32_t i = 0; i < n_segments; ++i) {
        const int64_t off = segments[2 * i], size = segments[2 * i + 1];
        if (off < 0 || size < 0 || off > n || size > n - off)
            return fail(nullptr, PP_ERR_ARG, "%s: segment %d lies outside [0, %lld)", who, i, (long long)n);
        if (groups && (groups[i] < 0 || groups[i] >= n_groups))
            return fail(nullptr, PP_ERR_ARG, "%s: segment %d is in group %d of %d", who, i, groups[i], n_groups);
    }
    if (!reduce) return PP_OK;
    if (!workspace || ((uintptr_t)workspace & 7)) return fail(nullptr, PP_ERR_ARG, "%s: workspace is NULL or not 8-byte aligned", who);
    if (grad_clip_partials(segments, n_segments) > grad_clip_layout(n, n_segments, n_groups).max_partials)
        return fail(nullptr, PP_ERR_ARG, "%s: segments overlap (more partial sums than the workspace holds)", who);
    return PP_OK;
}

}  // namespace

extern "C" {

int pp_head_loss(pp_handle e, const int32_t* labels, const float* reg_targets, int32_t batch,
                 const pp_loss_config* lc, float* losses, float* head_grad) {
    if (!e) return PP_ERR_ARG;
    if (!labels || !reg_targets || !lc || !losses) return fail(e, PP_ERR_ARG, "pp_head_loss: null argument");
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_head_loss: anchors not set");
    int st = check_batch(e, batch);
    if (st) return st;
    if (!(lc->sigma > 0.f)) return fail(e, PP_ERR_ARG, "pp_head_loss: sigma must be positive");
    if ((lc->use_direction_classifier != 0) != e->use_dir)
        return fail(e, PP_ERR_ARG, "pp_head_loss: loss config and engine disagree on use_direction_classifier");
    (void)hipSetDevice(e->device);
    const size_t npx = (size_t)e->head_h * e->head_w;
    if ((st = ensure_loss_buffers(e))) return st;
    HIPCHK(e, hipMemcpyAsync(e->loss.labels, labels, (size_t)batch * e->A * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(e, hipMemcpyAsync(e->loss.regt, reg_targets, (size_t)batch * e->A * 7 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    LossParams p;
    fill_loss_params(e, lc, batch, p);
    p.head_grad = head_grad ? e->loss.head_grad : nullptr;
    {
        ProfScope ps(e, "k_loss_pixels:loss+grad", true);
        if ((st = launch_head_loss(p, e->stream))) return fail(e, st, "pp_head_loss: %d anchors per pixel x %d classes not supported", e->napl, e->ncls);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(losses, e->loss.out, 8 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (head_grad)
        HIPCHK(e, hipMemcpyAsync(head_grad, e->loss.head_grad, (size_t)batch * npx * PP_HEAD_COLS * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

int pp_train_layout(pp_handle e, int32_t* n_entries, int64_t* n_param_floats, int64_t* n_state_floats) {
    if (!e) return PP_ERR_ARG;
    int st = train_state(e); if (st) return st;
    const TrainPlan& plan = e->train->plan;
    if (n_entries) *n_entries = (int32_t)plan.layout.size();
    if (n_param_floats) *n_param_floats = plan.n_params;
    if (n_state_floats) *n_state_floats = plan.n_state;
    return PP_OK;
}

int pp_train_layout_entry(pp_handle e, int32_t i, const char** name, int64_t* offset, int64_t* size, int32_t* is_state) {
    if (!e) return PP_ERR_ARG;
    int st = train_state(e); if (st) return st;
    if (i < 0 || i >= (int)e->train->plan.layout.size()) return fail(e, PP_ERR_ARG, "pp_train_layout_entry: index %d out of range", i);
    const TrainEntry& t = e->train->plan.layout[i];
    if (name) *name = t.name.c_str();
    if (offset) *offset = t.offset;
    if (size) *size = t.size;
    if (is_state) *is_state = t.is_state;
    return PP_OK;
}

int pp_train_step_async(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const int32_t* labels,
                        const float* reg_targets, int32_t batch, const pp_loss_config* lc) {
    if (!e) return PP_ERR_ARG;
    if (!labels || !reg_targets) return fail(e, PP_ERR_ARG, "pp_train_step: null argument");
    // labels and regression targets travel on the copy stream (behind the points, if their upload is still queued
    // there) while voxeliser and forward pass run: the loss kernel is the first reader, the second half of the step
    // waits for ev_tgt.  (The previous step has been synchronised before it returned: nobody still reads the buffers.)
    // Issued AFTER the first half has been launched: a pageable source makes hipMemcpyAsync block the host, and the
    // GPU should be busy with the forward pass by then.
    auto upload_targets = [&]() -> int {
        HIPCHK(e, hipMemcpyAsync(e->loss.labels, labels, (size_t)batch * e->A * sizeof(int32_t), hipMemcpyHostToDevice, e->copy_stream));
        HIPCHK(e, hipMemcpyAsync(e->loss.regt, reg_targets, (size_t)batch * e->A * 7 * sizeof(float), hipMemcpyHostToDevice, e->copy_stream));
        return copies_done(e, e->copy_stream);
    };
    return train_step_launch(e, params_dev, grads_dev, state_dev, batch, lc, upload_targets);
}

int pp_train_step_gt_async(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                           const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                           const pp_target_config* tc) {
    if (!e) return PP_ERR_ARG;
    int64_t total = 0;
    int st = check_gt(e, "pp_train_step_gt", gt_boxes, gt_classes, gt_counts, batch, tc, &total);
    if (st) return st;
    // the boxes follow the labels' route (copy stream, behind the first half); the anchor mask and the two assignment
    // passes are plain launches between the halves: the backward graph reads the fixed loss.labels / loss.regt
    auto assign = [&]() -> int {
        return targets_from_host(e, batch, gt_boxes, gt_classes, gt_counts, total, true, tc, false, e->copy_stream);
    };
    return train_step_launch(e, params_dev, grads_dev, state_dev, batch, lc, assign);
}

int pp_train_step_aug_async(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev,
                            const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch,
                            const pp_loss_config* lc, const pp_target_config* tc, const uint8_t* gt_valid,
                            const pp_augment_config* ac, const pp_aug_frame* frames, const double* box_draws) {
    if (!e) return PP_ERR_ARG;
    int64_t total = 0;
    int st = check_gt(e, "pp_train_step_aug", gt_boxes, gt_classes, gt_counts, batch, tc, &total);
    if (st == PP_OK) st = check_aug(e, "pp_train_step_aug", batch, total, ac, frames, box_draws);
    if (st) return st;
    // boxes and draws go up on the copy stream; the augmentation runs on the main stream ahead of the forward replay
    // (the augmented cloud replaces the resident one), the targets between the halves from the kept boxes
    auto augment = [&]() -> int {
        return augment_from_host(e, batch, gt_boxes, gt_classes, gt_valid, gt_counts, total, ac, frames, box_draws,
                                 e->copy_stream);
    };
    auto assign = [&]() -> int { return enqueue_targets(e, batch, e->tgt.gt, true, tc, false); };
    return train_step_launch(e, params_dev, grads_dev, state_dev, batch, lc, assign, augment);
}

int pp_train_step_aug(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                      const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                      const pp_target_config* tc, const uint8_t* gt_valid, const pp_augment_config* ac,
                      const pp_aug_frame* frames, const double* box_draws, float* losses) {
    return step_and_wait(e, "pp_train_step_aug", losses, [&] {
        return pp_train_step_aug_async(e, params_dev, grads_dev, state_dev, gt_boxes, gt_classes, gt_counts, batch, lc, tc,
                                       gt_valid, ac, frames, box_draws);
    });
}

int pp_train_step_sample_async(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev,
                               const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch,
                               const pp_loss_config* lc, const pp_target_config* tc, const uint8_t* gt_valid,
                               const pp_gt_sample_config* sc, const pp_gts_cand* cands, const int32_t* cand_counts,
                               const pp_augment_config* ac, const pp_aug_frame* frames, const double* box_draws) {
    if (!e) return PP_ERR_ARG;
    int64_t total = 0;
    int max_out_n = 0;
    std::vector<int> bound_off;
    int st = check_gt(e, "pp_train_step_sample", gt_boxes, gt_classes, gt_counts, batch, tc, &total);
    if (st == PP_OK)
        st = check_gts(e, "pp_train_step_sample", gt_counts, batch, sc, cands, cand_counts, &max_out_n, &bound_off);
    if (st) return st;
    const size_t bound_total = (size_t)bound_off[(size_t)batch];
    // the augmentation's draws: frame b has gt_counts[b] + (its largest round) rows, of which the first
    // gt_counts[b] + accepted are used
    int64_t rows = 0;
    if (ac) {
        if (ac->global_rot_per_object)
            return fail(e, PP_ERR_UNSUPPORTED, "pp_train_step_sample: global_random_rotation_range_per_object draws depend on "
                        "the box, which is chosen on the device");
        e->aug.h_draw_off.assign((size_t)batch, 0);
        for (int b = 0; b < batch; ++b) {
            int most = 0;
            for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) most = std::max(most, cand_counts[(size_t)b * PP_GTS_MAX_ROUNDS + r]);
            e->aug.h_draw_off[(size_t)b] = (int)rows;
            rows += gt_counts[b] + most;
        }
        if ((st = check_aug(e, "pp_train_step_sample", batch, rows, ac, frames, box_draws))) return st;
    }
    auto sample = [&]() -> int {
        int r = enqueue_gt_sample(e, batch, gt_boxes, gt_classes, gt_valid, gt_counts, total, sc, cands, cand_counts, max_out_n,
                                  e->copy_stream);
        if (r) return r;
        // No read-back here: the grown frames become the resident ones by the host-known bound (the tail past a
        // frame's device-side count is never read), and everything enqueued from here on is sized from it.
        if (bound_total)
            HIPCHK(e, hipMemcpyAsync(e->d_points, e->spare_pts, bound_total * e->F * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(e, hipMemcpyAsync(e->d_offsets, e->gts.offsets, (size_t)(batch + 1) * sizeof(int), hipMemcpyDeviceToDevice, e->stream));
        set_resident(e, batch, bound_off.data(), max_out_n, false);
        if (ac)      // on the sampler's output, which stays live beside tgt.gt, the augmentation's
            return enqueue_augment(e, batch, e->gts.out, rows, ac, frames, box_draws, e->copy_stream, &e->aug.h_draw_off);
        return PP_OK;
    };
    // (without augmentation the target kernels read the sampler's boxes where they are)
    auto assign = [&]() -> int { return enqueue_targets(e, batch, ac ? e->tgt.gt : e->gts.out, true, tc, false); };
    return train_step_launch(e, params_dev, grads_dev, state_dev, batch, lc, assign, sample);
}

int pp_train_step_sample(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                         const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                         const pp_target_config* tc, const uint8_t* gt_valid, const pp_gt_sample_config* sc,
                         const pp_gts_cand* cands, const int32_t* cand_counts, const pp_augment_config* ac,
                         const pp_aug_frame* frames, const double* box_draws, float* losses) {
    return step_and_wait(e, "pp_train_step_sample", losses, [&] {
        return pp_train_step_sample_async(e, params_dev, grads_dev, state_dev, gt_boxes, gt_classes, gt_counts, batch, lc, tc,
                                          gt_valid, sc, cands, cand_counts, ac, frames, box_draws);
    });
}

int pp_train_step_gt(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const float* gt_boxes,
                     const int32_t* gt_classes, const int32_t* gt_counts, int32_t batch, const pp_loss_config* lc,
                     const pp_target_config* tc, float* losses) {
    return step_and_wait(e, "pp_train_step_gt", losses, [&] {
        return pp_train_step_gt_async(e, params_dev, grads_dev, state_dev, gt_boxes, gt_classes, gt_counts, batch, lc, tc);
    });
}

int pp_train_step_wait(pp_handle e, float* losses) {
    if (!e) return PP_ERR_ARG;
    if (!losses) return fail(e, PP_ERR_ARG, "pp_train_step_wait: losses is NULL");
    if (!e->train_pending) return fail(e, PP_ERR_STATE, "pp_train_step_wait: no step in flight");
    (void)hipSetDevice(e->device);
    e->train_pending = false;
    HIPCHK(e, hipStreamSynchronize(e->stream));
    memcpy(losses, e->h_train_losses, 8 * sizeof(float));
    return PP_OK;
}

int pp_train_step(pp_handle e, const float* params_dev, float* grads_dev, float* state_dev, const int32_t* labels,
                  const float* reg_targets, int32_t batch, const pp_loss_config* lc, float* losses) {
    return step_and_wait(e, "pp_train_step", losses, [&] {
        return pp_train_step_async(e, params_dev, grads_dev, state_dev, labels, reg_targets, batch, lc);
    });
}

int pp_train_fetch_decisions(pp_handle e, int32_t layer, uint8_t* relu_mask, int64_t capacity, int64_t* count) {
    if (!e) return PP_ERR_ARG;
    if (!count) return fail(e, PP_ERR_ARG, "pp_train_fetch_decisions: count is NULL");
    if (!e->train || !e->train->buffers || e->train->last_batch < 1)
        return fail(e, PP_ERR_STATE, "pp_train_fetch_decisions: no training step to tap");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_train_fetch_decisions: the step has not been waited for");
    (void)hipSetDevice(e->device);
    pp_engine::TrainState* t = e->train;
    const size_t B = (size_t)t->last_batch;
    if (layer < 0) {      // the PFN: winning row per (pillar slot, channel), int32 stored as 4 bytes each
        const int64_t n = (int64_t)B * t->shape.max_voxels * t->shape.C;
        *count = n;
        if (!relu_mask) return PP_OK;
        if (capacity < n * 4) return fail(e, PP_ERR_ARG, "pp_train_fetch_decisions: %lld bytes needed", (long long)(n * 4));
        HIPCHK(e, hipStreamSynchronize(e->stream));
        HIPCHK(e, hipMemcpy(relu_mask, t->cx.pfn_arg, (size_t)n * 4, hipMemcpyDeviceToHost));
        return PP_OK;
    }
    if (layer >= (int)t->plan.layers.size())
        return fail(e, PP_ERR_ARG, "pp_train_fetch_decisions: layer %d out of range", layer);
    const LayerDesc& l = t->shape.layers[t->plan.layers[layer].layer];
    const int64_t n = (l.kind == LAYER_SEP) ? (int64_t)B * l.out_h * l.out_w * l.cout
                                            : (int64_t)B * l.in_h * l.in_w * l.k * l.k * l.cout;
    *count = n;
    if (!relu_mask) return PP_OK;
    if (capacity < n) return fail(e, PP_ERR_ARG, "pp_train_fetch_decisions: %lld bytes needed", (long long)n);
    unsigned char* d = nullptr;
    HIPCHK(e, hipMalloc(&d, (size_t)n));
    launch_relu_mask(t->cx.lbuf[layer].Z, t->cx.lbuf[layer].coef, (long)n, l.cout, d, e->stream);
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(relu_mask, d, (size_t)n, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (he != hipSuccess) return fail(e, PP_ERR_HIP, "pp_train_fetch_decisions: %s", hipGetErrorString(he));
    return PP_OK;
}

int pp_train_set_frozen(pp_handle e, const char* const* units, int32_t n) {
    if (!e) return PP_ERR_ARG;
    if (n < 0 || (n > 0 && !units)) return fail(e, PP_ERR_ARG, "pp_train_set_frozen: bad argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_train_set_frozen: a training step is in flight");
    int st = train_state(e); if (st) return st;
    std::vector<std::string> names;
    for (int32_t i = 0; i < n; ++i) {
        if (!units[i]) return fail(e, PP_ERR_ARG, "pp_train_set_frozen: unit %d is NULL", i);
        names.push_back(units[i]);
    }
    if (train_plan_freeze(e->train->plan, names) != PP_OK)
        return fail(e, PP_ERR_ARG, "pp_train_set_frozen: unknown or repeated unit name, or every unit frozen");
    return PP_OK;
}

int pp_train_graph_stats(pp_handle e, int32_t* captures, int32_t* replays) {
    if (!e) return PP_ERR_ARG;
    if (captures) *captures = e->train ? e->train->n_captures : 0;
    if (replays) *replays = e->train ? e->train->n_replays : 0;
    return PP_OK;
}

int pp_adamw_step_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                         int64_t n, float lr_t, float beta1, float beta2, float epsilon, float weight_decay) {
    if (n < 0 || (n > 0 && (!params || !grads || !m || !v))) return fail(nullptr, PP_ERR_ARG, "pp_adamw_step_device: bad argument");
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, PP_ERR_HIP, "pp_adamw_step_device: hipSetDevice(%d) failed", device);
    launch_adamw(params, grads, m, v, n, lr_t, beta1, beta2, epsilon, weight_decay, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(nullptr, PP_ERR_HIP, "pp_adamw_step_device: launch failed");
    return PP_OK;
}

int pp_adamw_step_segments_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                                  const int64_t* segments, int32_t n_segments, float lr_t, float beta1, float beta2,
                                  float epsilon, float weight_decay) {
    if (n_segments < 0 || (n_segments > 0 && (!params || !grads || !m || !v || !segments)))
        return fail(nullptr, PP_ERR_ARG, "pp_adamw_step_segments_device: bad argument");
    for (int32_t i = 0; i < n_segments; ++i)
        if (segments[2 * i] < 0 || segments[2 * i + 1] < 0)
            return fail(nullptr, PP_ERR_ARG, "pp_adamw_step_segments_device: segment %d is negative", i);
    if (hipSetDevice(device) != hipSuccess)
        return fail(nullptr, PP_ERR_HIP, "pp_adamw_step_segments_device: hipSetDevice(%d) failed", device);
    launch_adamw_segments(params, grads, m, v, segments, n_segments, lr_t, beta1, beta2, epsilon, weight_decay,
                          (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(nullptr, PP_ERR_HIP, "pp_adamw_step_segments_device: launch failed");
    return PP_OK;
}

int pp_grad_clip_workspace_bytes(int64_t n_floats, int32_t n_segments, int32_t n_groups, int64_t* bytes) {
    if (n_floats < 0 || n_segments < 0 || n_groups < 1 || !bytes)
        return fail(nullptr, PP_ERR_ARG, "pp_grad_clip_workspace_bytes: bad argument");
    *bytes = grad_clip_layout(n_floats, n_segments, n_groups).bytes;
    return PP_OK;
}

int pp_grad_norm_device(int device, void* stream, const float* grads, int64_t n, const int64_t* segments,
                        int32_t n_segments, const int32_t* groups, int32_t n_groups, void* workspace) {
    const char* who = "pp_grad_norm_device";
    if (n > 0 && !grads) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    int st = check_clip_table(who, n, segments, n_segments, groups, n_groups, workspace, true);
    if (st) return st;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, PP_ERR_HIP, "%s: hipSetDevice(%d) failed", who, device);
    launch_grad_norm(grads, segments, n_segments, groups, n_groups, PP_CLIP_NONE, 0.f, 0, workspace, n, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(nullptr, PP_ERR_HIP, "%s: launch failed", who);
    return PP_OK;
}

int pp_adamw_step_clipped_device(int device, void* stream, float* params, const float* grads, float* m, float* v,
                                 int64_t n, const int64_t* segments, int32_t n_segments, const int32_t* groups,
                                 int32_t n_groups, const pp_grad_clip_config* cfg, void* workspace, float lr_t,
                                 float beta1, float beta2, float epsilon, float weight_decay) {
    const char* who = "pp_adamw_step_clipped_device";
    if (!cfg || (n > 0 && (!params || !grads || !m || !v))) return fail(nullptr, PP_ERR_ARG, "%s: bad argument", who);
    if (cfg->mode < PP_CLIP_NONE || cfg->mode > PP_CLIP_GLOBAL_NORM) return fail(nullptr, PP_ERR_ARG, "%s: unknown mode %d", who, cfg->mode);
    if (cfg->mode != PP_CLIP_NONE && !(cfg->clip > 0.f && std::isfinite(cfg->clip)))
        return fail(nullptr, PP_ERR_ARG, "%s: clip must be positive and finite", who);
    const int skip = cfg->skip_nonfinite ? 1 : 0;
    const bool reduce = cfg->mode != PP_CLIP_VALUE || skip;          // (monitor mode takes the norms, too)
    int st = check_clip_table(who, n, segments, n_segments, groups, n_groups, workspace, reduce);
    if (st) return st;
    if (hipSetDevice(device) != hipSuccess) return fail(nullptr, PP_ERR_HIP, "%s: hipSetDevice(%d) failed", who, device);
    if (reduce)
        launch_grad_norm(grads, segments, n_segments, groups, n_groups, cfg->mode, cfg->clip, skip, workspace, n, (hipStream_t)stream);
    launch_adamw_segments_clipped(params, grads, m, v, segments, n_segments, groups, n_groups, cfg->mode, cfg->clip, skip,
                                  reduce ? workspace : nullptr, lr_t, beta1, beta2, epsilon, weight_decay, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return fail(nullptr, PP_ERR_HIP, "%s: launch failed", who);
    return PP_OK;
}

}  // extern "C"
