// C-ABI, preparing training data on the device: target assignment (kernels: targets.hip), augmentation (augment.hip), GT
// sampling (gt_sample.hip), the object-database build (gt_database.hip).  The fused training steps (api_train.hip) queue enqueue_*.
#include "pp_engine.h"

// `n` boxes [7] x y z w l h r: finite, sizes > 0
template <typename T>
static int check_boxes(pp_engine* e, const char* who, const T* boxes, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const T* q = boxes + i * 7;
        for (int k = 0; k < 7; ++k)
            if (!std::isfinite(q[k])) return fail(e, PP_ERR_ARG, "%s: box %lld is not finite", who, (long long)i);
        if (!(q[3] > 0 && q[4] > 0 && q[5] > 0))
            return fail(e, PP_ERR_ARG, "%s: box %lld has a size <= 0 (w l h = %g %g %g)", who, (long long)i, (double)q[3],
                        (double)q[4], (double)q[5]);
    }
    return PP_OK;
}

// per-frame box counts; *total = boxes over all frames
static int check_counts(pp_engine* e, const char* who, const int32_t* counts, int batch, int64_t* total) {
    *total = 0;
    for (int b = 0; b < batch; ++b) {
        if (counts[b] < 0 || counts[b] > PP_MAX_GT_PER_FRAME)
            return fail(e, PP_ERR_ARG, "%s: frame %d has %d boxes (0..%d)", who, b, counts[b], PP_MAX_GT_PER_FRAME);
        *total += counts[b];
    }
    return PP_OK;
}

// ---- training targets from ground-truth boxes (targets.hip) ----

// The boxes of `batch` frames as pp_assign_targets / pp_train_step_gt* take them; *total = boxes over all frames.
int check_gt(pp_engine* e, const char* who, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
             int batch, const pp_target_config* tc, int64_t* total) {
    if (!gt_counts || !tc) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    if (batch < 1 || batch > e->B) return fail(e, PP_ERR_ARG, "%s: batch %d outside [1, max_batch=%d]", who, batch, e->B);
    if (!std::isfinite(tc->matched_threshold) || !std::isfinite(tc->unmatched_threshold))
        return fail(e, PP_ERR_ARG, "%s: thresholds must be finite", who);
    int st = check_counts(e, who, gt_counts, batch, total); if (st) return st;
    const int64_t n = *total;
    if (n > 0 && !gt_boxes) return fail(e, PP_ERR_ARG, "%s: gt_boxes is NULL", who);
    if ((st = check_boxes(e, who, gt_boxes, n))) return st;
    for (int64_t i = 0; gt_classes && i < n; ++i)
        if (gt_classes[i] < 1 || gt_classes[i] > e->cfg.num_class)
            return fail(e, PP_ERR_ARG, "%s: box %lld has class %d (1..%d)", who, (long long)i, gt_classes[i], e->cfg.num_class);
    return PP_OK;
}

static void alloc_gt(DevAlloc& A, GtSet* g) {
    const size_t gmax = (size_t)A.e->B * PP_MAX_GT_PER_FRAME;
    A(&g->boxes, gmax * 7); A(&g->cls, gmax); A(&g->valid, gmax); A(&g->cnt, (size_t)A.e->B);
}

// Fills `buf` from the host arrays on `s` (`total` boxes in `batch` frames).  *view: the set as a kernel reads it,
// cls / valid NULL where the caller gave none.
static int upload_gt(pp_engine* e, const GtSet& buf, const float* boxes, const int32_t* classes, const uint8_t* valid,
                     const int32_t* counts, int64_t total, int batch, hipStream_t s, GtSet* view) {
    *view = buf;
    if (!classes) view->cls = nullptr;
    if (!valid) view->valid = nullptr;
    if (total > 0) {
        HIPCHK(e, hipMemcpyAsync(buf.boxes, boxes, (size_t)total * 7 * sizeof(float), hipMemcpyHostToDevice, s));
        if (classes) HIPCHK(e, hipMemcpyAsync(buf.cls, classes, (size_t)total * sizeof(int32_t), hipMemcpyHostToDevice, s));
        if (valid) HIPCHK(e, hipMemcpyAsync(buf.valid, valid, (size_t)total, hipMemcpyHostToDevice, s));
    }
    HIPCHK(e, hipMemcpyAsync(buf.cnt, counts, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, s));
    return PP_OK;
}

// Queues the assignment for `batch` frames on the handle's stream from the boxes in `gt` (already on the device, or
// queued ahead on this stream): the anchor mask of the resident frames is built from the current cell map when
// `resident_mask` (else tgt.mask holds the caller's), the per-box maxima are reset, then the two passes write
// loss.labels / loss.regt (and the optional per-anchor outputs).
int enqueue_targets(pp_engine* e, int batch, const GtSet& gt, bool resident_mask, const pp_target_config* tc, bool extra) {
    ProfScope ps(e, nullptr);      // each launch under its own name
    const uint8_t* mask = e->tgt.mask;
    if (resident_mask) {
        // the integral-image kernels on this pass's cell map (the bitmap variant would trust occbits_live, which
        // describes the last inference PFN launch); anchor_area_threshold < 0 keeps every anchor (area >= 0)
        if (e->cfg.anchor_area_threshold >= 0.f)
            launch_anchor_mask(e->d_cellmap, batch, e->nz, e->ny, e->nx, e->d_cells, e->A, e->cfg.anchor_area_threshold,
                               e->d_integ, e->tgt.mask, e->stream);
        else
            mask = nullptr;
    }
    {
        ProfScope pm(e, "memset:tgt_top", true);
        HIPCHK(e, hipMemsetAsync(e->tgt.top, 0, (size_t)batch * PP_MAX_GT_PER_FRAME * sizeof(unsigned), e->stream));
    }
    TargetParams p;
    p.batch = batch; p.A = e->A; p.anchor_near = e->d_anchor_near; p.anchors = e->d_anchors; p.mask = mask;
    p.gt = gt.boxes; p.gt_cls = gt.cls; p.gt_cnt = gt.cnt;
    p.top = e->tgt.top;
    p.matched = tc->matched_threshold; p.unmatched = tc->unmatched_threshold;
    p.labels = e->loss.labels; p.reg_targets = e->loss.regt;
    p.gt_index = extra ? e->tgt.index : nullptr; p.overlap = extra ? e->tgt.overlap : nullptr;
    launch_targets(p, e->stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// ... from host boxes: they go up into tgt.gt on `up` (the copy stream: the main stream then waits; or the main stream)
int targets_from_host(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                      int64_t total, bool resident_mask, const pp_target_config* tc, bool extra, hipStream_t up) {
    GtSet gt;
    int st = upload_gt(e, e->tgt.gt, gt_boxes, gt_classes, nullptr, gt_counts, total, batch, up, &gt);
    if (st == PP_OK) st = copies_done(e, up);
    return st ? st : enqueue_targets(e, batch, gt, resident_mask, tc, extra);
}

// The augmentation's argument checks beyond check_gt's: the config, the draws, and the resident batch.
int check_aug(pp_engine* e, const char* who, int batch, int64_t total, const pp_augment_config* ac,
              const pp_aug_frame* frames, const double* box_draws) {
    if (!ac || !frames) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    if (ac->num_try < 1 || ac->num_try > PP_AUG_MAX_TRY)
        return fail(e, PP_ERR_ARG, "%s: num_try %d outside 1..%d", who, ac->num_try, PP_AUG_MAX_TRY);
    if (e->cur_batch != batch)
        return fail(e, PP_ERR_ARG, "%s: %d frames are resident, batch is %d", who, e->cur_batch, batch);
    for (int b = 0; b < batch; ++b) {
        const pp_aug_frame& f = frames[b];
        if (!std::isfinite(f.theta) || !std::isfinite(f.scale) || !std::isfinite(f.t[0]) || !std::isfinite(f.t[1]) ||
            !std::isfinite(f.t[2]))
            return fail(e, PP_ERR_ARG, "%s: frame %d has a non-finite draw", who, b);
        if (!(f.scale > 0.0)) return fail(e, PP_ERR_ARG, "%s: frame %d has scale %g <= 0", who, b, f.scale);
    }
    const int64_t nd = total * ac->num_try * 5;
    if (nd > 0 && !box_draws) return fail(e, PP_ERR_ARG, "%s: box_draws is NULL", who);
    // one branch-free pass over the bits (an exponent of all ones: inf or NaN); the failing box is looked up after
    uint64_t bad = 0;
    const uint64_t* bits = (const uint64_t*)box_draws;
    for (int64_t i = 0; i < nd; ++i) bad |= (uint64_t)((bits[i] & 0x7ff0000000000000ull) == 0x7ff0000000000000ull);
    if (bad)
        for (int64_t i = 0; i < nd; ++i)
            if (!std::isfinite(box_draws[i]))
                return fail(e, PP_ERR_ARG, "%s: box draw %lld is not finite", who, (long long)(i / ((int64_t)ac->num_try * 5)));
    return PP_OK;
}

static int ensure_aug(pp_engine* e) {
    pp_engine::Aug& a = e->aug;
    if (a.ready) return PP_OK;
    const size_t gmax = (size_t)e->B * PP_MAX_GT_PER_FRAME;
    DevAlloc A{e, ensure_spare_pts(e)};
    alloc_gt(A, &a.in);
    A(&a.draws, gmax * PP_AUG_MAX_TRY * 5); A(&a.frames, (size_t)e->B); A(&a.rec, gmax); A(&a.box_tmp, gmax * 7);
    A(&a.keep, gmax); A(&a.sel, gmax); A(&a.cs, (size_t)e->B * 2); A(&a.draw_off, (size_t)e->B);
    a.ready = A.st == PP_OK;
    return A.st;
}

// Queues the augmentation of the resident frames on the handle's stream, from the boxes in `in` (on the device, or
// queued ahead on `up`); the draws go up on `up` (the copy stream: the main stream then waits; or the main stream).
// The result lands in the resident input buffer (a zero-copy feed is replaced by device copies); tgt.gt receives the
// kept boxes, their classes (1 where `in` has none) and counts.  draw_off: frame b's boxes take the draw rows from
// (*draw_off)[b] on and `total` counts the rows (the sampled step); else box i takes row i and `total` counts the boxes.
int enqueue_augment(pp_engine* e, int batch, const GtSet& in, int64_t total, const pp_augment_config* ac,
                    const pp_aug_frame* frames, const double* box_draws, hipStream_t up, const std::vector<int>* draw_off) {
    int st;
    pp_engine::Aug& a = e->aug;
    if ((st = ensure_aug(e))) return st;
    if (total > 0)
        HIPCHK(e, hipMemcpyAsync(a.draws, box_draws, (size_t)total * ac->num_try * 5 * sizeof(double), hipMemcpyHostToDevice, up));
    if (draw_off)
        HIPCHK(e, hipMemcpyAsync(a.draw_off, draw_off->data(), (size_t)batch * sizeof(int), hipMemcpyHostToDevice, up));
    HIPCHK(e, hipMemcpyAsync(a.frames, frames, (size_t)batch * sizeof(pp_aug_frame), hipMemcpyHostToDevice, up));
    if ((st = copies_done(e, up))) return st;
    const float* src = nullptr;
    if ((st = resident_points(e, batch, e->stream, true, &src))) return st;
    ProfScope ps(e, nullptr);      // each launch under its own name
    AugParams p;
    p.batch = batch; p.F = e->F; p.T = ac->num_try; p.v2 = ac->global_rot_per_object ? 1 : 0;
    p.pc[0] = e->cfg.pc_range[0]; p.pc[1] = e->cfg.pc_range[1]; p.pc[2] = e->cfg.pc_range[3]; p.pc[3] = e->cfg.pc_range[4];
    p.offsets = e->d_offsets; p.pts_in = src; p.pts_out = e->spare_pts;
    p.gt_in = in.boxes; p.cls_in = in.cls; p.valid = in.valid; p.cnt_in = in.cnt;
    p.draws = a.draws; p.draw_off = draw_off ? a.draw_off : nullptr; p.frames = a.frames; p.frame_cs = a.cs;
    p.boxrec = a.rec; p.box_tmp = a.box_tmp; p.keep = a.keep; p.sel = a.sel;
    p.gt_out = e->tgt.gt.boxes; p.cls_out = e->tgt.gt.cls; p.cnt_out = e->tgt.gt.cnt;
    launch_augment(p, e->cur_max_n, e->stream);
    HIPCHK(e, hipGetLastError());
    a.total = total;
    const size_t n = (size_t)e->cur_total;      // (also a zero-copy feed's last offset: feed_zero_copy sets both)
    if (n) HIPCHK(e, hipMemcpyAsync(e->d_points, e->spare_pts, n * e->F * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return PP_OK;
}

// ... from host boxes: they go up into aug.in on `up`, ahead of the draws
int augment_from_host(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                      const int32_t* gt_counts, int64_t total, const pp_augment_config* ac, const pp_aug_frame* frames,
                      const double* box_draws, hipStream_t up) {
    GtSet in;
    int st = ensure_aug(e);
    if (st == PP_OK) st = upload_gt(e, e->aug.in, gt_boxes, gt_classes, gt_valid, gt_counts, total, batch, up, &in);
    return st ? st : enqueue_augment(e, batch, in, total, ac, frames, box_draws, up);
}

// The sampling's argument checks beyond check_gt's, and the host-known bounds on what it writes: the pasted cloud's
// size is known on the device only, so every launch and copy behind it is sized from n_b + (points of all candidates
// of one round), which is refused here when it does not fit.  *max_out_n: the largest frame's bound; *bound_off
// [batch + 1]: prefix sums of the frames' bounds.
int check_gts(pp_engine* e, const char* who, const int32_t* gt_counts, int batch, const pp_gt_sample_config* sc,
              const pp_gts_cand* cands, const int32_t* cand_counts, int* max_out_n_p, std::vector<int>* bound_off) {
    if (!sc || !cands || !cand_counts) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    if (e->db.n < 0) return fail(e, PP_ERR_STATE, "%s: no database loaded (pp_gtdb_load)", who);
    if (e->cur_batch != batch)
        return fail(e, PP_ERR_ARG, "%s: %d frames are resident, batch is %d", who, e->cur_batch, batch);
    if (int st = require_host_exact(e, who)) return st;
    int max_out_n = 0;
    bound_off->assign((size_t)batch + 1, 0);
    for (int b = 0; b < batch; ++b) {
        const int32_t* cc = cand_counts + (size_t)b * PP_GTS_MAX_ROUNDS;
        const pp_gts_cand* c = cands + (size_t)b * PP_GTS_MAX_CAND;
        const int n_b = e->h_cur_off[b + 1] - e->h_cur_off[b];
        int s0 = 0;
        int64_t worst = 0;
        for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) {
            if (cc[r] < 0 || s0 + (int64_t)cc[r] > PP_GTS_MAX_CAND)
                return fail(e, PP_ERR_ARG, "%s: frame %d has more than %d candidates", who, b, PP_GTS_MAX_CAND);
            if (gt_counts[b] + cc[r] > PP_MAX_GT_PER_FRAME)
                return fail(e, PP_ERR_ARG, "%s: frame %d: %d boxes + %d candidates > %d", who, b, gt_counts[b], cc[r],
                            PP_MAX_GT_PER_FRAME);
            int64_t pts = 0;
            for (int s = s0; s < s0 + cc[r]; ++s) {
                if (c[s].object < 0 || c[s].object >= e->db.n)
                    return fail(e, PP_ERR_ARG, "%s: frame %d slot %d: object %d outside the database (%lld objects)", who,
                                b, s, c[s].object, (long long)e->db.n);
                if (s > s0 && c[s].group < c[s - 1].group)
                    return fail(e, PP_ERR_ARG, "%s: frame %d slot %d: groups out of order", who, b, s);
                pts += e->db.h_npts[(size_t)c[s].object];
            }
            worst = std::max(worst, pts);
            s0 += cc[r];
        }
        if (n_b + worst > e->NMAX)
            return fail(e, PP_ERR_ARG, "%s: frame %d: %d points + up to %lld pasted > max_points_per_frame=%d", who, b, n_b,
                        (long long)worst, e->NMAX);
        max_out_n = std::max(max_out_n, (int)(n_b + worst));
        (*bound_off)[(size_t)b + 1] = (*bound_off)[(size_t)b] + (int)(n_b + worst);
    }
    *max_out_n_p = max_out_n;
    return PP_OK;
}

static int ensure_gts(pp_engine* e) {
    pp_engine::Gts& g = e->gts;
    if (g.ready) return PP_OK;
    const size_t B = (size_t)e->B, cmax = B * PP_GTS_MAX_CAND;
    DevAlloc A{e, ensure_spare_pts(e)};
    alloc_gt(A, &g.in); alloc_gt(A, &g.out);
    A(&g.cands, cmax); A(&g.cand_counts, B * PP_GTS_MAX_ROUNDS); A(&g.planes, cmax); A(&g.status, cmax);
    A(&g.counts, cmax); A(&g.round, B); A(&g.acc_n, B); A(&g.acc_slot, cmax);
    A(&g.acc_pstart, B * (PP_GTS_MAX_CAND + 1)); A(&g.box_off, 2 * (B + 1)); A(&g.offsets, B + 1);
    g.ready = A.st == PP_OK;
    return A.st;
}

// Queues the sampling of the resident frames on the handle's stream; the inputs go up on `up` (the copy stream: the
// main stream then waits; or the main stream).  The grown cloud lands in the spare point buffer and the new offsets in
// gts.offsets; the caller moves both into the resident buffers (by the counts read back, or by the bound): set_resident.
int enqueue_gt_sample(pp_engine* e, int batch, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                      const int32_t* gt_counts, int64_t total, const pp_gt_sample_config* sc, const pp_gts_cand* cands,
                      const int32_t* cand_counts, int max_out_n, hipStream_t up) {
    int st;
    pp_engine::Gts& g = e->gts;
    if ((st = ensure_gts(e))) return st;
    GtSet in;
    if ((st = upload_gt(e, g.in, gt_boxes, gt_classes, gt_valid, gt_counts, total, batch, up, &in))) return st;
    HIPCHK(e, hipMemcpyAsync(g.cands, cands, (size_t)batch * PP_GTS_MAX_CAND * sizeof(pp_gts_cand), hipMemcpyHostToDevice, up));
    HIPCHK(e, hipMemcpyAsync(g.cand_counts, cand_counts, (size_t)batch * PP_GTS_MAX_ROUNDS * sizeof(int32_t), hipMemcpyHostToDevice, up));
    if ((st = copies_done(e, up))) return st;
    // a zero-copy feed is read from the caller's page-locked memory and replaced by device copies (as the augmentation does)
    const float* src = nullptr;
    if ((st = resident_points(e, batch, e->stream, true, &src))) return st;
    GtsParams p;
    p.batch = batch; p.F = e->F; p.max_pc = sc->max_point_collision; p.min_pc = sc->min_point_collision;
    p.offsets = e->d_offsets; p.pts_in = src; p.pts_out = e->spare_pts; p.offsets_out = g.offsets;
    p.gt_in = in.boxes; p.cls_in = in.cls; p.valid_in = in.valid; p.cnt_in = in.cnt;
    p.cands = g.cands; p.cand_counts = g.cand_counts;
    p.db_pts = e->db.pts; p.db_off = e->db.off; p.db_box = e->db.box; p.db_cls = e->db.cls;
    p.planes = g.planes; p.status = g.status; p.counts = g.counts; p.round_used = g.round;
    p.acc_n = g.acc_n; p.acc_slot = g.acc_slot; p.acc_pstart = g.acc_pstart; p.box_off = g.box_off;
    p.gt_out = g.out.boxes; p.cls_out = g.out.cls; p.valid_out = g.out.valid; p.cnt_out = g.out.cnt;
    {
        ProfScope ps(e, nullptr);      // each launch under its own name
        launch_gt_sample(p, e->cur_max_n, max_out_n, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    g.batch = batch;
    return PP_OK;
}

extern "C" {

int pp_augment(pp_handle e, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
               const int32_t* gt_counts, int32_t batch, const pp_augment_config* ac, const pp_aug_frame* frames,
               const double* box_draws, float* points_out, float* boxes_out, int32_t* classes_out, int32_t* counts_out) {
    if (!e) return PP_ERR_ARG;
    if (!points_out || !boxes_out || !classes_out || !counts_out) return fail(e, PP_ERR_ARG, "pp_augment: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_augment: a training step is in flight");
    if (int st = require_host_exact(e, "pp_augment")) return st;
    const pp_target_config tc = {0.5f, 0.35f, {0, 0}};
    int64_t total = 0;
    int st = check_gt(e, "pp_augment", gt_boxes, gt_classes, gt_counts, batch, &tc, &total);
    if (st == PP_OK) st = check_aug(e, "pp_augment", batch, total, ac, frames, box_draws);
    if (st) return st;
    (void)hipSetDevice(e->device);
    prof_reset(e);
    if ((st = augment_from_host(e, batch, gt_boxes, gt_classes, gt_valid, gt_counts, total, ac, frames, box_draws, e->stream)))
        return st;
    HIPCHK(e, hipMemcpyAsync(counts_out, e->tgt.gt.cnt, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    int64_t kept = 0;
    for (int b = 0; b < batch; ++b) kept += counts_out[b];
    if (e->cur_total)
        HIPCHK(e, hipMemcpyAsync(points_out, e->d_points, (size_t)e->cur_total * e->F * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (kept) {
        HIPCHK(e, hipMemcpyAsync(boxes_out, e->tgt.gt.boxes, (size_t)kept * 7 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipMemcpyAsync(classes_out, e->tgt.gt.cls, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

// ---- GT-database sampling (gt_sample.hip) ----

int pp_gtdb_load(pp_handle e, const float* points, const int64_t* point_offsets, const double* boxes,
                 const int32_t* classes, int64_t n) {
    if (!e) return PP_ERR_ARG;
    if (n < 0 || !point_offsets || (n > 0 && (!boxes || !classes)))
        return fail(e, PP_ERR_ARG, "pp_gtdb_load: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_gtdb_load: a training step is in flight");
    if (point_offsets[0] != 0) return fail(e, PP_ERR_ARG, "pp_gtdb_load: point_offsets[0] must be 0");
    if (n > 0x7fffffff / 8) return fail(e, PP_ERR_ARG, "pp_gtdb_load: too many objects");
    for (int64_t i = 0; i < n; ++i) {
        if (point_offsets[i + 1] < point_offsets[i])
            return fail(e, PP_ERR_ARG, "pp_gtdb_load: point_offsets not monotone at object %lld", (long long)i);
        if (classes[i] < 1 || classes[i] > e->cfg.num_class)
            return fail(e, PP_ERR_ARG, "pp_gtdb_load: object %lld has class %d (1..%d)", (long long)i, classes[i], e->cfg.num_class);
    }
    if (int st = check_boxes(e, "pp_gtdb_load", boxes, n)) return st;
    const int64_t total = point_offsets[n];
    if (total > 0x7fffffff / (e->F > 0 ? e->F : 1)) return fail(e, PP_ERR_ARG, "pp_gtdb_load: too many points");
    if (total > 0 && !points) return fail(e, PP_ERR_ARG, "pp_gtdb_load: points is NULL");
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    for (void* p : {(void*)e->db.pts, (void*)e->db.off, (void*)e->db.box, (void*)e->db.cls}) if (p) (void)hipFree(p);
    e->db.pts = nullptr; e->db.off = nullptr; e->db.box = nullptr; e->db.cls = nullptr;
    e->db.n = -1;
    std::vector<int> off32((size_t)n + 1);
    e->db.h_npts.resize((size_t)n);
    for (int64_t i = 0; i <= n; ++i) off32[(size_t)i] = (int)point_offsets[i];
    for (int64_t i = 0; i < n; ++i) e->db.h_npts[(size_t)i] = (int)(point_offsets[i + 1] - point_offsets[i]);
    HIPCHK(e, hipMalloc((void**)&e->db.pts, std::max<size_t>((size_t)total * e->F, 1) * sizeof(float)));
    HIPCHK(e, hipMalloc((void**)&e->db.off, ((size_t)n + 1) * sizeof(int)));
    HIPCHK(e, hipMalloc((void**)&e->db.box, std::max<size_t>((size_t)n * 7, 1) * sizeof(double)));
    HIPCHK(e, hipMalloc((void**)&e->db.cls, std::max<size_t>((size_t)n, 1) * sizeof(int)));
    if (total) HIPCHK(e, hipMemcpy(e->db.pts, points, (size_t)total * e->F * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(e->db.off, off32.data(), off32.size() * sizeof(int), hipMemcpyHostToDevice));
    if (n) HIPCHK(e, hipMemcpy(e->db.box, boxes, (size_t)n * 7 * sizeof(double), hipMemcpyHostToDevice));
    if (n) HIPCHK(e, hipMemcpy(e->db.cls, classes, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    e->db.n = n;
    return PP_OK;
}

int pp_gt_sample(pp_handle e, const float* gt_boxes, const int32_t* gt_classes, const uint8_t* gt_valid,
                 const int32_t* gt_counts, int32_t batch, const pp_gt_sample_config* sc, const pp_gts_cand* cands,
                 const int32_t* cand_counts, float* points_out, int64_t points_capacity, int32_t* offsets_out,
                 float* boxes_out, int32_t* classes_out, uint8_t* valid_out, int32_t* counts_out) {
    if (!e) return PP_ERR_ARG;
    if (!points_out || !offsets_out || !boxes_out || !classes_out || !valid_out || !counts_out)
        return fail(e, PP_ERR_ARG, "pp_gt_sample: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_gt_sample: a training step is in flight");
    if (e->db.n < 0) return fail(e, PP_ERR_STATE, "pp_gt_sample: no database loaded (pp_gtdb_load)");
    const pp_target_config tc = {0.5f, 0.35f, {0, 0}};
    int64_t total = 0;
    int max_out_n = 0;
    std::vector<int> bound_off;
    int st = check_gt(e, "pp_gt_sample", gt_boxes, gt_classes, gt_counts, batch, &tc, &total);
    if (st == PP_OK) st = check_gts(e, "pp_gt_sample", gt_counts, batch, sc, cands, cand_counts, &max_out_n, &bound_off);
    if (st) return st;
    const int64_t bound_total = bound_off[(size_t)batch];
    if (points_capacity < bound_total)
        return fail(e, PP_ERR_ARG, "%s: points_out holds %lld points, up to %lld are written", "pp_gt_sample",
                    (long long)points_capacity, (long long)bound_total);
    (void)hipSetDevice(e->device);
    prof_reset(e);
    if ((st = enqueue_gt_sample(e, batch, gt_boxes, gt_classes, gt_valid, gt_counts, total, sc, cands, cand_counts, max_out_n,
                                e->stream)))
        return st;
    hipStream_t s = e->stream;
    HIPCHK(e, hipMemcpyAsync(offsets_out, e->gts.offsets, (size_t)(batch + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(counts_out, e->gts.out.cnt, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    // the counts read back replace the host's copy of the offsets: everything downstream is sized from them
    const int64_t n_new = offsets_out[batch];
    int64_t kept = 0;
    int max_n = 0;
    for (int b = 0; b < batch; ++b) {
        kept += counts_out[b];
        max_n = std::max(max_n, offsets_out[b + 1] - offsets_out[b]);
    }
    if (n_new > bound_total || max_n > e->NMAX) return fail(e, PP_ERR_HIP, "pp_gt_sample: the device wrote past its bound");
    if (n_new) HIPCHK(e, hipMemcpyAsync(e->d_points, e->spare_pts, (size_t)n_new * e->F * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(e, hipMemcpyAsync(e->d_offsets, e->gts.offsets, (size_t)(batch + 1) * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (n_new) HIPCHK(e, hipMemcpyAsync(points_out, e->spare_pts, (size_t)n_new * e->F * sizeof(float), hipMemcpyDeviceToHost, s));
    if (kept) {
        HIPCHK(e, hipMemcpyAsync(boxes_out, e->gts.out.boxes, (size_t)kept * 7 * sizeof(float), hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipMemcpyAsync(classes_out, e->gts.out.cls, (size_t)kept * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(e, hipMemcpyAsync(valid_out, e->gts.out.valid, (size_t)kept, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(e, hipStreamSynchronize(s));
    set_resident(e, batch, offsets_out, max_n, true);
    return PP_OK;
}

// ---- building the object database from the resident frames (gt_database.hip) ----

namespace {

int ensure_gdb(pp_engine* e, int stride) {
    pp_engine::Gdb& g = e->gdb;
    if (g.ready) return PP_OK;
    const size_t B = (size_t)e->B, gmax = B * PP_MAX_GT_PER_FRAME;
    DevAlloc A{e};
    A(&g.boxes, gmax * 7); A(&g.cnt, B); A(&g.boxoff, B + 1); A(&g.planes, gmax);
    A(&g.chunks, gmax * stride); A(&g.totals, gmax); A(&g.off, gmax + 1);
    g.ready = A.st == PP_OK;
    return A.st;
}

int gtdb_run(pp_engine* e, const char* who, const double* boxes, const int32_t* box_counts, int32_t batch,
             int32_t* counts_out, int64_t* offsets_out, float* points_out, int64_t points_capacity, bool gather) {
    if (!box_counts || !counts_out || (gather && (!offsets_out || points_capacity < 0)))
        return fail(e, PP_ERR_ARG, "%s: null argument", who);
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    int st = check_batch(e, batch); if (st) return st;
    if (e->cur_batch != batch) return fail(e, PP_ERR_ARG, "%s: %d frames are resident, batch is %d", who, e->cur_batch, batch);
    if ((st = require_host_exact(e, who))) return st;
    // k_gdb_offsets scans 32-bit partial sums inside a wave: 64 threads x max_batch objects x max_points_per_frame points
    if ((int64_t)e->B * e->NMAX > (1ll << 25))
        return fail(e, PP_ERR_UNSUPPORTED, "%s: max_batch x max_points_per_frame above 2^25", who);
    int64_t total = 0;
    if ((st = check_counts(e, who, box_counts, batch, &total))) return st;
    std::vector<int> boxoff((size_t)batch + 1, 0);
    for (int b = 0; b < batch; ++b) boxoff[(size_t)b + 1] = boxoff[(size_t)b] + box_counts[b];
    if (total > 0 && !boxes) return fail(e, PP_ERR_ARG, "%s: boxes is NULL", who);
    if ((st = check_boxes(e, who, boxes, total))) return st;
    (void)hipSetDevice(e->device);
    const int stride = (e->NMAX + PP_GDB_CHUNK - 1) / PP_GDB_CHUNK;
    if ((st = ensure_gdb(e, stride))) return st;
    pp_engine::Gdb& g = e->gdb;
    hipStream_t s = e->stream;
    prof_reset(e);
    if (total) HIPCHK(e, hipMemcpyAsync(g.boxes, boxes, (size_t)total * 7 * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(g.cnt, box_counts, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(e, hipMemcpyAsync(g.boxoff, boxoff.data(), ((size_t)batch + 1) * sizeof(int), hipMemcpyHostToDevice, s));
    GdbParams p;
    p.batch = batch; p.F = e->F; p.offsets = e->d_offsets;
    // (the frames stay as they are: a later pp_detect_async reads the same feed)
    if ((st = resident_points(e, batch, s, false, &p.pts))) return st;
    p.boxes = g.boxes; p.box_cnt = g.cnt; p.box_off = g.boxoff; p.planes = g.planes;
    p.chunk_cnt = g.chunks; p.chunk_stride = stride; p.totals = g.totals; p.obj_off = g.off;
    p.out = nullptr;
    {
        ProfScope ps(e, nullptr);      // each launch under its own name
        launch_gtdb_count(p, (int)total, e->cur_max_n, s);
    }
    HIPCHK(e, hipGetLastError());
    std::vector<long long> off((size_t)total + 1, 0);
    if (total) HIPCHK(e, hipMemcpyAsync(counts_out, g.totals, (size_t)total * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipMemcpyAsync(off.data(), g.off, ((size_t)total + 1) * sizeof(long long), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    if (!gather) return PP_OK;
    const int64_t rows = off[(size_t)total];
    if (rows > points_capacity)
        return fail(e, PP_ERR_ARG, "%s: points_out holds %lld points, %lld are written", who, (long long)points_capacity,
                    (long long)rows);
    if (rows > 0 && !points_out) return fail(e, PP_ERR_ARG, "%s: points_out is NULL", who);
    for (int64_t i = 0; i <= total; ++i) offsets_out[i] = off[(size_t)i];
    if (rows == 0) return PP_OK;
    if ((st = dgrow(e, &g.out, &g.cap_out, (size_t)rows * e->F))) return st;
    p.out = g.out;
    {
        ProfScope ps(e, nullptr);
        launch_gtdb_gather(p, e->cur_max_n, s);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(points_out, g.out, (size_t)rows * e->F * sizeof(float), hipMemcpyDeviceToHost, s));
    HIPCHK(e, hipStreamSynchronize(s));
    return PP_OK;
}

}  // namespace

int pp_gtdb_count(pp_handle e, const double* boxes, const int32_t* box_counts, int32_t batch, int32_t* counts_out) {
    if (!e) return PP_ERR_ARG;
    return gtdb_run(e, "pp_gtdb_count", boxes, box_counts, batch, counts_out, nullptr, nullptr, 0, false);
}

int pp_gtdb_build(pp_handle e, const double* boxes, const int32_t* box_counts, int32_t batch, int32_t* counts_out,
                  int64_t* offsets_out, float* points_out, int64_t points_capacity) {
    if (!e) return PP_ERR_ARG;
    return gtdb_run(e, "pp_gtdb_build", boxes, box_counts, batch, counts_out, offsets_out, points_out, points_capacity, true);
}

int pp_gt_sample_info(pp_handle e, int32_t* status, int32_t* point_counts, int32_t* round_used, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_gt_sample_info: a training step is in flight");
    if (e->gts.batch < 1) return fail(e, PP_ERR_STATE, "pp_gt_sample_info: no pp_gt_sample has run");
    if (batch != e->gts.batch) return fail(e, PP_ERR_ARG, "pp_gt_sample_info: the last pp_gt_sample had %d frames, batch is %d", e->gts.batch, batch);
    (void)hipSetDevice(e->device);
    const size_t n = (size_t)batch * PP_GTS_MAX_CAND;
    if (status) HIPCHK(e, hipMemcpyAsync(status, e->gts.status, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (point_counts) HIPCHK(e, hipMemcpyAsync(point_counts, e->gts.counts, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (round_used) HIPCHK(e, hipMemcpyAsync(round_used, e->gts.round, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

int pp_augment_selected(pp_handle e, int32_t* selected, int64_t capacity, int64_t* count) {
    if (!e) return PP_ERR_ARG;
    if (!count || (capacity > 0 && !selected)) return fail(e, PP_ERR_ARG, "pp_augment_selected: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_augment_selected: a training step is in flight");
    if (!e->off_host_exact)      // the draw rows were allotted per frame: which of them are boxes is a device value
        return fail(e, PP_ERR_STATE, "pp_augment_selected: the last augmentation ran inside a sampled training step");
    (void)hipSetDevice(e->device);
    *count = e->aug.total;
    const int64_t n = std::min<int64_t>(capacity, e->aug.total);
    if (n > 0) {
        HIPCHK(e, hipMemcpyAsync(selected, e->aug.sel, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(e, hipStreamSynchronize(e->stream));
    }
    return PP_OK;
}
int pp_assign_targets(pp_handle e, const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_counts,
                      int32_t batch, const uint8_t* anchors_mask, const pp_target_config* tc, int32_t* labels,
                      float* reg_targets, int32_t* gt_index, float* overlap) {
    if (!e) return PP_ERR_ARG;
    if (!labels || !reg_targets) return fail(e, PP_ERR_ARG, "pp_assign_targets: null argument");
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_assign_targets: anchors not set");
    int64_t total = 0;
    int st = check_gt(e, "pp_assign_targets", gt_boxes, gt_classes, gt_counts, batch, tc, &total);
    if (st) return st;
    if (!anchors_mask && e->cur_batch != batch)
        return fail(e, PP_ERR_STATE, "pp_assign_targets: %d frames are resident, batch is %d (upload the frames or pass "
                    "anchors_mask)", e->cur_batch, batch);
    (void)hipSetDevice(e->device);
    if ((st = ensure_loss_buffers(e))) return st;
    const bool extra = gt_index || overlap;
    if (extra && !e->tgt.overlap) {
        DevAlloc A{e};
        A(&e->tgt.index, (size_t)e->B * e->A); A(&e->tgt.overlap, (size_t)e->B * e->A);
        if (A.st) return A.st;
    }
    if (anchors_mask) {
        HIPCHK(e, hipMemcpyAsync(e->tgt.mask, anchors_mask, (size_t)batch * e->A, hipMemcpyHostToDevice, e->stream));
    } else {
        // the resident frames' cell map: voxelised at upload time (wait for it) or here
        if ((st = wait_for_upload(e, e->stream))) return st;
        if (!e->vox_ahead && (st = run_voxelize(e, batch, e->cur_max_n))) return st;
    }
    prof_reset(e);
    if ((st = targets_from_host(e, batch, gt_boxes, gt_classes, gt_counts, total, anchors_mask == nullptr, tc, extra, e->stream)))
        return st;
    const size_t n = (size_t)batch * e->A;
    HIPCHK(e, hipMemcpyAsync(labels, e->loss.labels, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipMemcpyAsync(reg_targets, e->loss.regt, n * 7 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    if (gt_index) HIPCHK(e, hipMemcpyAsync(gt_index, e->tgt.index, n * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    if (overlap) HIPCHK(e, hipMemcpyAsync(overlap, e->tgt.overlap, n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

}  // extern "C"
