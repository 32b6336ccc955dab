// C-ABI, the obstacle costmap per frame (pp_set_costmap, pp_costmap_async, pp_get_costmaps, pp_costmap_info): the resident
// points and the last pass's detections or the streams' track tables -> one int8 grid per frame, on the device (kernels:
// costmap.hip; the rule: costmap.py).  A stage behind the pass, queued on the handle's stream as plain launches.
#include "pp_engine.h"

static_assert(sizeof(pp_costmap_config) == 128, "pp_costmap_config: 8 doubles, 16 int32 (the Python binding mirrors it)");
static_assert(PP_CM_TRACK_ROWS == 576, "a stream's tracks leave at most 64 x (1 + 8) footprints");

namespace {

void free_buffers(pp_engine* e) {
    pp_engine::Costmap& g = e->cmap;
    g.mem.release();
    g.cells = 0; g.pitch = 0; g.table_rows = 0; g.batch = 0;
}

// Everything pp_set_costmap refuses of a configuration, by field name.
int check_config(pp_engine* e, const pp_costmap_config& c) {
    const char* who = "pp_set_costmap";
    if (int st = check_cfg_doubles(e, who, {{"x_min", c.x_min, true}, {"y_min", c.y_min, true}, {"resolution", c.resolution, true},
                                            {"z_min", c.z_min, false}, {"z_max", c.z_max, false}, {"pad", c.pad, true},
                                            {"min_score", c.min_score, true}, {"horizon_dt", c.horizon_dt, true}})) return st;
    if (!(c.resolution > 0.0)) return fail(e, PP_ERR_ARG, "pp_set_costmap: resolution = %g must be > 0", c.resolution);
    if (!(c.pad >= 0.0)) return fail(e, PP_ERR_ARG, "pp_set_costmap: pad = %g must be >= 0", c.pad);
    if (!(c.horizon_dt > 0.0)) return fail(e, PP_ERR_ARG, "pp_set_costmap: horizon_dt = %g must be > 0", c.horizon_dt);
    if (c.z_min > c.z_max) return fail(e, PP_ERR_ARG, "pp_set_costmap: z_min = %g above z_max = %g", c.z_min, c.z_max);
    if (int st = check_cfg_window(e, who, c.width, c.height, PP_COSTMAP_MAX_CELLS, "PP_COSTMAP_MAX_CELLS")) return st;
    if (c.min_points < 1) return fail(e, PP_ERR_ARG, "pp_set_costmap: min_points = %d must be >= 1", c.min_points);
    if (c.objects < 0 || c.objects > 2) return fail(e, PP_ERR_ARG, "pp_set_costmap: objects = %d (0 none, 1 detections, 2 tracks)", c.objects);
    if (c.horizon_steps < 0 || c.horizon_steps > PP_COSTMAP_MAX_STEPS)
        return fail(e, PP_ERR_ARG, "pp_set_costmap: horizon_steps = %d outside [0, PP_COSTMAP_MAX_STEPS = %d]", c.horizon_steps, PP_COSTMAP_MAX_STEPS);
    if (c.point_cost < 0 || c.point_cost > 100) return fail(e, PP_ERR_ARG, "pp_set_costmap: point_cost = %d outside [0, 100]", c.point_cost);
    if (c.object_cost < 0 || c.object_cost > 100) return fail(e, PP_ERR_ARG, "pp_set_costmap: object_cost = %d outside [0, 100]", c.object_cost);
    for (int k = 0; k < c.horizon_steps; ++k)
        if (c.predict_cost[k] < 0 || c.predict_cost[k] > 100)
            return fail(e, PP_ERR_ARG, "pp_set_costmap: predict_cost[%d] = %d outside [0, 100]", k, c.predict_cost[k]);
    return PP_OK;
}

int make_buffers(pp_engine* e, int pitch, size_t cells) {
    pp_engine::Costmap& g = e->cmap;
    const size_t B = (size_t)e->B;
    const int hdr = (int)((B + 3) & ~(size_t)3);          // the count words stay 16-byte aligned behind the tallies
    const int rows = std::max((int)PP_CM_TRACK_ROWS, e->ncls * e->cfg.nms_post_max_size);
    const size_t bytes = (hdr + B * cells) * 4 + B * cells + B * cells * 4 + B * rows * sizeof(CmFootprint) + 2 * B * sizeof(int);
    StageMem& M = g.mem;
    M(&g.words, hdr + B * cells); M(&g.grid, B * cells); M(&g.tap, B * cells); M(&g.table, B * rows); M(&g.info, 2 * B);
    if (hipError_t st = M.failed()) {
        (void)hipGetLastError();
        return fail(e, PP_ERR_HIP, "pp_set_costmap: %d streams x %zu cells (rows of %d) need %zu bytes of device memory and the "
                    "device cannot hold them (%s): lower width or height", e->B, cells, pitch, bytes, hipGetErrorString(st));
    }
    g.pitch = pitch; g.cells = cells; g.hdr = hdr; g.table_rows = rows;
    HIPCHK(e, hipMemset(g.info, 0, 2 * B * sizeof(int)));
    return PP_OK;
}

}  // namespace

void costmap_release(pp_engine* e) {
    free_buffers(e);
    e->cmap = pp_engine::Costmap();
}

extern "C" {

int pp_set_costmap(pp_handle e, const pp_costmap_config* cfg) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_costmap: a training step is in flight");
    pp_engine::Costmap& g = e->cmap;
    if (!cfg) { g.on = false; return PP_OK; }
    pp_costmap_config c = *cfg;
    if (int st = check_config(e, c)) return st;
    c.confirmed_only = c.confirmed_only ? 1 : 0;
    (void)hipSetDevice(e->device);
    const int pitch = (c.width + 3) & ~3;
    const size_t cells = (size_t)pitch * c.height;
    if (cells != g.cells || pitch != g.pitch) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a run in flight uses the old buffers to its end
        g.on = false;
        free_buffers(e);
        if (int st = make_buffers(e, pitch, cells)) return st;
    }
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_costmap_config(pp_handle e, int32_t* on, pp_costmap_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->cmap.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->cmap.cfg;
    return PP_OK;
}

int pp_costmap_async(pp_handle e) {
    if (!e) return PP_ERR_ARG;
    pp_engine::Costmap& g = e->cmap;
    if (!g.on) return fail(e, PP_ERR_STATE, "pp_costmap_async: the costmap stage is not configured (pp_set_costmap first)");
    if (int st = check_resident_call(e, "pp_costmap_async", e->cur_batch, "upload or ingest frames first")) return st;   // (the call has no batch of its own)
    const pp_costmap_config& c = g.cfg;
    const int B = e->cur_batch;
    if (c.objects == 1 && (e->results_batch != B || e->results_gen != e->resident_gen || e->results_rows < 1))
        return fail(e, PP_ERR_STATE, "pp_costmap_async: objects = detections and no pass has run on the resident frames (pp_detect_async first)");
    if (c.objects == 2 && !e->trk.configured)
        return fail(e, PP_ERR_STATE, "pp_costmap_async: objects = tracks and pp_set_tracking has given no configuration");
    (void)hipSetDevice(e->device);
    CostmapParams p;
    memset(&p, 0, sizeof(p));
    if (int st = object_mask_for(e, "pp_costmap_async", PP_OBJMASK_COSTMAP, B, &p.mask, &p.mask_stride)) return st;
    if (int st = ground_for(e, "pp_costmap_async", PP_GROUND_COSTMAP, B, &p.gnd, &p.obs, &p.cls_stride)) return st;
    if (int st = resident_points(e, B, e->stream, false, &p.points)) return st;
    p.cfg = c;
    p.batch = B; p.F = e->F; p.pitch = g.pitch; p.max_n = std::min(e->cur_max_n, e->NMAX);
    p.offsets = e->d_offsets;
    p.dets = e->d_dets; p.n_dets = e->d_ndets; p.det_rows = c.objects == 1 ? e->results_rows : 0;
    p.slots = e->trk.state;
    p.table = g.table; p.table_rows = g.table_rows;
    p.n_fp = g.info; p.flagged = g.info + e->B;
    p.in_grid = reinterpret_cast<int*>(g.words);
    p.words = g.words + g.hdr;
    p.grid = g.grid; p.tap = g.tap;
    prof_reset(e);
    // the tallies and the count words of this run's frames: a smaller batch after a larger one starts from zero as well
    HIPCHK(e, hipMemsetAsync(g.words, 0, ((size_t)g.hdr + (size_t)B * g.cells) * sizeof(unsigned), e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_costmap(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload but one writes the buffer read here: its writer waits for this event as for a pass
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    g.batch = B; g.run_pitch = g.pitch; g.run_w = c.width; g.run_h = c.height; g.run_objects = c.objects;
    g.run_res = c.resolution;
    return PP_OK;
}

int pp_get_costmaps(pp_handle e, int8_t* grid, int32_t* counts, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (!grid) return fail(e, PP_ERR_ARG, "pp_get_costmaps: grid is NULL");
    pp_engine::Costmap& g = e->cmap;
    if (int st = check_last_run(e, "pp_get_costmaps", g.grid ? g.batch : 0, batch, true,
                                "no costmap stage has run (pp_costmap_async first)", "run", "frames")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // rows of `pitch` cells on the device, of `width` on the host; the frames lie row behind row in both
    const size_t W = (size_t)g.run_w, rows = (size_t)batch * g.run_h;
    HIPCHK(e, hipMemcpy2D(grid, W, g.grid, (size_t)g.run_pitch, W, rows, hipMemcpyDeviceToHost));
    if (counts) HIPCHK(e, hipMemcpy2D(counts, W * 4, g.tap, (size_t)g.run_pitch * 4, W * 4, rows, hipMemcpyDeviceToHost));
    if (g.run_objects == 1) {
        std::vector<int> flagged((size_t)batch, 0);
        HIPCHK(e, hipMemcpy(flagged.data(), g.info + e->B, (size_t)batch * sizeof(int), hipMemcpyDeviceToHost));
        for (int& f : flagged) f = f ? PP_NDETS_NONFINITE : 0;
        if (int st = check_numeric(e, flagged.data(), batch, "pp_get_costmaps")) return st;
    }
    return PP_OK;
}

int pp_costmap_info(pp_handle e, int32_t* points_in_grid, int32_t* footprints, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    pp_engine::Costmap& g = e->cmap;
    if (int st = check_last_run(e, "pp_costmap_info", g.grid ? g.batch : 0, batch, true,
                                "no costmap stage has run (pp_costmap_async first)", "run", "frames")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    if (points_in_grid) HIPCHK(e, hipMemcpy(points_in_grid, g.words, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (footprints) HIPCHK(e, hipMemcpy(footprints, g.info, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
