// C-ABI, the rolling occupancy map per stream (pp_set_occupancy, pp_occupancy_update_async, pp_get_occupancy,
// pp_occupancy_info, pp_occupancy_reset): the resident points of frame b under stream b's sensor-to-fixed pose -> the
// stream's log-odds window in the fixed frame and its int8 grid, on the device (kernels: occupancy.hip; the rule:
// occupancy.py).  The window's origin is host arithmetic (floor(t / resolution) in float64), so the host keeps it; the
// device keeps two copies of every stream's state and an update writes the one the stream does not hold.
#include "pp_engine.h"

static_assert(sizeof(pp_occupancy_config) == 56, "pp_occupancy_config: 4 doubles, 6 int32 (the Python binding mirrors it)");
static_assert(PP_OCC_MAX_CELLS == 1048576, "width * height of an occupancy window");

namespace {

constexpr int OCC_TABLE_MAX = 2001;         // l_max - l_min + 1 at most
constexpr double OCC_CELL_LIMIT = 1073741824.0;   // |t| / resolution from which a pose is refused: 2^30

void free_buffers(pp_engine* e) {
    pp_engine::Occupancy& g = e->occ;
    g.mem.release();
    g.cells = 0; g.pitch = 0; g.list_cap = 0; g.batch = 0;
}

void forget(pp_engine* e, int b0, int nb) {
    pp_engine::Occupancy& g = e->occ;
    for (int b = b0; b < b0 + nb; ++b) { g.has[(size_t)b] = 0; g.cleared[(size_t)b] = 0; }
}

// Everything pp_set_occupancy refuses of a configuration, by field name.
int check_config(pp_engine* e, const pp_occupancy_config& c) {
    const char* who = "pp_set_occupancy";
    if (int st = check_cfg_doubles(e, who, {{"resolution", c.resolution, true}, {"z_min", c.z_min, false}, {"z_max", c.z_max, false},
                                            {"max_range", c.max_range, true}})) return st;
    if (!(c.resolution > 0.0)) return fail(e, PP_ERR_ARG, "pp_set_occupancy: resolution = %g must be > 0", c.resolution);
    if (!(c.max_range > 0.0)) return fail(e, PP_ERR_ARG, "pp_set_occupancy: max_range = %g must be > 0", c.max_range);
    if (c.z_min > c.z_max) return fail(e, PP_ERR_ARG, "pp_set_occupancy: z_min = %g above z_max = %g", c.z_min, c.z_max);
    if (int st = check_cfg_window(e, who, c.width, c.height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    if (c.l_hit < 1 || c.l_hit > 1000) return fail(e, PP_ERR_ARG, "pp_set_occupancy: l_hit = %d outside [1, 1000]", c.l_hit);
    if (c.l_miss < 1 || c.l_miss > 1000) return fail(e, PP_ERR_ARG, "pp_set_occupancy: l_miss = %d outside [1, 1000]", c.l_miss);
    if (c.l_min < -1000 || c.l_min >= 0) return fail(e, PP_ERR_ARG, "pp_set_occupancy: l_min = %d outside [-1000, -1]", c.l_min);
    if (c.l_max <= 0 || c.l_max > 1000) return fail(e, PP_ERR_ARG, "pp_set_occupancy: l_max = %d outside [1, 1000]", c.l_max);
    return PP_OK;
}

// what the handle keeps whatever the window's shape: the table, the calls' buffers, the streams' host state
int make_fixed(pp_engine* e) {
    pp_engine::Occupancy& g = e->occ;
    const size_t B = (size_t)e->B;
    if (g.has.size() != B) {
        g.has.assign(B, 0); g.ox.assign(B, 0); g.oy.assign(B, 0); g.cur.assign(B, 0); g.cleared.assign(B, 0);
    }
    HIPCHK(e, g.h_call.alloc(g.ring, B));
    if (g.d_call) return PP_OK;
    DevAlloc A{e};
    A(&g.table, OCC_TABLE_MAX); A(&g.info, B * PP_OCC_INFO); A(&g.d_call, B);     // (d_call last: the ready flag)
    return A.st;
}

int make_buffers(pp_engine* e, int pitch, size_t cells, int list_cap) {
    pp_engine::Occupancy& g = e->occ;
    const size_t B = (size_t)e->B;
    const size_t bytes = B * cells * (4 + 1 + 2 * (2 + 1)) + B * (size_t)list_cap * sizeof(int);
    StageMem& M = g.mem;
    M(&g.marks, B * cells); M(&g.passed, B * cells); M(&g.list, B * (size_t)list_cap);
    for (int k = 0; k < 2; ++k) { M(&g.logodds[k], B * cells); M(&g.grid[k], B * cells); }
    if (hipError_t st = M.failed()) {
        (void)hipGetLastError();
        return fail(e, PP_ERR_HIP, "pp_set_occupancy: %d streams x %zu cells (rows of %d) need %zu bytes of device memory and the "
                    "device cannot hold them (%s): lower width or height", e->B, cells, pitch, bytes, hipGetErrorString(st));
    }
    g.pitch = pitch; g.cells = cells; g.list_cap = list_cap;
    return PP_OK;
}

}  // namespace

void occupancy_release(pp_engine* e) {
    free_buffers(e);
    e->occ.ring.release();
    e->occ = pp_engine::Occupancy();
}

extern "C" {

int pp_set_occupancy(pp_handle e, const pp_occupancy_config* cfg, const int8_t* cost_table, int32_t n_table) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_occupancy: a training step is in flight");
    pp_engine::Occupancy& g = e->occ;
    if (!cfg) { g.on = false; return PP_OK; }
    const pp_occupancy_config c = *cfg;
    if (int st = check_config(e, c)) return st;
    const int rows = c.l_max - c.l_min + 1;
    int8_t table[OCC_TABLE_MAX];
    if (cost_table) {
        if (n_table != rows)
            return fail(e, PP_ERR_ARG, "pp_set_occupancy: cost_table has %d entries, l_max - l_min + 1 = %d", n_table, rows);
        for (int i = 0; i < rows; ++i) {
            if (cost_table[i] < 0 || cost_table[i] > 100)
                return fail(e, PP_ERR_ARG, "pp_set_occupancy: cost_table[%d] = %d outside [0, 100]", i, (int)cost_table[i]);
            table[i] = cost_table[i];
        }
    } else {
        for (int i = 0; i < rows; ++i)
            table[i] = (int8_t)std::floor(100.0 / (1.0 + std::exp(-(double)(c.l_min + i) / 100.0)) + 0.5);
    }
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // an update in flight uses the table and the buffers to its end
    if (int st = make_fixed(e)) return st;
    const int pitch = (c.width + 3) & ~3;
    const size_t cells = (size_t)pitch * c.height;
    const int list_cap = (int)std::min<long long>((long long)c.width * c.height, (long long)e->NMAX);
    const pp_occupancy_config& o = g.cfg;
    const bool same_map = g.cells != 0 && o.width == c.width && o.height == c.height && o.resolution == c.resolution &&
                          o.l_hit == c.l_hit && o.l_miss == c.l_miss && o.l_min == c.l_min && o.l_max == c.l_max;
    if (cells != g.cells || pitch != g.pitch || list_cap != g.list_cap) {
        g.on = false;
        free_buffers(e);
        if (int st = make_buffers(e, pitch, cells, list_cap)) return st;
    }
    if (!same_map) {
        forget(e, 0, e->B);
        g.batch = 0;
    }
    HIPCHK(e, hipMemcpy(g.table, table, (size_t)rows, hipMemcpyHostToDevice));
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_occupancy_config(pp_handle e, int32_t* on, pp_occupancy_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->occ.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->occ.cfg;
    return PP_OK;
}

int pp_occupancy_update_async(pp_handle e, const double* poses, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_occupancy_update_async";
    pp_engine::Occupancy& g = e->occ;
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the occupancy stage is not configured (pp_set_occupancy first)", who);
    if (!poses) return fail(e, PP_ERR_ARG, "%s: poses is NULL", who);
    if (int st = check_resident_call(e, who, batch, "upload or ingest frames first")) return st;
    const pp_occupancy_config& c = g.cfg;
    if (int st = check_poses(e, who, poses, nullptr, batch, [&](int b, const double* P) {
        if (!(std::fabs(P[3] / c.resolution) < OCC_CELL_LIMIT) || !(std::fabs(P[7] / c.resolution) < OCC_CELL_LIMIT))
            return fail(e, PP_ERR_ARG, "%s: poses: the translation of stream %d (%g, %g) is 2^30 cells of %g m or more from the origin",
                        who, b, P[3], P[7], c.resolution);
        return (int)PP_OK;
    })) return st;
    const unsigned long long* mask = nullptr;
    int mask_stride = 0;
    if (int st = object_mask_for(e, who, PP_OBJMASK_OCCUPANCY, batch, &mask, &mask_stride)) return st;
    const unsigned long long *cls_gnd = nullptr, *cls_obs = nullptr;
    int cls_stride = 0;
    if (int st = ground_for(e, who, PP_GROUND_OCCUPANCY, batch, &cls_gnd, &cls_obs, &cls_stride)) return st;
    (void)hipSetDevice(e->device);
    int slot;
    HIPCHK(e, g.ring.take(&slot));
    OccCall* call = g.h_call.at(slot);
    std::vector<int> cleared((size_t)batch, 0);
    const int W = c.width, H = c.height;
    for (int b = 0; b < batch; ++b) {
        const double* P = poses + (size_t)b * 12;
        OccCall& k = call[b];
        memset(&k, 0, sizeof(k));
        for (int j = 0; j < 3; ++j) { k.r0[j] = P[j]; k.r1[j] = P[4 + j]; }
        k.tx = P[3]; k.ty = P[7];
        k.ox = (int)std::floor(P[3] / c.resolution) - W / 2;
        k.oy = (int)std::floor(P[7] / c.resolution) - H / 2;
        k.src = g.cur[(size_t)b];
        const long long sx = (long long)k.ox - g.ox[(size_t)b], sy = (long long)k.oy - g.oy[(size_t)b];
        k.fresh = !g.has[(size_t)b] || std::llabs(sx) >= W || std::llabs(sy) >= H;
        k.sdx = k.fresh ? 0 : (int)sx;
        k.sdy = k.fresh ? 0 : (int)sy;
        const long long kept = k.fresh ? 0 : (W - std::llabs(sx)) * (H - std::llabs(sy));
        cleared[(size_t)b] = (int)((long long)W * H - kept);
    }
    OccParams p;
    memset(&p, 0, sizeof(p));
    if (int st = resident_points(e, batch, e->stream, false, &p.points)) return st;
    p.cfg = c;
    p.batch = batch; p.F = e->F; p.pitch = g.pitch; p.max_n = std::min(e->cur_max_n, e->NMAX); p.list_cap = g.list_cap;
    p.offsets = e->d_offsets;
    p.call = g.d_call;
    p.marks = g.marks; p.passed = g.passed; p.list = g.list; p.info = g.info;
    p.logodds[0] = g.logodds[0]; p.logodds[1] = g.logodds[1];
    p.grid[0] = g.grid[0]; p.grid[1] = g.grid[1];
    p.table = g.table;
    p.mask = mask; p.mask_stride = mask_stride;
    p.gnd = cls_gnd; p.obs = cls_obs; p.cls_stride = cls_stride;
    prof_reset(e);
    HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
    HIPCHK(e, g.ring.sent(slot, e->stream));
    // the marks and the tallies of this call's streams
    HIPCHK(e, hipMemsetAsync(g.marks, 0, (size_t)batch * g.cells * sizeof(unsigned), e->stream));
    HIPCHK(e, hipMemsetAsync(g.passed, 0, (size_t)batch * g.cells, e->stream));
    HIPCHK(e, hipMemsetAsync(g.info, 0, (size_t)batch * PP_OCC_INFO * sizeof(int), e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_occupancy(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload but one writes the buffer read here: its writer waits for this event as for a pass
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    for (int b = 0; b < batch; ++b) {
        g.has[(size_t)b] = 1;
        g.ox[(size_t)b] = call[b].ox; g.oy[(size_t)b] = call[b].oy;
        g.cur[(size_t)b] = 1 - call[b].src;
        g.cleared[(size_t)b] = cleared[(size_t)b];
    }
    g.batch = batch;
    return PP_OK;
}

int pp_get_occupancy(pp_handle e, int8_t* grid, int16_t* logodds, double* origins, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (!grid) return fail(e, PP_ERR_ARG, "pp_get_occupancy: grid is NULL");
    if (!origins) return fail(e, PP_ERR_ARG, "pp_get_occupancy: origins is NULL");
    pp_engine::Occupancy& g = e->occ;
    if (int st = check_last_run(e, "pp_get_occupancy", g.marks ? g.batch : 0, batch, true,
                                "no update has run (pp_occupancy_update_async first)", "update", "streams")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // rows of `pitch` cells on the device, of `width` on the host
    const size_t W = (size_t)g.cfg.width, H = (size_t)g.cfg.height;
    for (int b = 0; b < batch; ++b) {
        int8_t* gb = grid + (size_t)b * W * H;
        int16_t* lb = logodds ? logodds + (size_t)b * W * H : nullptr;
        if (!g.has[(size_t)b]) {                           // reset since the update
            memset(gb, 0xff, W * H);
            if (lb) memset(lb, 0, W * H * sizeof(int16_t));
            origins[2 * b] = origins[2 * b + 1] = NAN;
            continue;
        }
        const int k = g.cur[(size_t)b];
        HIPCHK(e, hipMemcpy2D(gb, W, g.grid[k] + (size_t)b * g.cells, (size_t)g.pitch, W, H, hipMemcpyDeviceToHost));
        if (lb) HIPCHK(e, hipMemcpy2D(lb, W * 2, g.logodds[k] + (size_t)b * g.cells, (size_t)g.pitch * 2, W * 2, H, hipMemcpyDeviceToHost));
        origins[2 * b] = (double)g.ox[(size_t)b] * g.cfg.resolution;
        origins[2 * b + 1] = (double)g.oy[(size_t)b] * g.cfg.resolution;
    }
    return PP_OK;
}

int pp_occupancy_info(pp_handle e, int32_t* hits, int32_t* ground, int32_t* ignored, int32_t* cells_hit, int32_t* cells_free,
                      int32_t* cleared, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    pp_engine::Occupancy& g = e->occ;
    if (int st = check_last_run(e, "pp_occupancy_info", g.marks ? g.batch : 0, batch, true,
                                "no update has run (pp_occupancy_update_async first)", "update", "streams")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<int> info((size_t)batch * PP_OCC_INFO, 0);
    HIPCHK(e, hipMemcpy(info.data(), g.info, info.size() * sizeof(int), hipMemcpyDeviceToHost));
    int32_t* outs[5] = {hits, ground, ignored, cells_hit, cells_free};
    for (int b = 0; b < batch; ++b) {
        for (int k = 0; k < 5; ++k)
            if (outs[k]) outs[k][b] = info[(size_t)b * PP_OCC_INFO + k];
        if (cleared) cleared[b] = g.cleared[(size_t)b];
    }
    return PP_OK;
}

int pp_occupancy_masked(pp_handle e, int32_t* masked, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (!masked) return fail(e, PP_ERR_ARG, "pp_occupancy_masked: masked is NULL");
    pp_engine::Occupancy& g = e->occ;
    if (int st = check_last_run(e, "pp_occupancy_masked", g.marks ? g.batch : 0, batch, true,
                                "no update has run (pp_occupancy_update_async first)", "update", "streams")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy2D(masked, sizeof(int), g.info + 6, PP_OCC_INFO * sizeof(int), sizeof(int), (size_t)batch, hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_occupancy_reset(pp_handle e, int32_t stream) {
    if (!e) return PP_ERR_ARG;
    if (stream < -1 || stream >= e->B)
        return fail(e, PP_ERR_ARG, "pp_occupancy_reset: stream %d outside [0, max_batch=%d) (-1: all)", stream, e->B);
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_occupancy_reset: a training step is in flight");
    if (e->occ.has.empty()) return PP_OK;
    if (stream < 0) forget(e, 0, e->B);
    else forget(e, stream, 1);
    return PP_OK;
}

}  // extern "C"
