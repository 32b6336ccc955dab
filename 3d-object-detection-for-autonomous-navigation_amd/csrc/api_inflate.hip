// C-ABI, obstacle inflation (pp_set_inflation, pp_get_inflation_config, pp_inflate_async, pp_get_inflated,
// pp_inflation_info, pp_inflate_grids): the int8 grid the costmap stage or the occupancy maps leave on the device -> the
// grid with every obstacle grown by the robot's radius and a falling cost beyond it, in buffers of the stage's own (kernel:
// inflate.hip; the rule: inflation.py).  A stage behind either source, queued on the handle's stream as one plain launch;
// nothing travels from the host per call, so it takes no call ring.  pp_inflate_grids needs no handle: host buffers in,
// host buffers out, device memory for the call's duration.
#include "pp_engine.h"

static_assert(sizeof(pp_inflation_config) == 40, "pp_inflation_config: 4 doubles, 2 int32 (the Python binding mirrors it)");
static_assert(PP_INFLATE_MAX_RADIUS == 64, "R: a row's nearest obstacle is looked for in three 64-bit words");
static_assert(PP_INFLATE_COSTMAP == 0 && PP_INFLATE_OCCUPANCY == 1, "pp_engine::infl is indexed by source");

namespace {

constexpr int INFL_TABLE_MAX = PP_INFLATE_MAX_RADIUS * PP_INFLATE_MAX_RADIUS + 1;

const char* source_name(int source) { return source == PP_INFLATE_COSTMAP ? "costmap" : "occupancy"; }

// Everything pp_set_inflation and pp_inflate_grids refuse of a configuration, by field name; *R on success.
int check_config(pp_engine* e, const char* who, const pp_inflation_config& c, int* R) {
    if (int st = check_cfg_doubles(e, who, {{"resolution", c.resolution, true}, {"inscribed_radius", c.inscribed_radius, true},
                                            {"inflation_radius", c.inflation_radius, true},
                                            {"cost_scaling_factor", c.cost_scaling_factor, true}})) return st;
    if (!(c.resolution > 0.0)) return fail(e, PP_ERR_ARG, "%s: resolution = %g must be > 0", who, c.resolution);
    if (!(c.inscribed_radius >= 0.0)) return fail(e, PP_ERR_ARG, "%s: inscribed_radius = %g must be >= 0", who, c.inscribed_radius);
    if (c.inflation_radius < c.inscribed_radius)
        return fail(e, PP_ERR_ARG, "%s: inflation_radius = %g below inscribed_radius = %g", who, c.inflation_radius, c.inscribed_radius);
    if (!(c.cost_scaling_factor > 0.0)) return fail(e, PP_ERR_ARG, "%s: cost_scaling_factor = %g must be > 0", who, c.cost_scaling_factor);
    if (c.lethal_threshold < 1 || c.lethal_threshold > 100)
        return fail(e, PP_ERR_ARG, "%s: lethal_threshold = %d outside [1, 100]", who, c.lethal_threshold);
    if (c.unknown_min_cost < 1 || c.unknown_min_cost > 100)
        return fail(e, PP_ERR_ARG, "%s: unknown_min_cost = %d outside [1, 100]", who, c.unknown_min_cost);
    const double cells = std::ceil(c.inflation_radius / c.resolution);
    if (!(cells <= (double)PP_INFLATE_MAX_RADIUS))
        return fail(e, PP_ERR_ARG, "%s: inflation_radius = %g is %g cells of %g m, at most PP_INFLATE_MAX_RADIUS = %d", who,
                    c.inflation_radius, cells, c.resolution, PP_INFLATE_MAX_RADIUS);
    *R = (int)cells;
    return PP_OK;
}

// The caller's table, checked, or the rule's own: dst [R * R + 1]
int fill_table(pp_engine* e, const char* who, const pp_inflation_config& c, int R, const int8_t* table, int n_table, int8_t* dst) {
    const int n = R * R + 1;
    if (table) {
        if (n_table != n) return fail(e, PP_ERR_ARG, "%s: table has %d entries, R * R + 1 = %d (R = %d cells)", who, n_table, n, R);
        for (int i = 0; i < n; ++i) {
            if (table[i] < 0 || table[i] > 100) return fail(e, PP_ERR_ARG, "%s: table[%d] = %d outside [0, 100]", who, i, (int)table[i]);
            dst[i] = table[i];
        }
        return PP_OK;
    }
    for (int i = 0; i < n; ++i) {
        const double d = std::sqrt((double)i) * c.resolution;
        dst[i] = i == 0 ? 100 : d <= c.inscribed_radius ? 99 : d <= c.inflation_radius
                 ? (int8_t)std::floor(98.0 * std::exp(-c.cost_scaling_factor * (d - c.inscribed_radius)) + 0.5) : 0;
    }
    return PP_OK;
}

int check_source(pp_engine* e, const char* who, int source) {
    if (source != PP_INFLATE_COSTMAP && source != PP_INFLATE_OCCUPANCY)
        return fail(e, PP_ERR_ARG, "%s: source = %d (0 PP_INFLATE_COSTMAP, 1 PP_INFLATE_OCCUPANCY)", who, source);
    return PP_OK;
}

}  // namespace

void inflate_release(pp_engine* e) {
    for (pp_engine::Inflation& g : e->infl) {
        g.mem.release();
        g = pp_engine::Inflation();
    }
}

extern "C" {

int pp_set_inflation(pp_handle e, int32_t source, const pp_inflation_config* cfg, const int8_t* table, int32_t n_table) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_inflation";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::Inflation& g = e->infl[source];
    if (!cfg) { g.on = false; return PP_OK; }
    const pp_inflation_config c = *cfg;
    int R = 0;
    if (int st = check_config(e, who, c, &R)) return st;
    int8_t host[INFL_TABLE_MAX];
    if (int st = fill_table(e, who, c, R, table, n_table, host)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // a run in flight reads the table to its end
    if (!g.counts) {
        DevAlloc A{e};
        A(&g.table, (size_t)INFL_TABLE_MAX); A(&g.counts, (size_t)e->B * 2);     // (counts last: the ready flag)
        if (A.st) return A.st;
    }
    HIPCHK(e, hipMemcpy(g.table, host, (size_t)R * R + 1, hipMemcpyHostToDevice));
    g.cfg = c; g.R = R;
    g.on = true;
    return PP_OK;
}

int pp_get_inflation_config(pp_handle e, int32_t source, int32_t* on, pp_inflation_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_inflation_config", source)) return st;
    *on = e->infl[source].on ? 1 : 0;
    if (cfg_out) *cfg_out = e->infl[source].cfg;
    return PP_OK;
}

int pp_inflate_async(pp_handle e, int32_t source) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_inflate_async";
    if (int st = check_source(e, who, source)) return st;
    pp_engine::Inflation& g = e->infl[source];
    const char* name = source_name(source);
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the inflation of the %s source is not configured (pp_set_inflation first)", who, name);
    // the source: on, of the table's resolution, and run
    const bool cm = source == PP_INFLATE_COSTMAP;
    const pp_engine::Costmap& c = e->cmap;
    const pp_engine::Occupancy& o = e->occ;
    if (!(cm ? c.on : o.on))
        return fail(e, PP_ERR_STATE, "%s: the %s stage is not configured (%s first)", who, name, cm ? "pp_set_costmap" : "pp_set_occupancy");
    const int batch = cm ? (c.grid ? c.batch : 0) : (o.marks ? o.batch : 0);
    // the resolution of the grids that lie there: of the costmap's last run, whatever pp_set_costmap has given since (its
    // buffers and that run stay while the shape stands); an occupancy configuration of another resolution forgets the maps
    const double res = cm ? (batch > 0 ? c.run_res : c.cfg.resolution) : o.cfg.resolution;
    if (res != g.cfg.resolution)
        return fail(e, PP_ERR_STATE, "%s: the %s stage has resolution = %g, the inflation table was built for %g (pp_set_inflation again)",
                    who, name, res, g.cfg.resolution);
    if (int st = check_last_run(e, who, batch, batch, false, cm ? "no costmap stage has run (pp_costmap_async first)"
                                : "no update has run (pp_occupancy_update_async first)", "run", "grids")) return st;
    const int W = cm ? c.run_w : o.cfg.width, H = cm ? c.run_h : o.cfg.height, pitch = cm ? c.run_pitch : o.pitch;
    const size_t cells = (size_t)pitch * H;
    (void)hipSetDevice(e->device);
    if (cells != g.cells) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a run in flight writes the old buffers to its end
        g.mem.release();
        g.cells = 0; g.batch = 0;
        StageMem& M = g.mem;
        M(&g.out, (size_t)e->B * cells); M(&g.dist2, (size_t)e->B * cells);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d grids x %zu cells (rows of %d) need %zu bytes of device memory and the device cannot "
                        "hold them (%s)", who, e->B, cells, pitch, (size_t)e->B * cells * 3, hipGetErrorString(st));
        }
        g.cells = cells;
    }
    InflParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = W; p.height = H; p.R = g.R;
    p.lethal = g.cfg.lethal_threshold; p.unknown_min = g.cfg.unknown_min_cost;
    p.in_pitch = p.out_pitch = pitch;
    p.in_stride = p.out_stride = cells;
    if (cm) {
        p.in[0] = p.in[1] = c.grid;
    } else {
        p.in[0] = o.grid[0]; p.in[1] = o.grid[1];
        p.occ_call = o.d_call;                           // the last update's records: which copy it wrote, per stream
    }
    p.table = g.table; p.out = g.out; p.dist2 = g.dist2; p.counts = g.counts;
    prof_reset(e);
    HIPCHK(e, hipMemsetAsync(g.counts, 0, (size_t)batch * 2 * sizeof(int), e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_inflate(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    g.batch = batch; g.run_pitch = pitch; g.run_w = W; g.run_h = H; g.run_R = g.R;
    ++g.run_id;                                          // (the same buffers, other grids: what navfn recorded no longer holds)
    g.known.assign((size_t)batch, 1);
    if (!cm)
        for (int b = 0; b < batch; ++b) g.known[(size_t)b] = o.has[(size_t)b];
    return PP_OK;
}

int pp_get_inflated(pp_handle e, int32_t source, int8_t* grid, uint16_t* dist2, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_inflated";
    if (int st = check_source(e, who, source)) return st;
    if (!grid) return fail(e, PP_ERR_ARG, "%s: grid is NULL", who);
    pp_engine::Inflation& g = e->infl[source];
    if (int st = check_last_run(e, who, g.out ? g.batch : 0, batch, true, "no inflation has run on this source (pp_inflate_async first)",
                                "run", "grids")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    // rows of `pitch` cells on the device, of `width` on the host; the grids lie row behind row in both
    const size_t W = (size_t)g.run_w, H = (size_t)g.run_h, rows = (size_t)batch * H;
    HIPCHK(e, hipMemcpy2D(grid, W, g.out, (size_t)g.run_pitch, W, rows, hipMemcpyDeviceToHost));
    if (dist2) HIPCHK(e, hipMemcpy2D(dist2, W * 2, g.dist2, (size_t)g.run_pitch * 2, W * 2, rows, hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) {
        if (g.known[(size_t)b]) continue;                  // reset before the run: all unknown, nothing in reach
        memset(grid + (size_t)b * W * H, 0xff, W * H);
        if (dist2) std::fill_n(dist2 + (size_t)b * W * H, W * H, (uint16_t)(g.run_R * g.run_R + 1));
    }
    return PP_OK;
}

int pp_inflation_info(pp_handle e, int32_t source, int32_t* lethal, int32_t* raised, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_inflation_info";
    if (int st = check_source(e, who, source)) return st;
    pp_engine::Inflation& g = e->infl[source];
    if (int st = check_last_run(e, who, g.out ? g.batch : 0, batch, true, "no inflation has run on this source (pp_inflate_async first)",
                                "run", "grids")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<int> counts((size_t)batch * 2, 0);
    HIPCHK(e, hipMemcpy(counts.data(), g.counts, counts.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int b = 0; b < batch; ++b) {
        const bool known = g.known[(size_t)b] != 0;
        if (lethal) lethal[b] = known ? counts[(size_t)b * 2] : 0;
        if (raised) raised[b] = known ? counts[(size_t)b * 2 + 1] : 0;
    }
    return PP_OK;
}

int pp_inflate_grids(int device, const int8_t* grids, int32_t batch, int32_t height, int32_t width,
                     const pp_inflation_config* cfg, const int8_t* table, int32_t n_table, int8_t* out, uint16_t* dist2,
                     int32_t* counts) {
    const char* who = "pp_inflate_grids";
    if (!grids || !cfg || !out) return fail(nullptr, PP_ERR_ARG, "%s: grids, cfg or out is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (int st = check_cfg_window(nullptr, who, width, height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    int R = 0;
    if (int st = check_config(nullptr, who, *cfg, &R)) return st;
    int8_t host[INFL_TABLE_MAX];
    if (int st = fill_table(nullptr, who, *cfg, R, table, n_table, host)) return st;
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    const size_t cells = (size_t)width * height, n = (size_t)batch * cells;
    DevBuf d_in, d_out, d_dist2, d_table, d_counts;
    DEVCHK(d_in.alloc(n));
    DEVCHK(d_out.alloc(n));
    if (dist2) DEVCHK(d_dist2.alloc(n * sizeof(uint16_t)));
    DEVCHK(d_table.alloc((size_t)INFL_TABLE_MAX));
    DEVCHK(d_counts.alloc((size_t)batch * 2 * sizeof(int)));
    DEVCHK(hipMemcpy(d_in.p, grids, n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_table.p, host, (size_t)R * R + 1, hipMemcpyHostToDevice));
    DEVCHK(hipMemset(d_counts.p, 0, (size_t)batch * 2 * sizeof(int)));
    InflParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = width; p.height = height; p.R = R;
    p.lethal = cfg->lethal_threshold; p.unknown_min = cfg->unknown_min_cost;
    p.in_pitch = p.out_pitch = width;
    p.in_stride = p.out_stride = cells;
    p.in[0] = p.in[1] = (const int8_t*)d_in.p;
    p.table = (const int8_t*)d_table.p;
    p.out = (int8_t*)d_out.p; p.dist2 = (uint16_t*)d_dist2.p; p.counts = (int*)d_counts.p;
    launch_inflate(p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipMemcpy(out, d_out.p, n, hipMemcpyDeviceToHost));
    if (dist2) DEVCHK(hipMemcpy(dist2, d_dist2.p, n * sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (counts) DEVCHK(hipMemcpy(counts, d_counts.p, (size_t)batch * 2 * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
