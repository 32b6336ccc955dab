// C-ABI, scan match (pp_set_scan_match, pp_get_scan_match_config, pp_scan_match_async, pp_get_scan_match,
// pp_scan_match_grids): the resident points of frame b under stream b's prior sensor-to-fixed pose, matched against the
// log-odds window the occupancy stage holds for the stream -> eight words and the candidates' scores per stream, on the
// device (kernels: scan_match.hip; the rule: scan_match.py).  The stage reads the occupancy state in place and never
// writes it; the sensor's sub-cell position in the window is host arithmetic (float64), as the window's origin is.  The
// priors travel from the host on every call and are consumed on the main stream: a call ring of the stage's own
// (pp_ring.h).  Its window-shaped buffers follow the occupancy configuration: every call compares the shape they were
// made for with the one in force and re-makes them where pp_set_occupancy changed it, so api_occupancy.hip knows nothing
// of this stage.  pp_scan_match_grids needs no handle: host buffers in, host buffers out, device memory for the call's
// duration.
#include "pp_engine.h"

static_assert(sizeof(pp_scan_match_config) == 32, "pp_scan_match_config: 8 int32 (the Python binding mirrors it)");
static_assert(sizeof(ScanCall) == 64, "ScanCall: 6 doubles, 4 int32, packed by the host per stream");
static_assert(PP_SCAN_RESULT == 8 && PP_SCAN_MAX_CANDIDATES == 65536, "the result words; a key's low 16 bits are the candidate");
static_assert(PP_LOCAL_SUB == 1024 && PP_LOCAL_HEADINGS == 4096, "sub-cells per cell, ticks per revolution");

namespace {

constexpr double SCAN_CELL_LIMIT = 1073741824.0;   // |t| / resolution from which a prior is refused: 2^30, as the occupancy update

// Everything pp_set_scan_match and pp_scan_match_grids refuse of a configuration, by field name.
int check_config(pp_engine* e, const char* who, const pp_scan_match_config& c) {
    const struct { const char* name; int v, lo, hi; } f[] = {
        {"nx", c.nx, 0, 127}, {"ny", c.ny, 0, 127}, {"nt", c.nt, 0, 127}, {"xy_step", c.xy_step, 1, 4096},
        {"theta_step", c.theta_step, 1, 512}, {"min_cells", c.min_cells, 0, PP_OCC_MAX_CELLS}, {"min_mean", c.min_mean, -100000, 100000},
        {"reserved", c.reserved, 0, 0}};
    for (const auto& x : f)
        if (x.v < x.lo || x.v > x.hi) return fail(e, PP_ERR_ARG, "%s: %s = %d outside [%d, %d]", who, x.name, x.v, x.lo, x.hi);
    const long long n = (long long)(2 * c.nx + 1) * (2 * c.ny + 1) * (2 * c.nt + 1);
    if (n > PP_SCAN_MAX_CANDIDATES)
        return fail(e, PP_ERR_ARG, "%s: (2 nx + 1)(2 ny + 1)(2 nt + 1) = %lld candidates, at most PP_SCAN_MAX_CANDIDATES = %d", who, n,
                    PP_SCAN_MAX_CANDIDATES);
    return PP_OK;
}

int candidates(const pp_scan_match_config& c) { return (2 * c.nx + 1) * (2 * c.ny + 1) * (2 * c.nt + 1); }
int tiles_of(const pp_scan_match_config& c) { return ((2 * c.nx + 1) * (2 * c.ny + 1) + SCAN_TILE - 1) / SCAN_TILE; }

// what a prior's translation is refused for, as pp_occupancy_update_async refuses it
int check_translation(pp_engine* e, const char* who, int b, const double* P, double resolution) {
    if (!(std::fabs(P[3] / resolution) < SCAN_CELL_LIMIT) || !(std::fabs(P[7] / resolution) < SCAN_CELL_LIMIT))
        return fail(e, PP_ERR_ARG, "%s: poses: the translation of stream %d (%g, %g) is 2^30 cells of %g m or more from the origin",
                    who, b, P[3], P[7], resolution);
    return PP_OK;
}

// one stream's record: the rotation rows, and the sensor in sub-cells of the window whose origin cell is (ox, oy)
void fill_call(ScanCall& k, const double* P, const pp_occupancy_config& c, bool has, int ox, int oy, int src) {
    memset(&k, 0, sizeof(k));
    for (int j = 0; j < 3; ++j) { k.r0[j] = P[j]; k.r1[j] = P[4 + j]; }
    if (!has) { k.flags = PP_SCAN_NO_MAP; return; }
    k.src = src;
    const double sx = std::floor((P[3] / c.resolution - (double)ox) * (double)PP_LOCAL_SUB);
    const double sy = std::floor((P[7] / c.resolution - (double)oy) * (double)PP_LOCAL_SUB);
    // the sensor's cell (sx >> 10, sy >> 10) lies in the window iff 0 <= sx < width * 1024; held as doubles until then
    if (!(sx >= 0.0 && sx < (double)c.width * PP_LOCAL_SUB && sy >= 0.0 && sy < (double)c.height * PP_LOCAL_SUB)) {
        k.flags = PP_SCAN_OUTSIDE;
        return;
    }
    k.sx = (int)sx; k.sy = (int)sy;
}

void fill_shape(ScanParams& p, const pp_occupancy_config& occ, const pp_scan_match_config& cfg) {
    p.occ = occ; p.cfg = cfg;
    p.n_trans = (2 * cfg.nx + 1) * (2 * cfg.ny + 1);
    p.tiles = tiles_of(cfg);
    p.mark_words = (occ.width * occ.height + 31) / 32;
}

}  // namespace

void scan_match_release(pp_engine* e) {
    pp_engine::ScanMatch& g = e->scan;
    g.mem_cfg.release();
    g.mem_win.release();
    g.ring.release();
    g = pp_engine::ScanMatch();
}

extern "C" {

int pp_set_scan_match(pp_handle e, const pp_scan_match_config* cfg, const int32_t* trig, int32_t n_trig) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_scan_match";
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::ScanMatch& g = e->scan;
    if (!cfg) { g.on = false; return PP_OK; }
    if (!e->occ.on) return fail(e, PP_ERR_STATE, "%s: the occupancy stage is not configured (pp_set_occupancy first)", who);
    const pp_scan_match_config c = *cfg;
    if (int st = check_config(e, who, c)) return st;
    std::vector<unsigned> packed;
    if (int st = pack_trig(e, who, trig, n_trig, packed)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // a match in flight reads the table and writes the buffers to its end
    HIPCHK(e, g.h_call.alloc(g.ring, (size_t)e->B));
    if (!g.d_call) {
        DevAlloc A{e};
        A(&g.trig, (size_t)PP_LOCAL_HEADINGS); A(&g.words, (size_t)PP_SCAN_RESULT * e->B);
        A(&g.d_call, (size_t)e->B);                      // (d_call last: the ready flag)
        if (A.st) return A.st;
    }
    const int cands = candidates(c), parts = (2 * c.nt + 1) * tiles_of(c);
    if (cands > g.cand_cap || parts > g.part_cap) {
        g.on = false;
        g.mem_cfg.release();
        g.cand_cap = 0; g.part_cap = 0; g.batch = 0;
        StageMem& M = g.mem_cfg;
        M(&g.scores, (size_t)e->B * cands); M(&g.partial, (size_t)e->B * parts);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d streams x %d candidates need %zu bytes of device memory and the device cannot hold them (%s)",
                        who, e->B, cands, (size_t)e->B * ((size_t)cands * 4 + (size_t)parts * 8), hipGetErrorString(st));
        }
        g.cand_cap = cands; g.part_cap = parts;
    }
    HIPCHK(e, hipMemcpy(g.trig, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_scan_match_config(pp_handle e, int32_t* on, pp_scan_match_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->scan.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->scan.cfg;
    return PP_OK;
}

int pp_scan_match_async(pp_handle e, const double* poses, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_scan_match_async";
    pp_engine::ScanMatch& g = e->scan;
    const pp_engine::Occupancy& o = e->occ;
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the scan match is not configured (pp_set_scan_match first)", who);
    if (!o.on) return fail(e, PP_ERR_STATE, "%s: the occupancy stage is not configured (pp_set_occupancy first)", who);
    if (!poses) return fail(e, PP_ERR_ARG, "%s: poses is NULL", who);
    if (int st = check_resident_call(e, who, batch, "upload or ingest frames first")) return st;
    const pp_occupancy_config& c = o.cfg;
    if (int st = check_poses(e, who, poses, nullptr, batch, [&](int b, const double* P) { return check_translation(e, who, b, P, c.resolution); }))
        return st;
    const unsigned long long* mask = nullptr;
    int mask_stride = 0;
    if (int st = object_mask_for(e, who, PP_OBJMASK_SCAN_MATCH, batch, &mask, &mask_stride)) return st;
    const unsigned long long *cls_gnd = nullptr, *cls_obs = nullptr;
    int cls_stride = 0;
    if (int st = ground_for(e, who, PP_GROUND_SCAN_MATCH, batch, &cls_gnd, &cls_obs, &cls_stride)) return st;
    (void)hipSetDevice(e->device);
    // the buffers shaped by the occupancy window: re-made where pp_set_occupancy changed it since they were made
    const int list_cap = (int)std::min<long long>((long long)c.width * c.height, (long long)e->NMAX);
    if (c.width != g.win_w || c.height != g.win_h || list_cap != g.list_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a match in flight writes the old buffers to its end
        g.mem_win.release();
        g.win_w = 0; g.win_h = 0; g.list_cap = 0; g.mark_words = 0; g.batch = 0;
        const int mark_words = (c.width * c.height + 31) / 32;
        StageMem& M = g.mem_win;
        M(&g.clear, (size_t)e->B * (SCAN_INFO + (size_t)mark_words)); M(&g.list, (size_t)e->B * list_cap);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d streams x %d cells need %zu bytes of device memory and the device cannot hold them (%s)", who,
                        e->B, c.width * c.height, (size_t)e->B * ((SCAN_INFO + (size_t)mark_words) * 4 + (size_t)list_cap * 8),
                        hipGetErrorString(st));
        }
        g.win_w = c.width; g.win_h = c.height; g.list_cap = list_cap; g.mark_words = mark_words;
    }
    int slot;
    HIPCHK(e, g.ring.take(&slot));                       // behind the last check that can refuse
    ScanCall* call = g.h_call.at(slot);
    for (int b = 0; b < batch; ++b)
        fill_call(call[b], poses + (size_t)b * 12, c, o.has[(size_t)b] != 0, o.ox[(size_t)b], o.oy[(size_t)b], o.cur[(size_t)b]);
    ScanParams p;
    memset(&p, 0, sizeof(p));
    if (int st = resident_points(e, batch, e->stream, false, &p.points)) return st;
    fill_shape(p, c, g.cfg);
    p.batch = batch; p.F = e->F; p.pitch = o.pitch; p.map_stride = o.cells; p.max_n = std::min(e->cur_max_n, e->NMAX);
    p.list_cap = g.list_cap;
    p.offsets = e->d_offsets;
    p.call = g.d_call; p.trig = g.trig;
    p.logodds[0] = o.logodds[0]; p.logodds[1] = o.logodds[1];
    p.info = (int*)g.clear; p.marks = g.clear + (size_t)e->B * SCAN_INFO; p.list = g.list;
    p.scores = g.scores; p.partial = g.partial; p.words = g.words;
    p.mask = mask; p.mask_stride = mask_stride;
    p.gnd = cls_gnd; p.obs = cls_obs; p.cls_stride = cls_stride;
    prof_reset(e);
    HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
    HIPCHK(e, g.ring.sent(slot, e->stream));
    // the tallies of every stream and the marks of this call's streams, in one clear
    HIPCHK(e, hipMemsetAsync(g.clear, 0, ((size_t)e->B * SCAN_INFO + (size_t)batch * g.mark_words) * sizeof(unsigned), e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_scan_match(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload but one writes the buffer read here: its writer waits for this event as for a pass
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    g.batch = batch; g.run_cands = candidates(g.cfg);
    return PP_OK;
}

int pp_get_scan_match(pp_handle e, int32_t* words, int32_t* scores, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_scan_match";
    if (!words) return fail(e, PP_ERR_ARG, "%s: words is NULL", who);
    pp_engine::ScanMatch& g = e->scan;
    if (int st = check_last_run(e, who, g.batch, batch, true, "no match has run (pp_scan_match_async first)", "match", "streams")) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, hipMemcpy(words, g.words, (size_t)batch * PP_SCAN_RESULT * sizeof(int), hipMemcpyDeviceToHost));
    if (scores) HIPCHK(e, hipMemcpy(scores, g.scores, (size_t)batch * g.run_cands * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_scan_match_grids(int device, const int16_t* logodds, const uint8_t* known, int32_t batch, int32_t height, int32_t width,
                        const float* points, const int32_t* offsets, int32_t num_features, const double* poses,
                        const int32_t* origin_cells, const int32_t* has_map, const pp_occupancy_config* occ_cfg,
                        const pp_scan_match_config* cfg, const int32_t* trig, int32_t n_trig, int32_t* words, int32_t* scores) {
    const char* who = "pp_scan_match_grids";
    if (!logodds || !known || !occ_cfg || !cfg) return fail(nullptr, PP_ERR_ARG, "%s: logodds, known, occ_cfg or cfg is NULL", who);
    if (!offsets || !poses || !origin_cells || !has_map || !words)
        return fail(nullptr, PP_ERR_ARG, "%s: offsets, poses, origin_cells, has_map or words is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (int st = check_cfg_window(nullptr, who, width, height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    const pp_occupancy_config oc = *occ_cfg;
    if (oc.width != width || oc.height != height)
        return fail(nullptr, PP_ERR_ARG, "%s: occ_cfg is %d x %d, the grids are %d x %d", who, oc.width, oc.height, width, height);
    if (int st = check_cfg_doubles(nullptr, who, {{"resolution", oc.resolution, true}, {"z_min", oc.z_min, false}, {"z_max", oc.z_max, false},
                                                  {"max_range", oc.max_range, true}})) return st;
    if (!(oc.resolution > 0.0)) return fail(nullptr, PP_ERR_ARG, "%s: resolution = %g must be > 0", who, oc.resolution);
    if (!(oc.max_range > 0.0)) return fail(nullptr, PP_ERR_ARG, "%s: max_range = %g must be > 0", who, oc.max_range);
    if (num_features < 3) return fail(nullptr, PP_ERR_ARG, "%s: num_features = %d must be >= 3", who, num_features);
    if (int st = check_config(nullptr, who, *cfg)) return st;
    std::vector<unsigned> packed;
    if (int st = pack_trig(nullptr, who, trig, n_trig, packed)) return st;
    if (offsets[0] != 0) return fail(nullptr, PP_ERR_ARG, "%s: offsets[0] must be 0", who);
    int max_n = 0;
    for (int b = 0; b < batch; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail(nullptr, PP_ERR_ARG, "%s: offsets not monotone at frame %d", who, b);
        max_n = std::max(max_n, offsets[b + 1] - offsets[b]);
    }
    const size_t total = (size_t)offsets[batch];
    if (total && !points) return fail(nullptr, PP_ERR_ARG, "%s: points is NULL", who);
    if (int st = check_poses(nullptr, who, poses, nullptr, batch, [&](int b, const double* P) { return check_translation(nullptr, who, b, P, oc.resolution); }))
        return st;
    const size_t cells = (size_t)width * height, n = (size_t)batch * cells;
    // the device reads the log-odds alone: 0 where a cell is not known, as the occupancy stage keeps its state
    std::vector<int16_t> L(n);
    for (size_t i = 0; i < n; ++i) L[i] = known[i] ? logodds[i] : (int16_t)0;
    std::vector<ScanCall> calls((size_t)batch);
    for (int b = 0; b < batch; ++b)
        fill_call(calls[(size_t)b], poses + (size_t)b * 12, oc, has_map[b] != 0, origin_cells[2 * b], origin_cells[2 * b + 1], 0);
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    ScanParams p;
    memset(&p, 0, sizeof(p));
    fill_shape(p, oc, *cfg);
    const int cands = candidates(*cfg), parts = (2 * cfg->nt + 1) * p.tiles;
    p.list_cap = (int)std::min<size_t>(cells, (size_t)std::max(max_n, 1));
    const size_t clear_words = (size_t)batch * (SCAN_INFO + (size_t)p.mark_words);
    DevBuf d_L, d_pts, d_off, d_trig, d_call, d_clear, d_list, d_scores, d_partial, d_words;
    DEVCHK(d_L.alloc(n * sizeof(int16_t)));
    DEVCHK(d_pts.alloc(total * num_features * sizeof(float)));
    DEVCHK(d_off.alloc((size_t)(batch + 1) * sizeof(int)));
    DEVCHK(d_trig.alloc(packed.size() * sizeof(unsigned)));
    DEVCHK(d_call.alloc((size_t)batch * sizeof(ScanCall)));
    DEVCHK(d_clear.alloc(clear_words * sizeof(unsigned)));
    DEVCHK(d_list.alloc((size_t)batch * p.list_cap * sizeof(int2)));
    DEVCHK(d_scores.alloc((size_t)batch * cands * sizeof(int)));
    DEVCHK(d_partial.alloc((size_t)batch * parts * sizeof(unsigned long long)));
    DEVCHK(d_words.alloc((size_t)batch * PP_SCAN_RESULT * sizeof(int)));
    DEVCHK(hipMemcpy(d_L.p, L.data(), n * sizeof(int16_t), hipMemcpyHostToDevice));
    if (total) DEVCHK(hipMemcpy(d_pts.p, points, total * num_features * sizeof(float), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_off.p, offsets, (size_t)(batch + 1) * sizeof(int), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_trig.p, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_call.p, calls.data(), (size_t)batch * sizeof(ScanCall), hipMemcpyHostToDevice));
    DEVCHK(hipMemsetAsync(d_clear.p, 0, clear_words * sizeof(unsigned), nullptr));
    p.batch = batch; p.F = num_features; p.pitch = width; p.map_stride = cells; p.max_n = max_n;
    p.points = (const float*)d_pts.p; p.offsets = (const int*)d_off.p;
    p.call = (const ScanCall*)d_call.p; p.trig = (const unsigned*)d_trig.p;
    p.logodds[0] = p.logodds[1] = (const int16_t*)d_L.p;
    p.info = (int*)d_clear.p; p.marks = (unsigned*)d_clear.p + (size_t)batch * SCAN_INFO; p.list = (int2*)d_list.p;
    p.scores = (int*)d_scores.p; p.partial = (unsigned long long*)d_partial.p; p.words = (int*)d_words.p;
    launch_scan_match(p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipStreamSynchronize(nullptr));
    DEVCHK(hipMemcpy(words, p.words, (size_t)batch * PP_SCAN_RESULT * sizeof(int), hipMemcpyDeviceToHost));
    if (scores) DEVCHK(hipMemcpy(scores, p.scores, (size_t)batch * cands * sizeof(int), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
