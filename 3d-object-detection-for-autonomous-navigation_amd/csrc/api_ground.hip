// C-ABI, the ground stage (pp_set_ground, pp_get_ground_config, pp_ground_async, pp_ground_used, pp_ground_shape,
// pp_get_ground, pp_ground_points): the resident rows -> one plane per frame and two bits per row, GROUND and OBSTACLE, on the device
// (kernels: ground.hip; the rule: ground.py).  A stage of its own, queued on the handle's stream as plain launches.  The
// occupancy update, the scan match and the costmap's point layer read the words through ground_for (pp_engine.h) and know
// nothing else of this stage.  The triples of a call travel from the host and are consumed on the main stream: a call ring
// of the stage's own (pp_ring.h).  pp_ground_points needs no handle: host buffers in, host buffers out, device memory for
// the call's duration.
#include "pp_engine.h"

static_assert(sizeof(pp_ground_config) == 96, "pp_ground_config: 9 doubles, a uint64, 4 int32 (the Python binding mirrors it)");
static_assert(PP_GROUND_MAX_HYP >= 512, "the stage benches use 512 hypotheses");

namespace {

constexpr int GR_ALL = PP_GROUND_OCCUPANCY | PP_GROUND_SCAN_MATCH | PP_GROUND_COSTMAP;
constexpr double GR_REFINE_LIMIT = 64.0;         // ground.REFINE_LIMIT

// Everything pp_set_ground and pp_ground_points refuse of a configuration, by field name (max_rows: the rows of a frame at most)
int check_config(pp_engine* e, const char* who, const pp_ground_config& c, long long max_rows, bool consumers) {
    if (int st = check_cfg_doubles(e, who, {{"max_range", c.max_range, true}, {"cand_z_max", c.cand_z_max, true}, {"max_slope", c.max_slope, true},
                                            {"h_min", c.h_min, true}, {"h_max", c.h_max, true}, {"inlier_dist", c.inlier_dist, true},
                                            {"ground_dist", c.ground_dist, true}, {"overhead_max", c.overhead_max, true},
                                            {"fallback_c", c.fallback_c, true}})) return st;
    if (!(c.max_range > 0.0)) return fail(e, PP_ERR_ARG, "%s: max_range = %g must be > 0", who, c.max_range);
    if (!(c.max_slope >= 0.0)) return fail(e, PP_ERR_ARG, "%s: max_slope = %g must be >= 0", who, c.max_slope);
    if (!(c.inlier_dist >= 0.0)) return fail(e, PP_ERR_ARG, "%s: inlier_dist = %g must be >= 0", who, c.inlier_dist);
    if (!(c.ground_dist >= 0.0)) return fail(e, PP_ERR_ARG, "%s: ground_dist = %g must be >= 0", who, c.ground_dist);
    if (!(c.h_min <= c.h_max)) return fail(e, PP_ERR_ARG, "%s: h_min = %g above h_max = %g", who, c.h_min, c.h_max);
    if (!(c.overhead_max >= c.ground_dist)) return fail(e, PP_ERR_ARG, "%s: overhead_max = %g under ground_dist = %g", who, c.overhead_max, c.ground_dist);
    if (c.hypotheses < 1 || c.hypotheses > PP_GROUND_MAX_HYP)
        return fail(e, PP_ERR_ARG, "%s: hypotheses = %d outside [1, PP_GROUND_MAX_HYP = %d]", who, c.hypotheses, PP_GROUND_MAX_HYP);
    if (c.min_inliers < 1) return fail(e, PP_ERR_ARG, "%s: min_inliers = %d must be >= 1", who, c.min_inliers);
    if (c.refine != 0 && c.refine != 1) return fail(e, PP_ERR_ARG, "%s: refine = %d (0 or 1)", who, c.refine);
    if (consumers && (c.consumers < 0 || (c.consumers & ~GR_ALL)))
        return fail(e, PP_ERR_ARG, "%s: consumers = %d holds bits outside PP_GROUND_OCCUPANCY | PP_GROUND_SCAN_MATCH | PP_GROUND_COSTMAP = %d",
                    who, c.consumers, GR_ALL);
    if (c.refine) {                                       // ground.check_refine: the refit's sums stay exact
        if (!(c.max_range <= GR_REFINE_LIMIT)) return fail(e, PP_ERR_ARG, "%s: refine needs max_range <= 64, got %g", who, c.max_range);
        if (!(std::fabs(c.cand_z_max) <= GR_REFINE_LIMIT)) return fail(e, PP_ERR_ARG, "%s: refine needs |cand_z_max| <= 64, got %g", who, c.cand_z_max);
        const double reach = c.max_slope * c.max_range + std::max(std::fabs(c.h_min), std::fabs(c.h_max)) + c.inlier_dist;
        if (!(reach <= GR_REFINE_LIMIT - 1.0))
            return fail(e, PP_ERR_ARG, "%s: refine needs max_slope * max_range + max(|h_min|, |h_max|) + inlier_dist <= 63, got %g", who, reach);
        if (!(max_rows < (1ll << 25))) return fail(e, PP_ERR_ARG, "%s: refine needs rows per frame * 2^28 < 2^53, got %lld rows", who, max_rows);
    }
    return PP_OK;
}

int make_buffers(pp_engine* e) {
    pp_engine::Ground& g = e->ground;
    const size_t B = (size_t)e->B, tri = (size_t)PP_GROUND_MAX_HYP * 3;
    HIPCHK(e, g.h_tri.alloc(g.ring, B * tri));
    if (g.d_tri) return PP_OK;
    const int stride = std::max(4 * ((e->NMAX + 255) / 256), 1);
    DevAlloc A{e};
    A(&g.hyp, B * PP_GROUND_MAX_HYP); A(&g.chyp, B * PP_GROUND_MAX_HYP); A(&g.counts, B * PP_GROUND_MAX_HYP); A(&g.sums, B * PP_GROUND_SUMS); A(&g.plane, B * 3);
    A(&g.info, B * PP_GROUND_INFO); A(&g.gnd, B * (size_t)stride); A(&g.obs, B * (size_t)stride);
    A(&g.d_tri, B * tri);                                // (d_tri last: the ready flag)
    if (A.st) return A.st;
    g.stride = stride;
    return PP_OK;
}

// the device buffers of a run -> the caller's (each may be NULL); the stream is idle
#define GRCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(e, PP_ERR_HIP, "%s: %s", who, hipGetErrorString(e_)); } while (0)
int fetch(pp_engine* e, const char* who, const GrParams& p, int run_words, double* planes, int32_t* info, uint64_t* gw, uint64_t* ow,
          int words_per_frame, int64_t* sums, int32_t* counts) {
    const size_t B = (size_t)p.batch;
    if (planes) GRCHK(hipMemcpy(planes, p.plane, B * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (info) GRCHK(hipMemcpy(info, p.info, B * PP_GROUND_INFO * sizeof(int), hipMemcpyDeviceToHost));
    if (sums) GRCHK(hipMemcpy(sums, p.sums, B * PP_GROUND_SUMS * sizeof(long long), hipMemcpyDeviceToHost));
    if (counts) GRCHK(hipMemcpy(counts, p.counts, B * (size_t)p.K * sizeof(int), hipMemcpyDeviceToHost));
    for (int which = 0; which < 2; ++which) {
        uint64_t* dst = which ? ow : gw;
        if (!dst) continue;
        memset(dst, 0, B * (size_t)words_per_frame * sizeof(uint64_t));
        if (run_words > 0)
            GRCHK(hipMemcpy2D(dst, (size_t)words_per_frame * 8, which ? p.obs : p.gnd, (size_t)p.stride * 8, (size_t)run_words * 8, B,
                               hipMemcpyDeviceToHost));
    }
    return PP_OK;
}
#undef GRCHK

}  // namespace

void ground_release(pp_engine* e) {
    e->ground.ring.release();
    e->ground = pp_engine::Ground();
}

extern "C" {

int pp_set_ground(pp_handle e, const pp_ground_config* cfg) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_ground: a training step is in flight");
    pp_engine::Ground& g = e->ground;
    if (!cfg) { g.on = false; return PP_OK; }
    pp_ground_config c = *cfg;
    if (int st = check_config(e, "pp_set_ground", c, e->NMAX, true)) return st;
    (void)hipSetDevice(e->device);
    if (int st = make_buffers(e)) return st;
    if (memcmp(&c, &g.cfg, sizeof(c)) != 0) g.batch = 0;   // the last classes are another rule's
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_ground_config(pp_handle e, int32_t* on, pp_ground_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->ground.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->ground.cfg;
    return PP_OK;
}

int pp_ground_async(pp_handle e, const uint32_t* triples, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_ground_async";
    pp_engine::Ground& g = e->ground;
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the ground stage is not configured (pp_set_ground first)", who);
    if (int st = check_resident_call(e, who, batch, "upload or ingest frames first")) return st;
    if (!triples) return fail(e, PP_ERR_ARG, "%s: triples is NULL", who);
    const pp_ground_config& c = g.cfg;
    (void)hipSetDevice(e->device);
    const size_t count = (size_t)batch * c.hypotheses * 3;
    int slot = -1;
    HIPCHK(e, g.ring.take(&slot));                       // behind the last check that can refuse
    memcpy(g.h_tri.at(slot), triples, count * sizeof(unsigned));
    GrParams p;
    memset(&p, 0, sizeof(p));
    if (int st = resident_points(e, batch, e->stream, false, &p.points)) return st;
    p.cfg = c; p.batch = batch; p.F = e->F; p.max_n = std::min(e->cur_max_n, e->NMAX); p.K = c.hypotheses;
    p.offsets = e->d_offsets;
    p.triples = g.d_tri; p.hyp = g.hyp; p.chyp = g.chyp; p.counts = g.counts; p.sums = g.sums; p.plane = g.plane; p.info = g.info;
    p.gnd = g.gnd; p.obs = g.obs; p.stride = g.stride;
    prof_reset(e);
    HIPCHK(e, g.h_tri.send(slot, g.d_tri, count, e->stream));
    HIPCHK(e, g.ring.sent(slot, e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_ground(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    // the next upload but one writes the buffer read here: its writer waits for this event as for a pass
    HIPCHK(e, hipEventRecord(e->ev_read[e->in_buf], e->stream));
    g.batch = batch; g.run_words = (p.max_n + 63) / 64; g.run_k = p.K; g.gen = e->resident_gen;
    return PP_OK;
}

int pp_ground_used(pp_handle e, int32_t* readers) {
    if (!e || !readers) return PP_ERR_ARG;
    *readers = e->ground.used;
    return PP_OK;
}

int pp_ground_shape(pp_handle e, int32_t* batch, int32_t* words_per_frame) {
    if (!e || !batch || !words_per_frame) return PP_ERR_ARG;
    *batch = e->ground.batch;
    *words_per_frame = e->ground.batch ? e->ground.run_words : 0;
    return PP_OK;
}

int pp_get_ground(pp_handle e, double* planes, int32_t* info, uint64_t* ground_words, uint64_t* obstacle_words, int64_t* sums,
                  int32_t* counts, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_ground";
    pp_engine::Ground& g = e->ground;
    if (int st = check_last_run(e, who, g.batch, batch, true, "no ground plane has been computed (pp_ground_async first)", "run", "frames")) return st;
    if (g.gen != e->resident_gen)
        return fail(e, PP_ERR_STATE, "%s: the frames the last classes belong to are gone (pp_ground_async again)", who);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    GrParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.K = g.run_k; p.hyp = g.hyp; p.counts = g.counts; p.sums = g.sums; p.plane = g.plane; p.info = g.info;
    p.gnd = g.gnd; p.obs = g.obs; p.stride = g.stride;
    return fetch(e, who, p, g.run_words, planes, info, ground_words, obstacle_words, g.run_words, sums, counts);
}

int pp_ground_points(int device, const float* points, const int32_t* offsets, int32_t num_features, int32_t batch,
                     const pp_ground_config* cfg, const uint32_t* triples, double* planes, int32_t* info, uint64_t* ground_words,
                     uint64_t* obstacle_words, int32_t words_per_frame, int64_t* sums, int32_t* counts) {
    const char* who = "pp_ground_points";
    if (!offsets || !cfg || !triples) return fail(nullptr, PP_ERR_ARG, "%s: offsets, cfg or triples is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (num_features < 3) return fail(nullptr, PP_ERR_ARG, "%s: num_features = %d must be >= 3", who, num_features);
    if (offsets[0] != 0) return fail(nullptr, PP_ERR_ARG, "%s: offsets[0] must be 0", who);
    int max_n = 0;
    for (int b = 0; b < batch; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail(nullptr, PP_ERR_ARG, "%s: offsets not monotone at frame %d", who, b);
        max_n = std::max(max_n, offsets[b + 1] - offsets[b]);
    }
    if (int st = check_config(nullptr, who, *cfg, max_n, false)) return st;
    const size_t total = (size_t)offsets[batch];
    if (total && !points) return fail(nullptr, PP_ERR_ARG, "%s: points is NULL", who);
    const int run_words = (max_n + 63) / 64;
    if ((ground_words || obstacle_words) && words_per_frame < run_words)
        return fail(nullptr, PP_ERR_ARG, "%s: words_per_frame = %d, the longest frame has %d rows: %d words", who, words_per_frame, max_n, run_words);
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    GrParams p;
    memset(&p, 0, sizeof(p));
    p.cfg = *cfg; p.batch = batch; p.F = num_features; p.max_n = max_n; p.K = cfg->hypotheses;
    p.stride = std::max(4 * ((max_n + 255) / 256), 1);
    const size_t B = (size_t)batch, K = (size_t)p.K;
    DevBuf d_pts, d_off, d_tri, d_hyp, d_chyp, d_counts, d_sums, d_plane, d_info, d_gnd, d_obs;
    DEVCHK(d_pts.alloc(total * num_features * sizeof(float)));
    DEVCHK(d_off.alloc((B + 1) * sizeof(int)));
    DEVCHK(d_tri.alloc(B * K * 3 * sizeof(unsigned)));
    DEVCHK(d_hyp.alloc(B * K * sizeof(GrHyp)));
    DEVCHK(d_chyp.alloc(B * K * sizeof(GrHyp)));
    DEVCHK(d_counts.alloc(B * K * sizeof(int)));
    DEVCHK(d_sums.alloc(B * PP_GROUND_SUMS * sizeof(long long)));
    DEVCHK(d_plane.alloc(B * 3 * sizeof(double)));
    DEVCHK(d_info.alloc(B * PP_GROUND_INFO * sizeof(int)));
    DEVCHK(d_gnd.alloc(B * p.stride * sizeof(unsigned long long)));
    DEVCHK(d_obs.alloc(B * p.stride * sizeof(unsigned long long)));
    if (total) DEVCHK(hipMemcpy(d_pts.p, points, total * num_features * sizeof(float), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_off.p, offsets, (B + 1) * sizeof(int), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_tri.p, triples, B * K * 3 * sizeof(unsigned), hipMemcpyHostToDevice));
    p.points = (const float*)d_pts.p; p.offsets = (const int*)d_off.p; p.triples = (const unsigned*)d_tri.p;
    p.hyp = (GrHyp*)d_hyp.p; p.chyp = (GrHyp*)d_chyp.p; p.counts = (int*)d_counts.p; p.sums = (long long*)d_sums.p; p.plane = (double*)d_plane.p;
    p.info = (int*)d_info.p; p.gnd = (unsigned long long*)d_gnd.p; p.obs = (unsigned long long*)d_obs.p;
    launch_ground(p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipStreamSynchronize(nullptr));
    return fetch(nullptr, who, p, run_words, planes, info, ground_words, obstacle_words, words_per_frame, sums, counts);
}

}  // extern "C"
