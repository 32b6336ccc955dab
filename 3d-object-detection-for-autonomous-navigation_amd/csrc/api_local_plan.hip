// C-ABI, local planner (pp_set_local_plan, pp_get_local_plan_config, pp_local_plan_async, pp_get_local_plan,
// pp_local_plan_grids, and with movers pp_set_local_movers, pp_get_local_movers_config, pp_local_plan_movers_async,
// pp_get_local_movers, pp_local_plan_grids_movers): the inflated int8 grid a source's inflation leaves on the device and the cost-to-go field its
// navigation function leaves there -> one (v, w) command per grid from a window of rollouts (kernels: local_plan.hip; the
// rule: local_planner.py).  A stage behind either navigation function: rollout and finish as plain launches on the
// handle's stream.  pp_navfn_async returns before the relaxation has converged and only navfn's getters settle it, so
// pp_local_plan_async queues its two launches behind the rounds already queued, and pp_get_local_plan first runs navfn's
// settled_run on the source: if that queued any further round, rollout and finish are queued again.  A fetched command
// therefore always rests on the exact field, whatever queued_rounds says.  The poses and windows travel from the host on
// every call and are consumed on the main stream: a call ring of the stage's own (pp_ring.h).  pp_local_plan_grids needs
// no handle: host buffers in, host buffers out, device memory for the call's duration.
// MOVERS.  pp_local_plan_movers_async is pp_local_plan_async with one launch in front: k_local_movers turns the track slots
// of stream b into the integer table of grid b, where the tracker left them; the float64 frame records (origin, resolution,
// step seconds) ride the stage's call ring next to the poses and windows.  The rollout and the finish then run in their
// instantiations with movers.  The getter's re-queue runs those two again on the table that call built: the tracks may
// have moved on since, the table has not.
// FOOTPRINT.  pp_set_local_footprint (and pp_get_local_footprint_config, pp_get_local_footprint,
// pp_local_plan_grids_footprint) gives the source a table of probes, checked and packed here into a word of two int16
// halves per probe; while it is on, both async calls launch the rollout and the finish in their instantiations with a
// footprint, in front of which the chunks' slots of `partial` are set to all ones (the rollout lowers them) and n_footprint
// is cleared.  No third async entry: the footprint is a property of the robot, not of a call.
#include "pp_engine.h"

static_assert(sizeof(pp_local_plan_config) == 32, "pp_local_plan_config: 8 int32 (the Python binding mirrors it)");
static_assert(sizeof(LocalCall) == 32, "LocalCall: 8 int32, packed by the host per grid");
static_assert(sizeof(pp_local_mover_config) == 32, "pp_local_mover_config: 2 doubles, 4 int32 (the Python binding mirrors it)");
static_assert(sizeof(LocalFrame) == 32, "LocalFrame: 4 doubles, as pp_local_plan_movers_async's frame rows");
static_assert(PP_LOCAL_MAX_MOVERS == PP_TRACK_MAX && PP_TRACK_MAX == PP_WAVE, "k_local_movers: one lane per track slot, a mover per slot at most");
static_assert(PP_LOCAL_MOVER_INFO == 4 && LOC_M_NEAR == 3, "a grid's info words are the mover_info fields");
static_assert(sizeof(pp_local_footprint_config) == 16, "pp_local_footprint_config: 4 int32 (the Python binding mirrors it)");
static_assert(PP_LOCAL_FOOT_INFO == 4 && LOC_F_RESERVED == 3, "a grid's footprint words are the foot_info fields");
static_assert(PP_LOCAL_MAX_PROBE == 32767, "a probe's coordinates are int16 halves of one word");
static_assert(PP_LOCAL_SUB == 1024 && PP_LOCAL_HEADINGS == 4096, "sub-cells per cell, ticks per revolution");
static_assert(PP_LOCAL_RESULT == LOC_STATE, "a grid's result words are its state fields");
static_assert(PP_INFLATE_COSTMAP == 0 && PP_INFLATE_OCCUPANCY == 1, "pp_engine::local is indexed by source, as navfn");

namespace {

constexpr int LOC_MAX_SV = 1024, LOC_MAX_SW = 512;

const char* source_name(int source) { return source == PP_INFLATE_COSTMAP ? "costmap" : "occupancy"; }

// Everything pp_set_local_plan and pp_local_plan_grids refuse of a configuration, by field name.  The ranges are what
// keeps a score below 2^41 (local_plan.hip).
int check_config(pp_engine* e, const char* who, const pp_local_plan_config& c) {
    const struct { const char* name; int v, lo, hi; } f[] = {
        {"nv", c.nv, 1, PP_LOCAL_MAX_SAMPLES}, {"nw", c.nw, 1, PP_LOCAL_MAX_SAMPLES}, {"steps", c.steps, 1, PP_LOCAL_MAX_STEPS},
        {"lookahead", c.lookahead, 0, PP_LOCAL_MAX_LOOKAHEAD}, {"pot_weight", c.pot_weight, 0, 255},
        {"occ_weight", c.occ_weight, 0, 65535}, {"speed_weight", c.speed_weight, 0, 65535}, {"turn_weight", c.turn_weight, 0, 65535}};
    for (const auto& x : f)
        if (x.v < x.lo || x.v > x.hi) return fail(e, PP_ERR_ARG, "%s: %s = %d outside [%d, %d]", who, x.name, x.v, x.lo, x.hi);
    if ((long long)c.nv * c.nw > PP_LOCAL_MAX_SAMPLES)
        return fail(e, PP_ERR_ARG, "%s: nv * nw = %lld samples, at most PP_LOCAL_MAX_SAMPLES = %d", who, (long long)c.nv * c.nw, PP_LOCAL_MAX_SAMPLES);
    return PP_OK;
}

int check_source(pp_engine* e, const char* who, int source) {
    if (source != PP_INFLATE_COSTMAP && source != PP_INFLATE_OCCUPANCY)
        return fail(e, PP_ERR_ARG, "%s: source = %d (0 PP_INFLATE_COSTMAP, 1 PP_INFLATE_OCCUPANCY)", who, source);
    return PP_OK;
}

// the calls' records, and what is refused of a window: every sample within |sv| <= 1024 and |sw| <= 512 (the extremes of
// a window are its first and last sample).  `call` may be NULL: check only.
int fill_calls(pp_engine* e, const char* who, LocalCall* call, const pp_local_plan_config& cfg, const int32_t* poses,
               const int32_t* windows, const int32_t* goal_state, int batch) {
    for (int b = 0; b < batch; ++b) {
        const long long v0 = windows[4 * b], dv = windows[4 * b + 1], w0 = windows[4 * b + 2], dw = windows[4 * b + 3];
        const long long v1 = v0 + (cfg.nv - 1) * dv, w1 = w0 + (cfg.nw - 1) * dw;
        if (std::max(std::llabs(v0), std::llabs(v1)) > LOC_MAX_SV)
            return fail(e, PP_ERR_ARG, "%s: windows: grid %d: sv runs from %lld to %lld, outside [-%d, %d]", who, b, v0, v1, LOC_MAX_SV, LOC_MAX_SV);
        if (std::max(std::llabs(w0), std::llabs(w1)) > LOC_MAX_SW)
            return fail(e, PP_ERR_ARG, "%s: windows: grid %d: sw runs from %lld to %lld, outside [-%d, %d]", who, b, w0, w1, LOC_MAX_SW, LOC_MAX_SW);
        if (!call) continue;
        LocalCall& c = call[b];
        c.X = poses[3 * b]; c.Y = poses[3 * b + 1]; c.h = poses[3 * b + 2] & (PP_LOCAL_HEADINGS - 1);
        c.v0 = (int)v0; c.dv = (int)dv; c.w0 = (int)w0; c.dw = (int)dw;
        c.flags = goal_state && goal_state[b] != 0 ? LOC_NO_GOAL : 0;
    }
    return PP_OK;
}

void fill_config(LocalParams& p, const pp_local_plan_config& c) {
    p.nv = c.nv; p.nw = c.nw; p.steps = c.steps; p.lookahead = c.lookahead;
    p.pot_w = c.pot_weight; p.occ_w = c.occ_weight; p.speed_w = c.speed_weight; p.turn_w = c.turn_weight;
}

// what pp_set_local_movers and pp_local_plan_grids_movers refuse of horizon and mover_weight
int check_mover_ints(pp_engine* e, const char* who, int horizon, int mover_weight) {
    if (horizon < 0 || horizon > PP_LOCAL_MAX_STEPS) return fail(e, PP_ERR_ARG, "%s: horizon = %d outside [0, %d]", who, horizon, PP_LOCAL_MAX_STEPS);
    if (mover_weight < 0 || mover_weight > 65535) return fail(e, PP_ERR_ARG, "%s: mover_weight = %d outside [0, 65535]", who, mover_weight);
    return PP_OK;
}

// a host-given table: every mover of every grid within the ranges the kernels' integer widths rest on
int check_movers(const char* who, const int32_t* movers, const int32_t* n_movers, int batch) {
    for (int b = 0; b < batch; ++b) {
        if (n_movers[b] < 0 || n_movers[b] > PP_LOCAL_MAX_MOVERS)
            return fail(nullptr, PP_ERR_ARG, "%s: grid %d: n_movers = %d outside [0, %d]", who, b, n_movers[b], PP_LOCAL_MAX_MOVERS);
        for (int m = 0; m < n_movers[b]; ++m) {
            const int32_t* v = movers + ((size_t)b * PP_LOCAL_MAX_MOVERS + m) * 6;
            const long long pos = 1ll << 29;
            if (std::llabs((long long)v[0]) > pos || std::llabs((long long)v[1]) > pos)
                return fail(nullptr, PP_ERR_ARG, "%s: grid %d, mover %d: position (%d, %d) outside [-2^29, 2^29]", who, b, m, v[0], v[1]);
            if (std::llabs((long long)v[2]) > PP_LOCAL_MAX_MOVER_SPEED || std::llabs((long long)v[3]) > PP_LOCAL_MAX_MOVER_SPEED)
                return fail(nullptr, PP_ERR_ARG, "%s: grid %d, mover %d: movement (%d, %d) per step outside [-%d, %d]", who, b, m, v[2], v[3],
                            PP_LOCAL_MAX_MOVER_SPEED, PP_LOCAL_MAX_MOVER_SPEED);
            if (v[4] < 0 || v[4] > v[5] || v[5] > PP_LOCAL_MAX_MOVER_RADIUS)
                return fail(nullptr, PP_ERR_ARG, "%s: grid %d, mover %d: radii r_hard = %d, r_soft = %d, not 0 <= r_hard <= r_soft <= %d", who, b, m,
                            v[4], v[5], PP_LOCAL_MAX_MOVER_RADIUS);
        }
    }
    return PP_OK;
}

// what pp_set_local_footprint and pp_local_plan_grids_footprint refuse of a footprint, naming the field or the probe; the
// table packed into `out` (fx in the low half, fy in the high half of a word)
int check_footprint(pp_engine* e, const char* who, int foot_lethal, const int32_t* probes, int n, std::vector<unsigned>& out) {
    if (foot_lethal < 1 || foot_lethal > 100) return fail(e, PP_ERR_ARG, "%s: foot_lethal = %d outside [1, 100]", who, foot_lethal);
    if (n < 1 || n > PP_LOCAL_MAX_PROBES) return fail(e, PP_ERR_ARG, "%s: n_probes = %d outside [1, PP_LOCAL_MAX_PROBES = %d]", who, n, PP_LOCAL_MAX_PROBES);
    if (!probes) return fail(e, PP_ERR_ARG, "%s: probes is NULL", who);
    out.resize((size_t)n);
    for (int q = 0; q < n; ++q) {
        const int32_t fx = probes[2 * q], fy = probes[2 * q + 1];
        if (fx < -PP_LOCAL_MAX_PROBE || fx > PP_LOCAL_MAX_PROBE || fy < -PP_LOCAL_MAX_PROBE || fy > PP_LOCAL_MAX_PROBE)
            return fail(e, PP_ERR_ARG, "%s: probe %d: (%d, %d) outside [-%d, %d]", who, q, fx, fy, PP_LOCAL_MAX_PROBE, PP_LOCAL_MAX_PROBE);
        out[(size_t)q] = ((unsigned)fx & 0xFFFFu) | ((unsigned)fy << 16);
    }
    return PP_OK;
}

// the reason counts cleared, rollout, finish behind whatever `s` holds
int queue_run(pp_engine* e, const LocalParams& p, hipStream_t s) {
    HIPCHK(e, hipMemsetAsync(p.state + (size_t)LOC_N_OK * p.state_stride, 0, (size_t)4 * p.state_stride * sizeof(int), s));
    if (p.movers) HIPCHK(e, hipMemsetAsync(p.mover_info + (size_t)LOC_M_DYNAMIC * p.state_stride, 0, (size_t)p.state_stride * sizeof(int), s));
    if (p.probes) {                                      // n_footprint cleared; the chunks' least keys all ones: the rollout lowers them
        HIPCHK(e, hipMemsetAsync(p.foot_info + (size_t)LOC_F_FOOTPRINT * p.state_stride, 0, (size_t)p.state_stride * sizeof(int), s));
        HIPCHK(e, hipMemsetAsync(p.partial, 0xFF, (size_t)p.batch * LOC_MAX_CHUNKS * sizeof(unsigned long long), s));
    }
    launch_local_rollout(p, s);
    launch_local_finish(p, s);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

}  // namespace

// the source's navigation function has run and the inflated grids it read are still the ones that lie there: the same
// buffers of the same shape (a freed one would be read otherwise), and no pp_inflate_async since (the buffers are reused
// while the shape stands, so the pointer alone would pass the next cycle's grids under this cycle's field)
int check_navfn_run(pp_engine* e, const char* who, int source) {
    const pp_engine::Navfn& g = e->navfn[source];
    const pp_engine::Inflation& in = e->infl[source];
    const NavParams& r = g.run;
    if (in.out != r.grid || in.cells != r.stride || in.run_w != r.width || in.run_h != r.height || in.run_pitch != r.pitch || in.batch < g.batch ||
        in.run_id != g.infl_run)
        return fail(e, PP_ERR_STATE, "%s: the inflated grids of the %s source were re-made since its navigation function ran "
                    "(pp_navfn_async again)", who, source_name(source));
    return PP_OK;
}

void local_plan_release(pp_engine* e) {
    for (pp_engine::LocalPlan& g : e->local) {
        g.mem.release();
        g.ring.release();
        g = pp_engine::LocalPlan();
    }
}

extern "C" {

int pp_set_local_plan(pp_handle e, int32_t source, const pp_local_plan_config* cfg, const int32_t* trig, int32_t n_trig) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_local_plan";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::LocalPlan& g = e->local[source];
    if (!cfg) { g.on = false; return PP_OK; }
    const pp_local_plan_config c = *cfg;
    if (int st = check_config(e, who, c)) return st;
    std::vector<unsigned> packed;
    if (int st = pack_trig(e, who, trig, n_trig, packed)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // a run in flight reads the table to its end
    HIPCHK(e, g.h_call.alloc(g.ring, (size_t)e->B));
    if (!g.d_call) {
        DevAlloc A{e};
        A(&g.trig, (size_t)PP_LOCAL_HEADINGS); A(&g.state, (size_t)LOC_STATE * e->B); A(&g.partial, (size_t)LOC_MAX_CHUNKS * e->B);
        A(&g.score, (size_t)e->B); A(&g.d_call, (size_t)e->B);                    // (d_call last: the ready flag)
        if (A.st) return A.st;
    }
    HIPCHK(e, hipMemcpy(g.trig, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_local_plan_config(pp_handle e, int32_t source, int32_t* on, pp_local_plan_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_local_plan_config", source)) return st;
    *on = e->local[source].on ? 1 : 0;
    if (cfg_out) *cfg_out = e->local[source].cfg;
    return PP_OK;
}

int pp_set_local_movers(pp_handle e, int32_t source, const pp_local_mover_config* cfg) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_local_movers";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::LocalPlan& g = e->local[source];
    if (!cfg) { g.movers_on = false; return PP_OK; }
    const pp_local_mover_config c = *cfg;
    if (int st = check_mover_ints(e, who, c.horizon, c.mover_weight)) return st;
    if (!std::isfinite(c.pad_hard) || !std::isfinite(c.pad_soft) || c.pad_hard < 0.0 || c.pad_soft < c.pad_hard)
        return fail(e, PP_ERR_ARG, "%s: pad_hard = %g, pad_soft = %g: finite and 0 <= pad_hard <= pad_soft", who, c.pad_hard, c.pad_soft);
    if (c.confirmed_only != 0 && c.confirmed_only != 1) return fail(e, PP_ERR_ARG, "%s: confirmed_only = %d outside [0, 1]", who, c.confirmed_only);
    if (c.reserved != 0) return fail(e, PP_ERR_ARG, "%s: reserved = %d must be 0", who, c.reserved);
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // (a run in flight took its configuration by value; as pp_set_local_plan)
    HIPCHK(e, g.h_frame.alloc(g.ring, (size_t)e->B));
    if (!g.d_frame) {
        DevAlloc A{e};
        A(&g.movers, (size_t)e->B * PP_LOCAL_MAX_MOVERS * 6); A(&g.mover_info, (size_t)PP_LOCAL_MOVER_INFO * e->B);
        A(&g.d_frame, (size_t)e->B);                     // (d_frame last: the ready flag)
        if (A.st) return A.st;
    }
    g.mcfg = c;
    g.movers_on = true;
    return PP_OK;
}

int pp_get_local_movers_config(pp_handle e, int32_t source, int32_t* on, pp_local_mover_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_local_movers_config", source)) return st;
    *on = e->local[source].movers_on ? 1 : 0;
    if (cfg_out) *cfg_out = e->local[source].mcfg;
    return PP_OK;
}

int pp_set_local_footprint(pp_handle e, int32_t source, const pp_local_footprint_config* cfg, const int32_t* probes, int32_t n) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_local_footprint";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::LocalPlan& g = e->local[source];
    if (n == 0 && !probes) { g.foot_on = false; return PP_OK; }
    if (!cfg) return fail(e, PP_ERR_ARG, "%s: cfg is NULL (n = 0 with probes NULL turns the footprint off)", who);
    const pp_local_footprint_config c = *cfg;
    for (int i = 0; i < 3; ++i)
        if (c.reserved[i] != 0) return fail(e, PP_ERR_ARG, "%s: reserved[%d] = %d must be 0", who, i, c.reserved[i]);
    std::vector<unsigned> packed;
    if (int st = check_footprint(e, who, c.foot_lethal, probes, n, packed)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));          // a run in flight reads the table to its end
    if (!g.foot_info) {
        DevAlloc A{e};
        A(&g.d_probes, (size_t)PP_LOCAL_MAX_PROBES); A(&g.foot_info, (size_t)PP_LOCAL_FOOT_INFO * e->B);      // (foot_info last: the ready flag)
        if (A.st) return A.st;
    }
    HIPCHK(e, hipMemcpy(g.d_probes, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    if (g.run.probes) g.batch = 0;                       // a getter could queue the last run again, on a table that is gone
    g.probes.assign(probes, probes + (size_t)2 * n);
    g.fcfg = c;
    g.foot_on = true;
    return PP_OK;
}

int pp_get_local_footprint_config(pp_handle e, int32_t source, int32_t* on, pp_local_footprint_config* cfg_out, int32_t* probes_out,
                                  int32_t* n_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_local_footprint_config", source)) return st;
    const pp_engine::LocalPlan& g = e->local[source];
    *on = g.foot_on ? 1 : 0;
    if (cfg_out) *cfg_out = g.fcfg;
    if (probes_out && !g.probes.empty()) memcpy(probes_out, g.probes.data(), g.probes.size() * sizeof(int32_t));
    if (n_out) *n_out = (int32_t)(g.probes.size() / 2);
    return PP_OK;
}

// pp_local_plan_async (frame == NULL) and pp_local_plan_movers_async
static int plan_async(pp_engine* e, const char* who, int32_t source, const int32_t* poses, const int32_t* windows,
                      const double* frame, bool with_movers, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (int st = check_source(e, who, source)) return st;
    if (!poses || !windows) return fail(e, PP_ERR_ARG, "%s: poses or windows is NULL", who);
    pp_engine::LocalPlan& g = e->local[source];
    const pp_engine::Navfn& nav = e->navfn[source];
    const char* name = source_name(source);
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the local planner of the %s source is not configured (pp_set_local_plan first)", who, name);
    if (!nav.on) return fail(e, PP_ERR_STATE, "%s: the navigation function of the %s source is not configured (pp_set_navfn first)", who, name);
    if (int st = check_last_run(e, who, nav.pot[0] ? nav.batch : 0, batch, false, "no navigation function has run on this source (pp_navfn_async first)",
                                "navigation function", "grids")) return st;
    if (int st = check_navfn_run(e, who, source)) return st;
    if (int st = fill_calls(e, who, nullptr, g.cfg, poses, windows, nullptr, batch)) return st;
    if (with_movers) {
        if (!g.movers_on) return fail(e, PP_ERR_STATE, "%s: the movers of the %s source are not configured (pp_set_local_movers first)", who, name);
        if (!e->trk.ready) return fail(e, PP_ERR_STATE, "%s: the handle has no track tables (pp_set_tracking first)", who);
        if (!frame) return fail(e, PP_ERR_ARG, "%s: frame is NULL", who);
        for (int b = 0; b < batch; ++b) {
            const double* f = frame + (size_t)4 * b;
            if (!std::isfinite(f[0]) || !std::isfinite(f[1])) return fail(e, PP_ERR_ARG, "%s: frame: grid %d: origin (%g, %g) must be finite", who, b, f[0], f[1]);
            if (!std::isfinite(f[2]) || !(f[2] > 0.0)) return fail(e, PP_ERR_ARG, "%s: frame: grid %d: res = %g (must be finite and > 0)", who, b, f[2]);
            if (!std::isfinite(f[3]) || !(f[3] > 0.0)) return fail(e, PP_ERR_ARG, "%s: frame: grid %d: dt = %g (must be finite and > 0)", who, b, f[3]);
        }
    }
    const int samples = g.cfg.nv * g.cfg.nw;
    (void)hipSetDevice(e->device);
    if (samples > g.samples_cap || g.cfg.steps > g.steps_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a run in flight writes the old buffers to its end
        g.mem.release();
        g.samples_cap = 0; g.steps_cap = 0; g.batch = 0;
        StageMem& M = g.mem;
        M(&g.keys, (size_t)e->B * samples); M(&g.traj, (size_t)e->B * (g.cfg.steps + 1) * 3);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d grids x %d samples and %d steps need %zu bytes of device memory and the device cannot "
                        "hold them (%s)", who, e->B, samples, g.cfg.steps, (size_t)e->B * ((size_t)samples * 8 + (size_t)(g.cfg.steps + 1) * 12),
                        hipGetErrorString(st));
        }
        g.samples_cap = samples; g.steps_cap = g.cfg.steps;
    }
    int slot;
    HIPCHK(e, g.ring.take(&slot));                       // behind the last check that can refuse
    (void)fill_calls(e, who, g.h_call.at(slot), g.cfg, poses, windows, nullptr, batch);
    const NavParams& r = nav.run;
    LocalParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = r.width; p.height = r.height; p.pitch = r.pitch; p.stride = r.stride;
    p.lethal = r.lethal; p.allow_unknown = r.allow_unknown; p.unknown_cost = r.unknown_cost;
    fill_config(p, g.cfg);
    p.grid = r.grid; p.pot = r.pot[nav.rounds & 1]; p.nav_call = r.call; p.nav_state = r.state; p.nav_state_stride = r.state_stride;
    p.call = g.d_call; p.trig = g.trig; p.partial = g.partial;
    p.state = g.state; p.state_stride = e->B; p.score = g.score; p.traj = g.traj;
    p.keys = nullptr;                                    // stored when a getter asks for them
    prof_reset(e);
    HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
    if (with_movers) {
        memcpy(g.h_frame.at(slot), frame, (size_t)batch * sizeof(LocalFrame));
        HIPCHK(e, g.h_frame.send(slot, g.d_frame, (size_t)batch, e->stream));
        p.movers = g.movers; p.mover_info = g.mover_info; p.horizon = g.mcfg.horizon; p.mover_w = g.mcfg.mover_weight;
    }
    if (g.foot_on) {
        p.probes = g.d_probes; p.n_probes = (int)(g.probes.size() / 2); p.foot_lethal = g.fcfg.foot_lethal; p.foot_info = g.foot_info;
    }
    HIPCHK(e, g.ring.sent(slot, e->stream));
    {
        ProfScope ps(e, nullptr);
        if (with_movers) {
            LocalMoverParams m;
            memset(&m, 0, sizeof(m));
            m.batch = batch; m.fixed = source == PP_INFLATE_OCCUPANCY ? 1 : 0; m.confirmed_only = g.mcfg.confirmed_only;
            m.pad_hard = g.mcfg.pad_hard; m.pad_soft = g.mcfg.pad_soft;
            m.slots = e->trk.state; m.pose_prev = e->trk.d_pose_prev; m.frame = g.d_frame;
            m.movers = g.movers; m.mover_info = g.mover_info; m.info_stride = e->B;
            launch_local_movers(m, e->stream);
        }
        if (int st = queue_run(e, p, e->stream)) return st;
    }
    g.batch = batch; g.run = p; g.nav_run = nav.run_id; g.nav_rounds = nav.rounds;
    return PP_OK;
}

int pp_local_plan_async(pp_handle e, int32_t source, const int32_t* poses, const int32_t* windows, int32_t batch) {
    return plan_async(e, "pp_local_plan_async", source, poses, windows, nullptr, false, batch);
}

int pp_local_plan_movers_async(pp_handle e, int32_t source, const int32_t* poses, const int32_t* windows, const double* frame,
                               int32_t batch) {
    return plan_async(e, "pp_local_plan_movers_async", source, poses, windows, frame, true, batch);
}

// what both getters do before they copy: the field settled, and rollout and finish queued again where it moved on or the
// keys are missing; then the stream waited for
static int settle_local(pp_engine* e, const char* who, int32_t source, bool want_keys, int32_t batch) {
    pp_engine::LocalPlan& g = e->local[source];
    if (int st = check_last_run(e, who, g.batch, batch, false, "no local plan has run on this source (pp_local_plan_async first)",
                                "run", "grids")) return st;
    if (g.nav_run != e->navfn[source].run_id)
        return fail(e, PP_ERR_STATE, "%s: a pp_navfn_async of the %s source came after the last pp_local_plan_async (pp_local_plan_async again)",
                    who, source_name(source));
    pp_engine::Navfn* nav = nullptr;
    if (int st = settled_run(e, who, source, batch, &nav)) return st;
    LocalParams& p = g.run;
    if (nav->rounds != g.nav_rounds || (want_keys && !p.keys)) {      // the field moved on behind the launches, or no keys yet: again
        if (int st = check_navfn_run(e, who, source)) return st;
        p.pot = nav->run.pot[nav->rounds & 1];
        if (want_keys) p.keys = g.keys;
        prof_reset(e);
        ProfScope ps(e, nullptr);
        if (int st = queue_run(e, p, e->stream)) return st;
        g.nav_rounds = nav->rounds;
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

int pp_get_local_plan(pp_handle e, int32_t source, int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_local_plan";
    if (int st = check_source(e, who, source)) return st;
    if (int st = settle_local(e, who, source, keys != nullptr, batch)) return st;
    const LocalParams& p = e->local[source].run;
    const size_t ss = (size_t)p.state_stride;
    if (result) {
        std::vector<int> host((size_t)LOC_STATE * ss);
        HIPCHK(e, hipMemcpy(host.data(), p.state, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < LOC_STATE; ++k) result[(size_t)b * PP_LOCAL_RESULT + k] = host[(size_t)k * ss + b];
    }
    if (score) HIPCHK(e, hipMemcpy(score, p.score, (size_t)batch * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (traj) HIPCHK(e, hipMemcpy(traj, p.traj, (size_t)batch * (p.steps + 1) * 3 * sizeof(int), hipMemcpyDeviceToHost));
    if (keys) HIPCHK(e, hipMemcpy(keys, p.keys, (size_t)batch * p.nv * p.nw * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_get_local_movers(pp_handle e, int32_t source, int32_t* movers, int32_t* info, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_local_movers";
    if (int st = check_source(e, who, source)) return st;
    const pp_engine::LocalPlan& g = e->local[source];
    if (g.batch >= 1 && !g.run.movers)
        return fail(e, PP_ERR_STATE, "%s: the last run of the %s source was a pp_local_plan_async, it had no movers (pp_local_plan_movers_async first)",
                    who, source_name(source));
    if (int st = settle_local(e, who, source, false, batch)) return st;
    const LocalParams& p = g.run;
    const size_t ss = (size_t)p.state_stride;
    if (movers) HIPCHK(e, hipMemcpy(movers, p.movers, (size_t)batch * PP_LOCAL_MAX_MOVERS * 6 * sizeof(int), hipMemcpyDeviceToHost));
    if (info) {
        std::vector<int> host((size_t)PP_LOCAL_MOVER_INFO * ss);
        HIPCHK(e, hipMemcpy(host.data(), p.mover_info, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < PP_LOCAL_MOVER_INFO; ++k) info[(size_t)b * PP_LOCAL_MOVER_INFO + k] = host[(size_t)k * ss + b];
    }
    return PP_OK;
}

int pp_get_local_footprint(pp_handle e, int32_t source, int32_t* info, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_local_footprint";
    if (int st = check_source(e, who, source)) return st;
    const pp_engine::LocalPlan& g = e->local[source];
    if (g.batch >= 1 && !g.run.probes)
        return fail(e, PP_ERR_STATE, "%s: the last run of the %s source had no footprint (pp_set_local_footprint, then pp_local_plan_async)",
                    who, source_name(source));
    if (int st = settle_local(e, who, source, false, batch)) return st;
    const LocalParams& p = g.run;
    const size_t ss = (size_t)p.state_stride;
    if (info) {
        std::vector<int> host((size_t)PP_LOCAL_FOOT_INFO * ss);
        HIPCHK(e, hipMemcpy(host.data(), p.foot_info, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < PP_LOCAL_FOOT_INFO; ++k) info[(size_t)b * PP_LOCAL_FOOT_INFO + k] = host[(size_t)k * ss + b];
    }
    return PP_OK;
}

// pp_local_plan_grids (movers == NULL, probes == NULL), pp_local_plan_grids_movers and pp_local_plan_grids_footprint
static int plan_grids(const char* who, int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height, int32_t width,
                      const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg, const int32_t* trig, int32_t n_trig,
                      const int32_t* poses, const int32_t* windows, const int32_t* goal_state, bool with_movers, int32_t horizon,
                      int32_t mover_weight, const int32_t* movers, const int32_t* n_movers, int32_t* result, uint64_t* score,
                      int32_t* traj, uint64_t* keys, int32_t* info, bool with_foot = false, const int32_t* probes = nullptr,
                      int32_t n_probes = 0, int32_t foot_lethal = 0, int32_t* foot_info = nullptr) {
    if (!grids || !pots || !navfn_cfg || !cfg) return fail(nullptr, PP_ERR_ARG, "%s: grids, pots, navfn_cfg or cfg is NULL", who);
    if (!poses || !windows) return fail(nullptr, PP_ERR_ARG, "%s: poses or windows is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (int st = check_cfg_window(nullptr, who, width, height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    const struct { const char* name; int v, lo, hi; } f[] = {{"lethal_cost", navfn_cfg->lethal_cost, 1, 100},
        {"allow_unknown", navfn_cfg->allow_unknown, 0, 1}, {"unknown_cost", navfn_cfg->unknown_cost, 0, 100}};
    for (const auto& x : f)
        if (x.v < x.lo || x.v > x.hi) return fail(nullptr, PP_ERR_ARG, "%s: %s = %d outside [%d, %d]", who, x.name, x.v, x.lo, x.hi);
    if (int st = check_config(nullptr, who, *cfg)) return st;
    std::vector<unsigned> packed;
    if (int st = pack_trig(nullptr, who, trig, n_trig, packed)) return st;
    std::vector<LocalCall> calls((size_t)batch);
    if (int st = fill_calls(nullptr, who, calls.data(), *cfg, poses, windows, goal_state, batch)) return st;
    std::vector<int> minfo;
    if (with_movers) {
        if (!movers || !n_movers) return fail(nullptr, PP_ERR_ARG, "%s: movers or n_movers is NULL", who);
        if (int st = check_mover_ints(nullptr, who, horizon, mover_weight)) return st;
        if (int st = check_movers(who, movers, n_movers, batch)) return st;
        minfo.assign((size_t)PP_LOCAL_MOVER_INFO * batch, 0);
        for (int b = 0; b < batch; ++b) minfo[(size_t)LOC_M_COUNT * batch + b] = n_movers[b];
    }
    std::vector<unsigned> probe_words;
    if (with_foot)
        if (int st = check_footprint(nullptr, who, foot_lethal, probes, n_probes, probe_words)) return st;
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    const size_t cells = (size_t)width * height, n = (size_t)batch * cells;
    const size_t samples = (size_t)cfg->nv * cfg->nw, words = (size_t)(cfg->steps + 1) * 3;
    DevBuf d_grid, d_pot, d_trig, d_call, d_state, d_partial, d_score, d_traj, d_keys, d_movers, d_minfo;
    DEVCHK(d_grid.alloc(n));
    DEVCHK(d_pot.alloc(n * sizeof(unsigned)));
    DEVCHK(d_trig.alloc(packed.size() * sizeof(unsigned)));
    DEVCHK(d_call.alloc((size_t)batch * sizeof(LocalCall)));
    DEVCHK(d_state.alloc((size_t)LOC_STATE * batch * sizeof(int)));
    DEVCHK(d_partial.alloc((size_t)LOC_MAX_CHUNKS * batch * sizeof(unsigned long long)));
    DEVCHK(d_score.alloc((size_t)batch * sizeof(unsigned long long)));
    DEVCHK(d_traj.alloc((size_t)batch * words * sizeof(int)));
    if (keys) DEVCHK(d_keys.alloc((size_t)batch * samples * sizeof(unsigned long long)));
    DEVCHK(hipMemcpy(d_grid.p, grids, n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_pot.p, pots, n * sizeof(unsigned), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_trig.p, packed.data(), packed.size() * sizeof(unsigned), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_call.p, calls.data(), (size_t)batch * sizeof(LocalCall), hipMemcpyHostToDevice));
    LocalParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = width; p.height = height; p.pitch = width; p.stride = cells;
    p.lethal = navfn_cfg->lethal_cost; p.allow_unknown = navfn_cfg->allow_unknown; p.unknown_cost = navfn_cfg->unknown_cost;
    fill_config(p, *cfg);
    p.grid = (const int8_t*)d_grid.p; p.pot = (const unsigned*)d_pot.p;
    p.call = (const LocalCall*)d_call.p; p.trig = (const unsigned*)d_trig.p; p.partial = (unsigned long long*)d_partial.p;
    p.state = (int*)d_state.p; p.state_stride = batch; p.score = (unsigned long long*)d_score.p; p.traj = (int*)d_traj.p;
    p.keys = keys ? (unsigned long long*)d_keys.p : nullptr;
    if (with_movers) {
        const size_t table = (size_t)batch * PP_LOCAL_MAX_MOVERS * 6 * sizeof(int);
        DEVCHK(d_movers.alloc(table));
        DEVCHK(d_minfo.alloc(minfo.size() * sizeof(int)));
        DEVCHK(hipMemcpy(d_movers.p, movers, table, hipMemcpyHostToDevice));
        DEVCHK(hipMemcpy(d_minfo.p, minfo.data(), minfo.size() * sizeof(int), hipMemcpyHostToDevice));
        p.movers = (const int*)d_movers.p; p.mover_info = (int*)d_minfo.p; p.horizon = horizon; p.mover_w = mover_weight;
    }
    DevBuf d_probes, d_finfo;
    if (with_foot) {
        DEVCHK(d_probes.alloc(probe_words.size() * sizeof(unsigned)));
        DEVCHK(d_finfo.alloc((size_t)PP_LOCAL_FOOT_INFO * batch * sizeof(int)));
        DEVCHK(hipMemcpy(d_probes.p, probe_words.data(), probe_words.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        p.probes = (const unsigned*)d_probes.p; p.n_probes = n_probes; p.foot_lethal = foot_lethal; p.foot_info = (int*)d_finfo.p;
    }
    if (int st = queue_run(nullptr, p, nullptr)) return st;
    DEVCHK(hipStreamSynchronize(nullptr));
    if (with_foot && foot_info) {
        std::vector<int> host((size_t)PP_LOCAL_FOOT_INFO * batch);
        DEVCHK(hipMemcpy(host.data(), p.foot_info, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < PP_LOCAL_FOOT_INFO; ++k) foot_info[(size_t)b * PP_LOCAL_FOOT_INFO + k] = host[(size_t)k * batch + b];
    }
    if (with_movers && info) {
        DEVCHK(hipMemcpy(minfo.data(), p.mover_info, minfo.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < PP_LOCAL_MOVER_INFO; ++k) info[(size_t)b * PP_LOCAL_MOVER_INFO + k] = minfo[(size_t)k * batch + b];
    }
    if (result) {
        std::vector<int> host((size_t)LOC_STATE * batch);
        DEVCHK(hipMemcpy(host.data(), p.state, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < LOC_STATE; ++k) result[(size_t)b * PP_LOCAL_RESULT + k] = host[(size_t)k * batch + b];
    }
    if (score) DEVCHK(hipMemcpy(score, p.score, (size_t)batch * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (traj) DEVCHK(hipMemcpy(traj, p.traj, (size_t)batch * words * sizeof(int), hipMemcpyDeviceToHost));
    if (keys) DEVCHK(hipMemcpy(keys, p.keys, (size_t)batch * samples * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_local_plan_grids(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height, int32_t width,
                        const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg, const int32_t* trig, int32_t n_trig,
                        const int32_t* poses, const int32_t* windows, const int32_t* goal_state, int32_t* result, uint64_t* score,
                        int32_t* traj, uint64_t* keys) {
    return plan_grids("pp_local_plan_grids", device, grids, pots, batch, height, width, navfn_cfg, cfg, trig, n_trig, poses, windows,
                      goal_state, false, 0, 0, nullptr, nullptr, result, score, traj, keys, nullptr);
}

int pp_local_plan_grids_movers(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height,
                               int32_t width, const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg,
                               const int32_t* trig, int32_t n_trig, const int32_t* poses, const int32_t* windows,
                               const int32_t* goal_state, int32_t horizon, int32_t mover_weight, const int32_t* movers,
                               const int32_t* n_movers, int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys,
                               int32_t* info) {
    return plan_grids("pp_local_plan_grids_movers", device, grids, pots, batch, height, width, navfn_cfg, cfg, trig, n_trig, poses,
                      windows, goal_state, true, horizon, mover_weight, movers, n_movers, result, score, traj, keys, info);
}

int pp_local_plan_grids_footprint(int device, const int8_t* grids, const uint32_t* pots, int32_t batch, int32_t height,
                                  int32_t width, const pp_navfn_config* navfn_cfg, const pp_local_plan_config* cfg,
                                  const int32_t* trig, int32_t n_trig, const int32_t* poses, const int32_t* windows,
                                  const int32_t* goal_state, int32_t horizon, int32_t mover_weight, const int32_t* movers,
                                  const int32_t* n_movers, const int32_t* probes, int32_t n_probes, int32_t foot_lethal,
                                  int32_t* result, uint64_t* score, int32_t* traj, uint64_t* keys, int32_t* info,
                                  int32_t* foot_info) {
    return plan_grids("pp_local_plan_grids_footprint", device, grids, pots, batch, height, width, navfn_cfg, cfg, trig, n_trig, poses,
                      windows, goal_state, movers != nullptr, horizon, mover_weight, movers, n_movers, result, score, traj, keys, info,
                      true, probes, n_probes, foot_lethal, foot_info);
}

}  // extern "C"
