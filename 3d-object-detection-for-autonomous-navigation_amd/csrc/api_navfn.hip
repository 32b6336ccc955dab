// C-ABI, navigation function (pp_set_navfn, pp_get_navfn_config, pp_navfn_async, pp_get_navfn, pp_navfn_info,
// pp_navfn_grids): the inflated int8 grid a source's inflation leaves on the device -> the cost-to-go field from one goal
// cell per grid and the path that descends it from one start cell (kernels: navfn.hip; the rule: navfn.py).  A stage
// behind either inflation: init, relaxation rounds and finish as plain launches on the handle's stream.  pp_navfn_async
// queues a number of rounds and returns; a getter waits, reads the grids' `changed` flags and, while a grid's last round
// still moved a cell, queues further rounds in groups and runs finish again -- height * width rounds at the most, which
// provably suffice (a round finalises at least one more cell, the last one changes nothing).  So a fetched field is always
// the exact one, whatever queued_rounds says.  The goals and starts travel from the host on every call and are consumed on
// the main stream: a call ring of the stage's own (pp_ring.h).  pp_navfn_grids needs no handle: host buffers in, host
// buffers out, device memory for the call's duration.
#include "pp_engine.h"

static_assert(sizeof(pp_navfn_config) == 32, "pp_navfn_config: 8 int32 (the Python binding mirrors it)");
static_assert(sizeof(NavCall) == 20, "NavCall: 5 int32, packed by the host per grid");
static_assert(PP_NAVFN_MAX_PATH == 4096, "a path's cells");
static_assert(PP_INFLATE_COSTMAP == 0 && PP_INFLATE_OCCUPANCY == 1, "pp_engine::navfn is indexed by source, as infl");

namespace {

const char* source_name(int source) { return source == PP_INFLATE_COSTMAP ? "costmap" : "occupancy"; }

// Everything pp_set_navfn and pp_navfn_grids refuse of a configuration, by field name.  The ranges are what keeps a uint32
// potential from overflowing: c <= 50 + 5 * 100.
int check_config(pp_engine* e, const char* who, const pp_navfn_config& c) {
    const struct { const char* name; int v, lo, hi; } f[] = {
        {"lethal_cost", c.lethal_cost, 1, 100}, {"neutral_cost", c.neutral_cost, 1, 50}, {"cost_factor", c.cost_factor, 0, 5},
        {"allow_unknown", c.allow_unknown, 0, 1}, {"unknown_cost", c.unknown_cost, 0, 100}, {"connectivity", c.connectivity, 4, 8},
        {"max_path", c.max_path, 1, PP_NAVFN_MAX_PATH}, {"queued_rounds", c.queued_rounds, 0, 4096}};
    for (const auto& x : f)
        if (x.v < x.lo || x.v > x.hi) return fail(e, PP_ERR_ARG, "%s: %s = %d outside [%d, %d]", who, x.name, x.v, x.lo, x.hi);
    if (c.connectivity != 4 && c.connectivity != 8) return fail(e, PP_ERR_ARG, "%s: connectivity = %d must be 4 or 8", who, c.connectivity);
    return PP_OK;
}

int check_source(pp_engine* e, const char* who, int source) {
    if (source != PP_INFLATE_COSTMAP && source != PP_INFLATE_OCCUPANCY)
        return fail(e, PP_ERR_ARG, "%s: source = %d (0 PP_INFLATE_COSTMAP, 1 PP_INFLATE_OCCUPANCY)", who, source);
    return PP_OK;
}

void fill_config(NavParams& p, const pp_navfn_config& c) {
    p.lethal = c.lethal_cost; p.neutral = c.neutral_cost; p.factor = c.cost_factor; p.allow_unknown = c.allow_unknown;
    p.unknown_cost = c.unknown_cost; p.conn = c.connectivity; p.max_path = c.max_path;
}

void fill_calls(NavCall* call, const int32_t* goals, const int32_t* starts, int batch, const char* known) {
    for (int b = 0; b < batch; ++b) {
        NavCall& c = call[b];
        c.gx = goals[2 * b]; c.gy = goals[2 * b + 1];
        c.sx = starts ? starts[2 * b] : -1; c.sy = starts ? starts[2 * b + 1] : -1;
        c.flags = (starts ? NAV_HAS_START : 0) | (!known || known[b] ? NAV_KNOWN : 0);
    }
}

// the rounds a call queues when its configuration leaves that open, and a getter's group: a front crosses a tile per
// round at the least, so this reaches across an open grid
int default_rounds(int width, int height) {
    int tx = 0;
    const int tiles = navfn_tiles(width, height, &tx);
    return std::min(tx + tiles / tx + 2, 128);
}

// init + `rounds` rounds + finish behind whatever `s` holds
int queue_run(pp_engine* e, const NavParams& p, int rounds, hipStream_t s) {
    launch_navfn_init(p, s);
    for (int r = 0; r < rounds; ++r) launch_navfn_relax(p, r, s);
    launch_navfn_finish(p, rounds, s);                   // (init cleared NAV_REACHED)
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

}  // namespace

// Waits for `s`, then queues rounds in groups until the last round of every grid changed nothing; `host` then holds the
// state words and `s` is idle.  *rounds: queued so far, >= 1.
int settle(pp_engine* e, const char* who, const NavParams& p, int* rounds, hipStream_t s, std::vector<int>& host) {
    const long long cap = (long long)p.width * p.height;
    const int group = default_rounds(p.width, p.height);
    host.assign((size_t)NAV_STATE * p.state_stride, 0);
    for (;;) {
        HIPCHK(e, hipStreamSynchronize(s));
        HIPCHK(e, hipMemcpy(host.data(), p.state, host.size() * sizeof(int), hipMemcpyDeviceToHost));
        bool stands = true;
        for (int b = 0; b < p.batch; ++b)
            stands = stands && host[(size_t)(NAV_CHANGED + (*rounds - 1) % 3) * p.state_stride + b] == 0;
        if (stands) return PP_OK;
        const int n = (int)std::min<long long>(group, cap - *rounds);
        if (n < 1) return fail(e, PP_ERR_INTERNAL, "%s: the field still moves after %d rounds on %d x %d cells", who, *rounds, p.width, p.height);
        for (int r = 0; r < n; ++r) launch_navfn_relax(p, *rounds + r, s);
        *rounds += n;
        HIPCHK(e, hipMemsetAsync(p.state + (size_t)NAV_REACHED * p.state_stride, 0, (size_t)p.batch * sizeof(int), s));
        launch_navfn_finish(p, *rounds, s);
        HIPCHK(e, hipGetLastError());
    }
}

// what both getters start with: the last run, settled
int settled_run(pp_engine* e, const char* who, int source, int batch, pp_engine::Navfn** out) {
    if (int st = check_source(e, who, source)) return st;
    pp_engine::Navfn& g = e->navfn[source];
    if (int st = check_last_run(e, who, g.pot[0] ? g.batch : 0, batch, false, "no navigation function has run on this source (pp_navfn_async first)",
                                "run", "grids")) return st;
    (void)hipSetDevice(e->device);
    if (!g.settled) {
        prof_reset(e);
        ProfScope ps(e, nullptr);
        if (int st = settle(e, who, g.run, &g.rounds, e->stream, g.host)) return st;
        g.settled = true;
    }
    *out = &g;
    return PP_OK;
}

void navfn_release(pp_engine* e) {
    for (pp_engine::Navfn& g : e->navfn) {
        g.mem.release();
        g.ring.release();
        g = pp_engine::Navfn();
    }
}

extern "C" {

int pp_set_navfn(pp_handle e, int32_t source, const pp_navfn_config* cfg) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_navfn";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::Navfn& g = e->navfn[source];
    if (!cfg) { g.on = false; return PP_OK; }
    const pp_navfn_config c = *cfg;
    if (int st = check_config(e, who, c)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, g.h_call.alloc(g.ring, (size_t)e->B));
    if (!g.d_call) {
        DevAlloc A{e};
        A(&g.state, (size_t)NAV_STATE * e->B); A(&g.d_call, (size_t)e->B);       // (d_call last: the ready flag)
        if (A.st) return A.st;
    }
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_navfn_config(pp_handle e, int32_t source, int32_t* on, pp_navfn_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_navfn_config", source)) return st;
    *on = e->navfn[source].on ? 1 : 0;
    if (cfg_out) *cfg_out = e->navfn[source].cfg;
    return PP_OK;
}

int pp_navfn_async(pp_handle e, int32_t source, const int32_t* goals, const int32_t* starts, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_navfn_async";
    if (int st = check_source(e, who, source)) return st;
    if (!goals) return fail(e, PP_ERR_ARG, "%s: goals is NULL", who);
    pp_engine::Navfn& g = e->navfn[source];
    const pp_engine::Inflation& in = e->infl[source];
    const char* name = source_name(source);
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the navigation function of the %s source is not configured (pp_set_navfn first)", who, name);
    if (!in.on) return fail(e, PP_ERR_STATE, "%s: the inflation of the %s source is not configured (pp_set_inflation first)", who, name);
    if (int st = check_last_run(e, who, in.out ? in.batch : 0, batch, false, "no inflation has run on this source (pp_inflate_async first)",
                                "inflation", "grids")) return st;
    const int W = in.run_w, H = in.run_h, pitch = in.run_pitch;
    const size_t cells = (size_t)pitch * H;
    (void)hipSetDevice(e->device);
    if (cells != g.cells || g.cfg.max_path > g.path_cap) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a run in flight writes the old buffers to its end
        g.mem.release();
        g.cells = 0; g.path_cap = 0; g.batch = 0;
        StageMem& M = g.mem;
        M(&g.cost, (size_t)e->B * cells); M(&g.pot[0], (size_t)e->B * cells); M(&g.pot[1], (size_t)e->B * cells);
        M(&g.paths, (size_t)e->B * g.cfg.max_path * 2);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d grids x %zu cells (rows of %d) need %zu bytes of device memory and the device cannot "
                        "hold them (%s)", who, e->B, cells, pitch, (size_t)e->B * cells * 10, hipGetErrorString(st));
        }
        g.cells = cells; g.path_cap = g.cfg.max_path;
    }
    int slot;
    HIPCHK(e, g.ring.take(&slot));                       // behind the last check that can refuse
    fill_calls(g.h_call.at(slot), goals, starts, batch, in.known.data());
    NavParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = W; p.height = H; p.pitch = pitch; p.stride = cells;
    fill_config(p, g.cfg);
    p.grid = in.out; p.call = g.d_call;
    p.cost = g.cost; p.pot[0] = g.pot[0]; p.pot[1] = g.pot[1];
    p.state = g.state; p.state_stride = e->B; p.paths = g.paths;
    const int rounds = g.cfg.queued_rounds > 0 ? g.cfg.queued_rounds : default_rounds(W, H);
    prof_reset(e);
    HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
    HIPCHK(e, g.ring.sent(slot, e->stream));
    {
        ProfScope ps(e, nullptr);
        if (int st = queue_run(e, p, rounds, e->stream)) return st;
    }
    g.batch = batch; g.run = p; g.rounds = rounds; g.settled = false;
    ++g.run_id;
    g.infl_run = in.run_id;
    return PP_OK;
}

int pp_get_navfn(pp_handle e, int32_t source, uint32_t* pot, int32_t* paths, int32_t* path_len, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_navfn";
    pp_engine::Navfn* gp = nullptr;
    if (int st = settled_run(e, who, source, batch, &gp)) return st;
    const pp_engine::Navfn& g = *gp;
    const NavParams& p = g.run;
    // rows of `pitch` cells on the device, of `width` on the host; the grids lie row behind row in both
    const size_t W = (size_t)p.width, rows = (size_t)batch * p.height;
    if (pot) HIPCHK(e, hipMemcpy2D(pot, W * 4, p.pot[g.rounds & 1], (size_t)p.pitch * 4, W * 4, rows, hipMemcpyDeviceToHost));
    if (paths) HIPCHK(e, hipMemcpy(paths, p.paths, (size_t)batch * p.max_path * 2 * sizeof(int), hipMemcpyDeviceToHost));
    if (path_len)
        for (int b = 0; b < batch; ++b) path_len[b] = g.host[(size_t)NAV_PATH_LEN * p.state_stride + b];
    return PP_OK;
}

int pp_navfn_info(pp_handle e, int32_t source, int32_t* goal_state, int32_t* path_state, int32_t* rounds, int32_t* reached,
                  int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_navfn_info";
    pp_engine::Navfn* gp = nullptr;
    if (int st = settled_run(e, who, source, batch, &gp)) return st;
    const pp_engine::Navfn& g = *gp;
    const size_t ss = (size_t)g.run.state_stride;
    for (int b = 0; b < batch; ++b) {
        if (goal_state) goal_state[b] = g.host[NAV_GOAL_STATE * ss + b];
        if (path_state) path_state[b] = g.host[NAV_PATH_STATE * ss + b];
        if (rounds) rounds[b] = g.host[NAV_ROUNDS * ss + b];
        if (reached) reached[b] = g.host[NAV_REACHED * ss + b];
    }
    return PP_OK;
}

int pp_navfn_grids(int device, const int8_t* grids, int32_t batch, int32_t height, int32_t width, const pp_navfn_config* cfg,
                   const int32_t* goals, const int32_t* starts, uint32_t* pot, int32_t* paths, int32_t* path_len, int32_t* info) {
    const char* who = "pp_navfn_grids";
    if (!grids || !cfg || !goals) return fail(nullptr, PP_ERR_ARG, "%s: grids, cfg or goals is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (int st = check_cfg_window(nullptr, who, width, height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    if (int st = check_config(nullptr, who, *cfg)) return st;
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    const size_t cells = (size_t)width * height, n = (size_t)batch * cells;
    std::vector<NavCall> calls((size_t)batch);
    fill_calls(calls.data(), goals, starts, batch, nullptr);
    DevBuf d_in, d_cost, d_pot0, d_pot1, d_call, d_state, d_paths;
    DEVCHK(d_in.alloc(n));
    DEVCHK(d_cost.alloc(n * sizeof(uint16_t)));
    DEVCHK(d_pot0.alloc(n * sizeof(unsigned)));
    DEVCHK(d_pot1.alloc(n * sizeof(unsigned)));
    DEVCHK(d_call.alloc((size_t)batch * sizeof(NavCall)));
    DEVCHK(d_state.alloc((size_t)NAV_STATE * batch * sizeof(int)));
    DEVCHK(d_paths.alloc((size_t)batch * cfg->max_path * 2 * sizeof(int)));
    DEVCHK(hipMemcpy(d_in.p, grids, n, hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_call.p, calls.data(), (size_t)batch * sizeof(NavCall), hipMemcpyHostToDevice));
    NavParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = width; p.height = height; p.pitch = width; p.stride = cells;
    fill_config(p, *cfg);
    p.grid = (const int8_t*)d_in.p; p.call = (const NavCall*)d_call.p;
    p.cost = (uint16_t*)d_cost.p; p.pot[0] = (unsigned*)d_pot0.p; p.pot[1] = (unsigned*)d_pot1.p;
    p.state = (int*)d_state.p; p.state_stride = batch; p.paths = (int*)d_paths.p;
    int rounds = cfg->queued_rounds > 0 ? cfg->queued_rounds : default_rounds(width, height);
    if (int st = queue_run(nullptr, p, rounds, nullptr)) return st;
    std::vector<int> host;
    if (int st = settle(nullptr, who, p, &rounds, nullptr, host)) return st;
    if (pot) DEVCHK(hipMemcpy(pot, p.pot[rounds & 1], n * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (paths) DEVCHK(hipMemcpy(paths, p.paths, (size_t)batch * cfg->max_path * 2 * sizeof(int), hipMemcpyDeviceToHost));
    const int fields[4] = {NAV_GOAL_STATE, NAV_PATH_STATE, NAV_ROUNDS, NAV_REACHED};
    for (int b = 0; b < batch; ++b) {
        if (path_len) path_len[b] = host[(size_t)NAV_PATH_LEN * batch + b];
        if (info)
            for (int k = 0; k < 4; ++k) info[(size_t)k * batch + b] = host[(size_t)fields[k] * batch + b];
    }
    return PP_OK;
}

}  // extern "C"
