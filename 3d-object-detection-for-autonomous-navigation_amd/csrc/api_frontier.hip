// C-ABI, frontier clusters (pp_set_frontier, pp_get_frontier_config, pp_frontier_async, pp_get_frontiers,
// pp_frontier_grids): the inflated int8 grid a source's inflation leaves on the device -> the clusters of its frontier
// cells, ranked as exploration goals (kernels: frontier.hip; the rule: frontier.py).  A stage behind either inflation: five
// plain launches on the handle's stream, no rounds and no host loop.  With use_field the ranking reads the field the
// source's navigation function leaves on the device, exactly as the local planner does: pp_navfn_async returns before the
// relaxation has converged and only navfn's getters settle it, so pp_get_frontiers first runs navfn's settled_run on the
// source, and if that queued any further round the select launch -- the only one that reads the field -- is queued again.
// A fetched ranking therefore always rests on the exact field, whatever queued_rounds says.  The reference cells travel
// from the host on every call and are consumed on the main stream: a call ring of the stage's own (pp_ring.h).
// pp_frontier_grids needs no handle: host buffers in, host buffers out, device memory for the call's duration.
#include "pp_engine.h"

static_assert(sizeof(pp_frontier_config) == 32, "pp_frontier_config: 8 int32 (the Python binding mirrors it)");
static_assert(sizeof(FrontierCall) == 16, "FrontierCall: 4 int32, packed by the host per grid");
static_assert(PP_FRONTIER_INFO == FR_OVERRUN && PP_FRONTIER_INFO <= FR_INFO_WORDS, "a grid's info words are its first state words");
static_assert(PP_FRONTIER_NONE == PP_NAVFN_UNREACHED, "both read 0xFFFFFFFF");
static_assert(PP_INFLATE_COSTMAP == 0 && PP_INFLATE_OCCUPANCY == 1, "pp_engine::frontier is indexed by source, as infl");

namespace {

constexpr int FR_MAX_REF = 1 << 20;        // |reference coordinate| at most: D < 2^43, and (D << 20) | label fits 64 bits

const char* source_name(int source) { return source == PP_INFLATE_COSTMAP ? "costmap" : "occupancy"; }

// Everything pp_set_frontier and pp_frontier_grids refuse of a configuration, by field name.
int check_config(pp_engine* e, const char* who, const pp_frontier_config& c) {
    const struct { const char* name; int v, lo, hi; } f[] = {
        {"free_max", c.free_max, 0, 99}, {"connectivity", c.connectivity, 4, 8}, {"min_size", c.min_size, 1, PP_OCC_MAX_CELLS},
        {"max_frontiers", c.max_frontiers, 1, PP_FRONTIER_MAX}, {"rank", c.rank, 0, 1}, {"use_field", c.use_field, 0, 1},
        {"reserved[0]", c.reserved[0], 0, 0}, {"reserved[1]", c.reserved[1], 0, 0}};
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

// the calls' records, and what is refused of a reference cell.  `call` may be NULL: check only.
int fill_calls(pp_engine* e, const char* who, FrontierCall* call, const int32_t* refs, int batch, const char* known) {
    for (int b = 0; b < batch; ++b) {
        const int x = refs[2 * b], y = refs[2 * b + 1];
        if (x < -FR_MAX_REF || x > FR_MAX_REF || y < -FR_MAX_REF || y > FR_MAX_REF)
            return fail(e, PP_ERR_ARG, "%s: refs: grid %d: the reference cell (%d, %d) lies outside [-%d, %d]", who, b, x, y, FR_MAX_REF, FR_MAX_REF);
        if (!call) continue;
        call[b].rx = x; call[b].ry = y;
        call[b].flags = !known || known[b] ? FRONTIER_KNOWN : 0;
        call[b].pad = 0;
    }
    return PP_OK;
}

void fill_config(FrontierParams& p, const pp_frontier_config& c) {
    p.free_max = c.free_max; p.conn = c.connectivity; p.min_size = c.min_size; p.max_frontiers = c.max_frontiers;
    p.rank = c.rank; p.use_field = c.use_field;
}

// a grid's overrun word -> PP_ERR_INTERNAL; info (may be NULL) [batch][PP_FRONTIER_INFO]
int unpack_info(pp_engine* e, const char* who, const std::vector<int>& state, int batch, int32_t* info) {
    for (int b = 0; b < batch; ++b) {
        const int* s = state.data() + (size_t)b * FR_INFO_WORDS;
        if (s[FR_OVERRUN])
            return fail(e, PP_ERR_INTERNAL, "%s: grid %d: a union-find loop passed the bound its cell count gives", who, b);
        if (info) memcpy(info + (size_t)b * PP_FRONTIER_INFO, s, PP_FRONTIER_INFO * sizeof(int32_t));
    }
    return PP_OK;
}

}  // namespace

void frontier_release(pp_engine* e) {
    for (pp_engine::Frontier& g : e->frontier) {
        g.mem.release();
        g.ring.release();
        g = pp_engine::Frontier();
    }
}

extern "C" {

int pp_set_frontier(pp_handle e, int32_t source, const pp_frontier_config* cfg) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_set_frontier";
    if (int st = check_source(e, who, source)) return st;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    pp_engine::Frontier& g = e->frontier[source];
    if (!cfg) { g.on = false; return PP_OK; }
    const pp_frontier_config c = *cfg;
    if (int st = check_config(e, who, c)) return st;
    (void)hipSetDevice(e->device);
    HIPCHK(e, hipStreamSynchronize(e->stream));
    HIPCHK(e, g.h_call.alloc(g.ring, (size_t)e->B));
    if (!g.d_call) {
        DevAlloc A{e};
        A(&g.info, (size_t)FR_INFO_WORDS * e->B); A(&g.words, (size_t)e->B * PP_FRONTIER_MAX * 8);
        A(&g.d_call, (size_t)e->B);                      // (d_call last: the ready flag)
        if (A.st) return A.st;
    }
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_frontier_config(pp_handle e, int32_t source, int32_t* on, pp_frontier_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    if (int st = check_source(e, "pp_get_frontier_config", source)) return st;
    *on = e->frontier[source].on ? 1 : 0;
    if (cfg_out) *cfg_out = e->frontier[source].cfg;
    return PP_OK;
}

int pp_frontier_async(pp_handle e, int32_t source, const int32_t* refs, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_frontier_async";
    if (int st = check_source(e, who, source)) return st;
    if (!refs) return fail(e, PP_ERR_ARG, "%s: refs is NULL", who);
    pp_engine::Frontier& g = e->frontier[source];
    const pp_engine::Inflation& in = e->infl[source];
    const pp_engine::Navfn& nav = e->navfn[source];
    const char* name = source_name(source);
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: the frontier stage of the %s source is not configured (pp_set_frontier first)", who, name);
    if (!in.on) return fail(e, PP_ERR_STATE, "%s: the inflation of the %s source is not configured (pp_set_inflation first)", who, name);
    if (int st = check_last_run(e, who, in.out ? in.batch : 0, batch, false, "no inflation has run on this source (pp_inflate_async first)",
                                "inflation", "grids")) return st;
    if (int st = fill_calls(e, who, nullptr, refs, batch, nullptr)) return st;
    if (g.cfg.use_field) {
        if (int st = check_last_run(e, who, nav.pot[0] ? nav.batch : 0, batch, false, "no navigation function has run on this source (pp_navfn_async first)",
                                    "navigation function", "grids")) return st;
        if (int st = check_navfn_run(e, who, source)) return st;
    }
    const int W = in.run_w, H = in.run_h;
    const size_t cells = (size_t)W * H;
    (void)hipSetDevice(e->device);
    if (W != g.w || H != g.h) {
        HIPCHK(e, hipStreamSynchronize(e->stream));      // a run in flight writes the old buffers to its end
        g.mem.release();
        g.w = 0; g.h = 0; g.batch = 0;
        StageMem& M = g.mem;
        M(&g.labels, (size_t)e->B * cells); M(&g.count, (size_t)e->B * cells); M(&g.roots, (size_t)e->B * cells);
        M(&g.sums, (size_t)e->B * cells * 2); M(&g.rep, (size_t)e->B * cells);
        if (hipError_t st = M.failed()) {
            (void)hipGetLastError();
            return fail(e, PP_ERR_HIP, "%s: %d grids x %zu cells need %zu bytes of device memory and the device cannot hold them (%s)",
                        who, e->B, cells, (size_t)e->B * cells * 36, hipGetErrorString(st));
        }
        g.w = W; g.h = H;
    }
    int slot;
    HIPCHK(e, g.ring.take(&slot));                       // behind the last check that can refuse
    (void)fill_calls(e, who, g.h_call.at(slot), refs, batch, in.known.data());
    FrontierParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = W; p.height = H; p.pitch = in.run_pitch; p.stride = in.cells;
    fill_config(p, g.cfg);
    p.grid = in.out; p.call = g.d_call;
    if (g.cfg.use_field) { p.pot = nav.run.pot[nav.rounds & 1]; p.pot_pitch = nav.run.pitch; p.pot_stride = nav.run.stride; }
    p.labels = g.labels; p.count = g.count; p.sums = g.sums; p.rep = g.rep; p.roots = g.roots;
    p.info = g.info; p.words = g.words;
    prof_reset(e);
    HIPCHK(e, g.h_call.send(slot, g.d_call, (size_t)batch, e->stream));
    HIPCHK(e, g.ring.sent(slot, e->stream));
    HIPCHK(e, hipMemsetAsync(g.info, 0, (size_t)batch * FR_INFO_WORDS * sizeof(int), e->stream));
    {
        ProfScope ps(e, nullptr);
        launch_frontier(p, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    g.batch = batch; g.run = p; g.nav_run = nav.run_id; g.nav_rounds = nav.rounds;
    return PP_OK;
}

int pp_get_frontiers(pp_handle e, int32_t source, int32_t* words, int32_t* info, uint32_t* labels, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const char* who = "pp_get_frontiers";
    if (int st = check_source(e, who, source)) return st;
    pp_engine::Frontier& g = e->frontier[source];
    if (int st = check_last_run(e, who, g.labels ? g.batch : 0, batch, false, "no frontier stage has run on this source (pp_frontier_async first)",
                                "run", "grids")) return st;
    (void)hipSetDevice(e->device);
    FrontierParams& p = g.run;
    if (p.use_field) {
        if (g.nav_run != e->navfn[source].run_id)
            return fail(e, PP_ERR_STATE, "%s: a pp_navfn_async of the %s source came after the last pp_frontier_async (pp_frontier_async again)",
                        who, source_name(source));
        pp_engine::Navfn* nav = nullptr;
        if (int st = settled_run(e, who, source, batch, &nav)) return st;
        if (nav->rounds != g.nav_rounds) {               // the field moved on behind the launches: rank again
            if (int st = check_navfn_run(e, who, source)) return st;
            p.pot = nav->run.pot[nav->rounds & 1];
            prof_reset(e);
            ProfScope ps(e, nullptr);
            launch_frontier_select(p, e->stream);
            HIPCHK(e, hipGetLastError());
            g.nav_rounds = nav->rounds;
        }
    }
    HIPCHK(e, hipStreamSynchronize(e->stream));
    std::vector<int> state((size_t)batch * FR_INFO_WORDS);
    HIPCHK(e, hipMemcpy(state.data(), p.info, state.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (int st = unpack_info(e, who, state, batch, info)) return st;
    if (words) HIPCHK(e, hipMemcpy(words, p.words, (size_t)batch * PP_FRONTIER_MAX * 8 * sizeof(int), hipMemcpyDeviceToHost));
    if (labels) HIPCHK(e, hipMemcpy(labels, p.labels, (size_t)batch * p.width * p.height * sizeof(unsigned), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_frontier_grids(int device, const int8_t* grids, const uint32_t* pot, int32_t batch, int32_t height, int32_t width,
                      const pp_frontier_config* cfg, const int32_t* refs, int32_t* words, int32_t* info, uint32_t* labels) {
    const char* who = "pp_frontier_grids";
    if (!grids || !cfg || !refs) return fail(nullptr, PP_ERR_ARG, "%s: grids, cfg or refs is NULL", who);
    if (batch < 1 || batch > 65535) return fail(nullptr, PP_ERR_ARG, "%s: batch = %d outside [1, 65535]", who, batch);
    if (int st = check_cfg_window(nullptr, who, width, height, PP_OCC_MAX_CELLS, "PP_OCC_MAX_CELLS")) return st;
    if (int st = check_config(nullptr, who, *cfg)) return st;
    if (cfg->use_field && !pot) return fail(nullptr, PP_ERR_ARG, "%s: use_field = 1 and pot is NULL", who);
    std::vector<FrontierCall> calls((size_t)batch);
    if (int st = fill_calls(nullptr, who, calls.data(), refs, batch, nullptr)) return st;
    if (int st = check_device(who, device)) return st;
    DEVCHK(hipSetDevice(device));
    const size_t cells = (size_t)width * height, n = (size_t)batch * cells;
    DevBuf d_in, d_pot, d_call, d_labels, d_count, d_roots, d_sums, d_rep, d_info, d_words;
    DEVCHK(d_in.alloc(n));
    if (cfg->use_field) DEVCHK(d_pot.alloc(n * sizeof(unsigned)));
    DEVCHK(d_call.alloc((size_t)batch * sizeof(FrontierCall)));
    DEVCHK(d_labels.alloc(n * sizeof(unsigned)));
    DEVCHK(d_count.alloc(n * sizeof(unsigned)));
    DEVCHK(d_roots.alloc(n * sizeof(unsigned)));
    DEVCHK(d_sums.alloc(n * 2 * sizeof(unsigned long long)));
    DEVCHK(d_rep.alloc(n * sizeof(unsigned long long)));
    DEVCHK(d_info.alloc((size_t)batch * FR_INFO_WORDS * sizeof(int)));
    DEVCHK(d_words.alloc((size_t)batch * PP_FRONTIER_MAX * 8 * sizeof(int)));
    DEVCHK(hipMemcpy(d_in.p, grids, n, hipMemcpyHostToDevice));
    if (cfg->use_field) DEVCHK(hipMemcpy(d_pot.p, pot, n * sizeof(unsigned), hipMemcpyHostToDevice));
    DEVCHK(hipMemcpy(d_call.p, calls.data(), (size_t)batch * sizeof(FrontierCall), hipMemcpyHostToDevice));
    DEVCHK(hipMemset(d_info.p, 0, (size_t)batch * FR_INFO_WORDS * sizeof(int)));
    FrontierParams p;
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.width = width; p.height = height; p.pitch = width; p.stride = cells;
    fill_config(p, *cfg);
    p.grid = (const int8_t*)d_in.p; p.call = (const FrontierCall*)d_call.p;
    p.pot = (const unsigned*)d_pot.p; p.pot_pitch = width; p.pot_stride = cells;
    p.labels = (unsigned*)d_labels.p; p.count = (unsigned*)d_count.p; p.roots = (unsigned*)d_roots.p;
    p.sums = (unsigned long long*)d_sums.p; p.rep = (unsigned long long*)d_rep.p;
    p.info = (int*)d_info.p; p.words = (int*)d_words.p;
    launch_frontier(p, nullptr);
    DEVCHK(hipGetLastError());
    DEVCHK(hipDeviceSynchronize());
    std::vector<int> state((size_t)batch * FR_INFO_WORDS);
    DEVCHK(hipMemcpy(state.data(), d_info.p, state.size() * sizeof(int), hipMemcpyDeviceToHost));
    if (int st = unpack_info(nullptr, who, state, batch, info)) return st;
    if (words) DEVCHK(hipMemcpy(words, d_words.p, (size_t)batch * PP_FRONTIER_MAX * 8 * sizeof(int), hipMemcpyDeviceToHost));
    if (labels) DEVCHK(hipMemcpy(labels, d_labels.p, n * sizeof(unsigned), hipMemcpyDeviceToHost));
    return PP_OK;
}

}  // extern "C"
