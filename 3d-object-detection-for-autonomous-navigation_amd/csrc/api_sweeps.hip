// C-ABI, multi-sweep accumulation (pp_set_sweeps, pp_sweeps_accumulate*): the resident frames -> the resident frames plus
// their streams' stored sweeps under the ego poses, written into the handle's other input buffer, which becomes the
// resident one (kernels: sweeps.hip; the rule: sweeps.py).  One ring of history + 1 slots per stream lives on the device.
#include "pp_engine.h"

static_assert(sizeof(pp_sweep_config) == 24, "pp_sweep_config: a double, 4 int32 (the Python binding mirrors it)");
static_assert(sizeof(SweepChunk) == 32 && sizeof(SweepXf) == 104, "sweeps.hip reads these through scalar loads");

namespace {

void free_ring(pp_engine* e) {
    e->swp.mem.release();
    e->swp.chunk_cap = e->swp.cfg.history = 0;
}

// forgets the history of streams b0 .. b0 + nb - 1 (the device is idle)
int forget(pp_engine* e, size_t b0, size_t nb) {
    pp_engine::Sweeps& g = e->swp;
    const size_t slots = (size_t)g.cfg.history + 1;
    HIPCHK(e, hipMemset(g.slot_valid + b0 * slots, 0, nb * slots * sizeof(int)));
    HIPCHK(e, hipMemset(g.slot_cnt + b0 * slots, 0, nb * slots * sizeof(int)));
    HIPCHK(e, hipMemset(g.head + b0, 0, nb * sizeof(int)));
    for (size_t b = b0; b < b0 + nb; ++b) { g.last_stamp[b] = NAN; g.stored[b] = 0; }
    return PP_OK;
}

// The ring and the tables of configuration c (capacity filled in): max_batch streams.
int make_ring(pp_engine* e, const pp_sweep_config& c) {
    pp_engine::Sweeps& g = e->swp;
    const size_t B = (size_t)e->B, slots = (size_t)c.history + 1, H = (size_t)c.history;
    const size_t ring_floats = B * slots * (size_t)c.capacity * e->F;
    // chunks of a frame at most: its own rows, every used sweep, the push
    const size_t per_frame = (size_t)sweep_chunks(e->NMAX) + (H + 1) * sweep_chunks(c.capacity);
    const size_t cap = B * per_frame;
    if (cap > (size_t)INT32_MAX)
        return fail(e, PP_ERR_ARG, "pp_set_sweeps: history %d x capacity %d on %d streams needs %zu chunk records", c.history, c.capacity, e->B, cap);
    StageMem& M = g.mem;
    M(&g.ring, ring_floats);
    M(&g.slot_cnt, B * slots); M(&g.slot_valid, B * slots); M(&g.head, B);
    M(&g.slot_pose, B * slots * 12); M(&g.slot_stamp, B * slots);
    M(&g.xf, B * H); M(&g.segs, B * (H + 2)); M(&g.seg_chunk0, B * (H + 2)); M(&g.frame_chunks, B + 1);
    M(&g.chunks, cap); M(&g.nchunks, 1);
    M(&g.info, 4 * B); M(&g.d_call, B * 13);
    if (hipError_t st = M.failed()) {
        (void)hipGetLastError();
        return fail(e, PP_ERR_HIP, "pp_set_sweeps: the ring of %d streams x %d slots x capacity %d rows x %d floats needs %zu bytes "
                    "of device memory and the device cannot hold it (%s): lower history or capacity, or raise history_decimate",
                    e->B, (int)slots, c.capacity, e->F, ring_floats * sizeof(float), hipGetErrorString(st));
    }
    g.chunk_cap = (int)cap;
    g.cfg = c;
    g.last_stamp.assign(B, NAN);
    g.stored.assign(B, 0);
    HIPCHK(e, hipMemset(g.slot_pose, 0, B * slots * 12 * sizeof(double)));
    HIPCHK(e, hipMemset(g.slot_stamp, 0, B * slots * sizeof(double)));
    HIPCHK(e, hipMemset(g.info, 0, 4 * B * sizeof(int)));
    return forget(e, 0, B);
}

// Everything pp_sweeps_accumulate* refuses, before anything is queued.
int check_sweeps(pp_engine* e, const char* who, const double* poses, const double* stamps, int batch) {
    const pp_engine::Sweeps& g = e->swp;
    if (!g.on) return fail(e, PP_ERR_STATE, "%s: sweeps are not configured (pp_set_sweeps first)", who);
    if (!poses) return fail(e, PP_ERR_ARG, "%s: poses is NULL", who);
    if (!stamps) return fail(e, PP_ERR_ARG, "%s: stamps is NULL", who);
    if (int st = check_resident_call(e, who, batch, "upload or ingest frames first")) return st;
    return check_poses(e, who, poses, stamps, batch, [&](int b, const double*) {
        const double last = g.last_stamp[(size_t)b];
        if (!std::isnan(last) && !(stamps[b] > last))
            return fail(e, PP_ERR_ARG, "%s: stamps: the stamp of stream %d does not increase (%.17g after %.17g)", who, b, stamps[b], last);
        return (int)PP_OK;
    });
}

// Queues poses and stamps -> device and the two kernels on `stream` along the rewrite path (pp_engine.h): the resident
// frames' sizes are read on the device, the host then knows bounds only.
int enqueue_sweeps(pp_engine* e, const double* poses, const double* stamps, int batch, hipStream_t stream) {
    pp_engine::Sweeps& g = e->swp;
    const pp_sweep_config& c = g.cfg;
    int slot;
    HIPCHK(e, e->ring.take(&slot));
    double* ring = g.h_ring.at(slot);
    for (int b = 0; b < batch; ++b) {
        memcpy(ring + (size_t)b * 13, poses + (size_t)b * 12, 12 * sizeof(double));
        ring[(size_t)b * 13 + 12] = stamps[b];
    }
    int st;
    Rewrite w;
    if ((st = rewrite_begin(e, batch, stream, &w))) return st;
    // the host's bounds: rows of an output frame, chunks of the move launch
    std::vector<int> bound((size_t)batch + 1, 0);
    int max_n = 0;
    long long chunk_bound = 0;
    for (int b = 0; b < batch; ++b) {
        const int n_in = w.bound[(size_t)b + 1] - w.bound[(size_t)b];
        const long long full = (long long)n_in + (long long)g.stored[(size_t)b] * c.capacity;
        const int n_out = (int)std::min<long long>(full, e->NMAX);
        const int n_push = std::min((n_in + c.history_decimate - 1) / c.history_decimate, c.capacity);
        bound[(size_t)b + 1] = bound[(size_t)b] + n_out;
        max_n = std::max(max_n, n_out);
        chunk_bound += sweep_chunks(n_in) + (long long)g.stored[(size_t)b] * sweep_chunks(c.capacity) + sweep_chunks(n_push);
    }
    w.bound.swap(bound);
    w.max_n = max_n;
    HIPCHK(e, g.h_ring.send(slot, g.d_call, (size_t)batch * 13, stream));
    HIPCHK(e, e->ring.sent(slot, stream));
    SweepParams p;
    memset(&p, 0, sizeof(p));
    p.in = w.src; p.offsets_in = w.offsets_in;
    p.out = e->d_points; p.offsets_out = e->d_offsets;
    p.batch = batch; p.F = e->F; p.nmax = e->NMAX;
    p.history = c.history; p.capacity = c.capacity; p.decimate = c.history_decimate; p.time_feature = c.time_feature;
    p.max_age = c.max_age;
    p.call = g.d_call;
    p.ring = g.ring; p.slot_cnt = g.slot_cnt; p.slot_valid = g.slot_valid; p.slot_pose = g.slot_pose;
    p.slot_stamp = g.slot_stamp; p.head = g.head;
    p.xf = g.xf; p.segs = g.segs; p.seg_chunk0 = g.seg_chunk0; p.frame_chunks = g.frame_chunks;
    p.chunks = g.chunks; p.nchunks = g.nchunks; p.chunk_cap = g.chunk_cap;
    p.chunk_bound = (int)std::min<long long>(chunk_bound, g.chunk_cap);
    p.count = g.info; p.used = g.info + e->B; p.truncated = g.info + 2 * (size_t)e->B; p.push_truncated = g.info + 3 * (size_t)e->B;
    {
        ProfScope ps(e, nullptr);
        launch_sweeps(p, stream);
    }
    if ((st = rewrite_end(e, batch, w, stream))) return st;
    for (int b = 0; b < batch; ++b) {
        g.last_stamp[(size_t)b] = stamps[b];
        g.stored[(size_t)b] = std::min(g.stored[(size_t)b] + 1, c.history);
    }
    g.batch = batch;
    return PP_OK;
}

}  // namespace

void sweeps_release(pp_engine* e) {
    free_ring(e);
    e->swp = pp_engine::Sweeps();
}

extern "C" {

int pp_set_sweeps(pp_handle e, const pp_sweep_config* cfg) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_sweeps: a training step is in flight");
    pp_engine::Sweeps& g = e->swp;
    if (!cfg) { g.on = false; return PP_OK; }
    pp_sweep_config c = *cfg;
    if (c.history < 1 || c.history > PP_SWEEP_MAX)
        return fail(e, PP_ERR_ARG, "pp_set_sweeps: history = %d outside [1, PP_SWEEP_MAX = %d]", c.history, PP_SWEEP_MAX);
    if (c.capacity < 0) return fail(e, PP_ERR_ARG, "pp_set_sweeps: capacity = %d must be >= 1 (0: max_points_per_frame)", c.capacity);
    if (c.capacity == 0) c.capacity = e->NMAX;
    if (c.history_decimate < 1) return fail(e, PP_ERR_ARG, "pp_set_sweeps: history_decimate = %d must be >= 1", c.history_decimate);
    if (!std::isfinite(c.max_age) || !(c.max_age > 0.0))
        return fail(e, PP_ERR_ARG, "pp_set_sweeps: max_age = %g must be finite and > 0", c.max_age);
    if (c.time_feature != -1 && (c.time_feature < 3 || c.time_feature >= e->F))
        return fail(e, PP_ERR_ARG, "pp_set_sweeps: time_feature = %d with num_point_features = %d (-1%s)", c.time_feature, e->F,
                    e->F > 3 ? ", or a column from 3 to num_point_features - 1" : ": a 3-feature model has no spare column");
    if (e->F > crop_max_features())
        return fail(e, PP_ERR_UNSUPPORTED, "pp_set_sweeps: num_point_features is %d, rows of up to %d are moved", e->F, crop_max_features());
    (void)hipSetDevice(e->device);
    HIPCHK(e, g.h_ring.alloc(e->ring, (size_t)e->B * 13));
    if (g.cfg.history != c.history || g.cfg.capacity != c.capacity) {
        if (int st = quiesce(e)) return st;
        g.on = false;
        free_ring(e);
        if (int st = make_ring(e, c)) return st;
    }
    g.cfg = c;
    g.on = true;
    return PP_OK;
}

int pp_get_sweeps(pp_handle e, int32_t* on, pp_sweep_config* cfg_out) {
    if (!e || !on) return PP_ERR_ARG;
    *on = e->swp.on ? 1 : 0;
    if (cfg_out) *cfg_out = e->swp.cfg;
    return PP_OK;
}

int pp_sweeps_accumulate(pp_handle e, const double* poses, const double* stamps, int32_t batch, int32_t* counts_out,
                         float* points_out, int64_t points_capacity) {
    if (!e) return PP_ERR_ARG;
    if (!counts_out) return fail(e, PP_ERR_ARG, "pp_sweeps_accumulate: counts_out is NULL");
    int st = check_sweeps(e, "pp_sweeps_accumulate", poses, stamps, batch);
    if (st) return st;
    if ((st = rewrite_run(e, batch, false, [&](hipStream_t s) { return enqueue_sweeps(e, poses, stamps, batch, s); }))) return st;
    return rewrite_sync_tail(e, "pp_sweeps_accumulate", "%s: frame %d: the device wrote %d rows, the host's bound is %d",
                             "%s: points_out holds %lld points, the frames have %d", e->swp.info, batch, counts_out, points_out, points_capacity);
}

int pp_sweeps_accumulate_async(pp_handle e, const double* poses, const double* stamps, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (int st = check_sweeps(e, "pp_sweeps_accumulate_async", poses, stamps, batch)) return st;
    return rewrite_run(e, batch, true, [&](hipStream_t s) { return enqueue_sweeps(e, poses, stamps, batch, s); });
}

int pp_sweeps_info(pp_handle e, int32_t* counts, int32_t* used, int32_t* truncated, int32_t* push_truncated, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    const pp_engine::Sweeps& g = e->swp;
    if (int st = check_last_run(e, "pp_sweeps_info", g.info ? g.batch : 0, batch, false, "no accumulate has run", "call", "frames")) return st;
    (void)hipSetDevice(e->device);
    if (int st = quiesce(e)) return st;
    int32_t* outs[4] = {counts, used, truncated, push_truncated};
    for (int k = 0; k < 4; ++k)
        if (outs[k]) HIPCHK(e, hipMemcpy(outs[k], g.info + (size_t)k * e->B, (size_t)batch * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

int pp_sweeps_reset(pp_handle e, int32_t stream) {
    if (!e) return PP_ERR_ARG;
    if (stream < -1 || stream >= e->B)
        return fail(e, PP_ERR_ARG, "pp_sweeps_reset: stream %d outside [0, max_batch=%d) (-1: all)", stream, e->B);
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_sweeps_reset: a training step is in flight");
    if (!e->swp.ring) return PP_OK;
    (void)hipSetDevice(e->device);
    if (int st = quiesce(e)) return st;
    return stream < 0 ? forget(e, 0, (size_t)e->B) : forget(e, (size_t)stream, 1);
}

}  // extern "C"
