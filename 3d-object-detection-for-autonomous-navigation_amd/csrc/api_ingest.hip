// C-ABI, live-camera ingest (pp_ingest_*): PointCloud2 messages or raw depth images (kernels: ingest.hip) -> the resident
// points and offsets.  Every exported call is one argument record handed to ingest_call: the two feeds differ in what
// check_one refuses and fills (their layouts and frame records); the checks around it, the staging, the input-buffer flip
// and the ordering are one path (check_call, enqueue_ingest).  A rig call (pp_ingest_rig_*) takes the same path with one
// record per SOURCE and the sources' own selections and transforms in a table beside them.  The
// pp_ingest_*pointcloud2_fields* calls add a table of feature columns, one row per frame or source, which travels as the
// frame records do.
#include "pp_engine.h"

namespace {

template <typename Frame>
struct IngestPlanT {
    std::vector<Frame> frames;
    std::vector<int> bound_off;    // [batch + 1] prefix sums of the frames' kept bounds
    int max_bound = 0, stride = 0;
    int64_t bytes = 0;             // byte_offsets[records] - byte_offsets[0]
    std::vector<RigSource> rig;    // a rig call: one entry per source, `frames` then holds the SOURCES' records; else empty
    std::vector<IngFeat> feats;    // a _fields call: [frames or sources][nfeat]; else empty
    int nfeat = 0;
};
template <typename Layout> struct FrameOf;
template <> struct FrameOf<pp_pc2_layout> { typedef IngFrame type; };
template <> struct FrameOf<pp_depth_layout> { typedef DepthFrame type; };

// What an exported call was given.  A plain call: one configuration, source_frame NULL, sources 0; one without ING_FIELDS:
// features NULL and nfeat 0, neither looked at; an asynchronous one: no tap.
enum { ING_RIG = 1, ING_FIELDS = 2, ING_ASYNC = 4 };
template <typename Layout>
struct IngestArgs {
    const uint8_t* data;
    const int64_t* bo;             // [records + 1] byte offsets; records: frames, or the sources of a rig call
    const Layout* L;               // [records]
    const pp_ingest_config* cfgs;  // one, or [sources]
    const int32_t* source_frame;   // [sources]
    int sources, batch;
    const pp_pc2_feature* features;
    int nfeat;
    float* points_out;             // the parity tap and the points it holds
    int64_t points_out_capacity;
    int kind;                      // ING_RIG | ING_FIELDS | ING_ASYNC
};

// `at`: "" for the one configuration of a plain call, "source 3: " for a rig's
int check_selection(pp_engine* e, const char* who, const char* at, const pp_ingest_config* c) {
    if (c->decimate < 1) return fail(e, PP_ERR_ARG, "%s: %sdecimate %d < 1", who, at, c->decimate);
    if (c->first < 0) return fail(e, PP_ERR_ARG, "%s: %sfirst %d < 0", who, at, c->first);
    return PP_OK;
}

inline int64_t kept_bound(int64_t n, const pp_ingest_config* c) {
    return n > c->first ? (n - c->first + c->decimate - 1) / c->decimate : 0;
}

// What is refused about one message (`at`: "frame 1" or "source 3"; its bytes are data[bo[i] .. bo[i + 1])); fills its
// record and the bound on the points it keeps under `c`.
int check_one(pp_engine* e, const char* who, const char* at, const int64_t* bo, int i, const pp_pc2_layout& l,
              const pp_ingest_config* c, IngFrame* f, int64_t* bound) {
    if (l.width < 0 || l.height < 0 || l.point_step < 1 || l.row_step < 0)
        return fail(e, PP_ERR_ARG, "%s: %s: width %d, height %d, point_step %d, row_step %d", who, at, l.width,
                    l.height, l.point_step, l.row_step);
    const int64_t n_rec = (int64_t)l.width * l.height;
    if (n_rec > (1ll << 30)) return fail(e, PP_ERR_ARG, "%s: %s: width %d x height %d records", who, at, l.width, l.height);
    if (l.datatype >> 8)
        return fail(e, PP_ERR_UNSUPPORTED, "%s: %s: datatype: x, y and z differ (%d, %d, %d)", who, at,
                    l.datatype & 255, (l.datatype >> 8) & 255, (l.datatype >> 16) & 255);
    if (l.datatype >= 1 && l.datatype <= 6)
        return fail(e, PP_ERR_UNSUPPORTED, "%s: %s: datatype %d is an integer type (7 FLOAT32 or 8 FLOAT64)", who, at, l.datatype);
    if (l.datatype != 7 && l.datatype != 8)
        return fail(e, PP_ERR_ARG, "%s: %s: unknown datatype %d", who, at, l.datatype);
    const int size = l.datatype == 8 ? 8 : 4;
    const int offs[3] = {l.x_offset, l.y_offset, l.z_offset};
    static const char* const names[3] = {"x_offset", "y_offset", "z_offset"};
    for (int k = 0; k < 3; ++k)
        if (offs[k] < 0 || (int64_t)offs[k] + size > l.point_step)
            return fail(e, PP_ERR_ARG, "%s: %s: %s %d (%d bytes) does not fit point_step %d", who, at, names[k], offs[k],
                        size, l.point_step);
    if ((int64_t)l.row_step < (int64_t)l.width * l.point_step)
        return fail(e, PP_ERR_ARG, "%s: %s: row_step %d < width %d x point_step %d", who, at, l.row_step, l.width, l.point_step);
    const int64_t need = (int64_t)l.height * l.row_step;
    if (bo[i] < 0 || bo[i + 1] < bo[i] || bo[i + 1] - bo[i] < need)
        return fail(e, PP_ERR_ARG, "%s: %s: byte_offsets give it %lld bytes, height %d x row_step %d = %lld needed", who, at,
                    (long long)(bo[i + 1] - bo[i]), l.height, l.row_step, (long long)need);
    *bound = kept_bound(n_rec, c);
    f->byte_off = bo[i] - bo[0];
    f->n_rec = (int)n_rec;
    const bool tight = l.row_step == l.width * l.point_step || l.height <= 1;
    f->width = tight ? (int)n_rec : l.width;
    f->point_step = l.point_step; f->row_step = l.row_step;
    f->x_off = l.x_offset; f->y_off = l.y_offset; f->z_off = l.z_offset;
    f->f64 = l.datatype == 8; f->big_endian = l.is_bigendian != 0;
    f->nchunks = ingest_chunks(f->n_rec);
    return PP_OK;
}

// What is refused about the feature columns of one message (`at` as above); fills their records.
int check_features_one(pp_engine* e, const char* who, const char* at, const pp_pc2_layout& l, const pp_pc2_feature* ft,
                       int nfeat, IngFeat* out) {
    static const int sizes[9] = {0, 1, 1, 2, 2, 4, 4, 4, 8};
    for (int j = 0; j < nfeat; ++j) {
        const pp_pc2_feature& t = ft[j];
        if (t.datatype < 0 || t.datatype > 8)
            return fail(e, PP_ERR_ARG, "%s: %s: feature %d: unknown datatype %d (0 constant, 1 INT8 ... 8 FLOAT64)", who, at, j,
                        t.datatype);
        const int size = sizes[t.datatype];
        if (t.datatype != 0 && (t.offset < 0 || (int64_t)t.offset + size > l.point_step))
            return fail(e, PP_ERR_ARG, "%s: %s: feature %d: offset %d (%d bytes) does not fit point_step %d", who, at, j, t.offset,
                        size, l.point_step);
        if (!std::isfinite(t.scale)) return fail(e, PP_ERR_ARG, "%s: %s: feature %d: scale %g is not finite", who, at, j, t.scale);
        if (!std::isfinite(t.bias)) return fail(e, PP_ERR_ARG, "%s: %s: feature %d: bias %g is not finite", who, at, j, t.bias);
        out[j].off = t.datatype ? t.offset : 0; out[j].type = t.datatype; out[j].scale = t.scale; out[j].bias = t.bias;
    }
    return PP_OK;
}
inline int check_features_one(pp_engine*, const char*, const char*, const pp_depth_layout&, const pp_pc2_feature*, int, IngFeat*) {
    return PP_OK;                                  // (an image has no field)
}

// The same for one depth image.
int check_one(pp_engine* e, const char* who, const char* at, const int64_t* bo, int i, const pp_depth_layout& l,
              const pp_ingest_config* c, DepthFrame* f, int64_t* bound) {
    if (l.width < 0 || l.height < 0 || l.row_step < 0)
        return fail(e, PP_ERR_ARG, "%s: %s: width %d, height %d, row_step %d", who, at, l.width, l.height, l.row_step);
    const int64_t n_pix = (int64_t)l.width * l.height;
    if (n_pix > (1ll << 30)) return fail(e, PP_ERR_ARG, "%s: %s: width %d x height %d pixels", who, at, l.width, l.height);
    if (l.encoding != PP_DEPTH_U16 && l.encoding != PP_DEPTH_F32)
        return fail(e, PP_ERR_ARG, "%s: %s: unknown encoding %d (PP_DEPTH_U16 %d or PP_DEPTH_F32 %d)", who, at, l.encoding,
                    (int)PP_DEPTH_U16, (int)PP_DEPTH_F32);
    const int size = l.encoding == PP_DEPTH_F32 ? 4 : 2;
    if ((int64_t)l.row_step < (int64_t)l.width * size)
        return fail(e, PP_ERR_ARG, "%s: %s: row_step %d < width %d x %d bytes", who, at, l.row_step, l.width, size);
    const int64_t need = (int64_t)l.height * l.row_step;
    if (bo[i] < 0 || bo[i + 1] < bo[i] || bo[i + 1] - bo[i] < need)
        return fail(e, PP_ERR_ARG, "%s: %s: byte_offsets give it %lld bytes, height %d x row_step %d = %lld needed", who, at,
                    (long long)(bo[i + 1] - bo[i]), l.height, l.row_step, (long long)need);
    const float focal[2] = {l.fx, l.fy}, centre[2] = {l.ppx, l.ppy};
    static const char* const fnames[2] = {"fx", "fy"};
    static const char* const cnames[2] = {"ppx", "ppy"};
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(focal[k]) || focal[k] == 0.0f)
            return fail(e, PP_ERR_ARG, "%s: %s: %s %g is not a finite non-zero focal length", who, at, fnames[k], (double)focal[k]);
        if (!std::isfinite(centre[k]))
            return fail(e, PP_ERR_ARG, "%s: %s: %s %g is not finite", who, at, cnames[k], (double)centre[k]);
    }
    if (l.encoding == PP_DEPTH_U16 && !(std::isfinite(l.depth_scale) && l.depth_scale > 0.0f))
        return fail(e, PP_ERR_ARG, "%s: %s: depth_scale %g is not a finite positive number", who, at, (double)l.depth_scale);
    if (!(l.z_min <= l.z_max))
        return fail(e, PP_ERR_ARG, "%s: %s: z_min %g > z_max %g (or one is NaN)", who, at, (double)l.z_min, (double)l.z_max);
    *bound = kept_bound(n_pix, c);
    f->byte_off = bo[i] - bo[0];
    f->width = l.width; f->n_pix = (int)n_pix; f->row_step = l.row_step;
    f->tight = l.row_step == l.width * size || l.height <= 1;
    f->f32 = l.encoding == PP_DEPTH_F32; f->big_endian = l.is_bigendian != 0;
    f->nchunks = ingest_chunks(f->n_pix);
    f->fx = l.fx; f->fy = l.fy; f->ppx = l.ppx; f->ppy = l.ppy;
    f->depth_scale = l.depth_scale; f->z_min = l.z_min; f->z_max = l.z_max;
    return PP_OK;
}

// Everything a pp_ingest_* call refuses, before anything is queued: what every call refuses before it looks at a record;
// a rig's frame map; per record (frame, or source) its selection, its layout, its feature columns and the bound of its
// frame; fills the plan.
template <typename Layout, typename Frame>
int check_call(pp_engine* e, const char* who, const IngestArgs<Layout>& a, IngestPlanT<Frame>* plan) {
    const bool rig = (a.kind & ING_RIG) != 0;
    const bool fields = (a.kind & ING_FIELDS) != 0;             // else: a call that delivers x y z only
    const int nfeat = fields ? a.nfeat : 0;
    const int batch = a.batch, records = rig ? a.sources : a.batch;
    const int64_t* bo = a.bo;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "%s: a training step is in flight", who);
    if (!fields) {
        if (e->F != 3)
            return fail(e, PP_ERR_UNSUPPORTED, "%s: num_point_features is %d, the live path delivers x y z only (3)", who, e->F);
    } else {
        if (nfeat > 0 && !a.features) return fail(e, PP_ERR_ARG, "%s: features is NULL, nfeat is %d", who, nfeat);
        if (nfeat != e->F - 3)
            return fail(e, PP_ERR_ARG, "%s: nfeat %d, num_point_features is %d: x y z and %d feature column(s) expected", who,
                        nfeat, e->F, e->F - 3);
    }
    if (!bo || !a.L || !a.cfgs) return fail(e, PP_ERR_ARG, "%s: null argument", who);
    int st = check_batch(e, batch); if (st) return st;
    if (!rig) {
        if ((st = check_selection(e, who, "", a.cfgs))) return st;
    } else {
        const int32_t* source_frame = a.source_frame;
        const int sources = a.sources;
        if (!source_frame) return fail(e, PP_ERR_ARG, "%s: null argument", who);
        if (sources < 1) return fail(e, PP_ERR_ARG, "%s: sources %d < 1", who, sources);
        if (source_frame[0] != 0)
            return fail(e, PP_ERR_ARG, "%s: source 0: source_frame %d, the frame map starts at frame 0", who, source_frame[0]);
        for (int s = 1, run = 1; s < sources; ++s) {
            const int prev = source_frame[s - 1], cur = source_frame[s];
            if (cur < prev)
                return fail(e, PP_ERR_ARG, "%s: source %d: source_frame %d < %d of the source before it (the frame map never decreases)",
                            who, s, cur, prev);
            if (cur > prev + 1)
                return fail(e, PP_ERR_ARG, "%s: source %d: source_frame %d skips frame %d (every frame has at least one source)", who, s,
                            cur, prev + 1);
            run = cur == prev ? run + 1 : 1;
            if (run > PP_RIG_MAX_SOURCES)
                return fail(e, PP_ERR_ARG, "%s: source %d: frame %d has more than PP_RIG_MAX_SOURCES=%d sources", who, s, cur,
                            PP_RIG_MAX_SOURCES);
        }
        if (source_frame[sources - 1] != batch - 1)
            return fail(e, PP_ERR_ARG, "%s: source %d: source_frame %d, the frame map ends at frame batch - 1 = %d", who, sources - 1,
                        source_frame[sources - 1], batch - 1);
    }
    plan->nfeat = nfeat;
    plan->feats.assign((size_t)records * plan->nfeat, IngFeat());
    plan->frames.assign((size_t)records, Frame());
    plan->rig.assign(rig ? (size_t)records : 0, RigSource());
    plan->bound_off.assign((size_t)batch + 1, 0);
    std::vector<int64_t> sum((size_t)batch, 0);         // the frames' bounds: a rig's frame sums its sources'
    for (int i = 0; i < records; ++i) {
        const pp_ingest_config* c = rig ? a.cfgs + i : a.cfgs;
        char at[32];
        if (rig) {
            snprintf(at, sizeof(at), "source %d: ", i);
            if ((st = check_selection(e, who, at, c))) return st;
        }
        snprintf(at, sizeof(at), rig ? "source %d" : "frame %d", i);
        int64_t bound = 0;
        Frame& f = plan->frames[(size_t)i];
        if ((st = check_one(e, who, at, bo, i, a.L[i], c, &f, &bound))) return st;
        if (plan->nfeat && (st = check_features_one(e, who, at, a.L[i], a.features + (size_t)i * nfeat, nfeat,
                                                    plan->feats.data() + (size_t)i * nfeat))) return st;
        const int b = rig ? a.source_frame[i] : i;
        sum[(size_t)b] += bound;
        if (sum[(size_t)b] > e->NMAX) {
            if (!rig)
                return fail(e, PP_ERR_ARG, "%s: frame %d: width %d x height %d keeps up to %lld points > max_points_per_frame=%d", who, b,
                            a.L[i].width, a.L[i].height, (long long)bound, e->NMAX);
            return fail(e, PP_ERR_ARG, "%s: source %d: frame %d keeps up to %lld points with it (width %d x height %d: %lld) > "
                        "max_points_per_frame=%d", who, i, b, (long long)sum[(size_t)b], a.L[i].width, a.L[i].height, (long long)bound,
                        e->NMAX);
        }
        if (rig) {
            RigSource& g = plan->rig[(size_t)i];
            g.frame = b; g.first = c->first; g.decimate = c->decimate; g.reserved = 0;
            memcpy(g.r, c->r, sizeof(g.r)); memcpy(g.r2, c->r2, sizeof(g.r2)); memcpy(g.lift, c->lift, sizeof(g.lift));
        }
        plan->stride = std::max(plan->stride, f.nchunks);
    }
    for (int b = 0; b < batch; ++b) {
        plan->max_bound = std::max(plan->max_bound, (int)sum[(size_t)b]);
        plan->bound_off[(size_t)b + 1] = plan->bound_off[(size_t)b] + (int)sum[(size_t)b];
    }
    plan->bytes = bo[records] - bo[0];
    if (plan->bytes > 0 && !a.data) return fail(e, PP_ERR_ARG, "%s: data is NULL", who);
    return PP_OK;
}

int ensure_ing(pp_engine* e) {
    pp_engine::Ing& g = e->ing;
    if (g.frames) return PP_OK;
    const size_t nf = (size_t)std::max(e->F - 3, 1);
    HIPCHK(e, g.h_ring.alloc(e->ring, (size_t)e->B));
    HIPCHK(e, g.h_feats.alloc(e->ring, (size_t)e->B * nf));
    DevAlloc A{e};
    A(&g.feats, (size_t)e->B * nf);
    A(&g.finite, (size_t)e->B); A(&g.kept, (size_t)e->B); A(&g.frames, (size_t)e->B);     // (frames last: the ready flag)
    return A.st;
}

// the per-source tables of a rig call, for the most sources a call can have
int ensure_rig(pp_engine* e) {
    pp_engine::Ing::Rig& r = e->ing.rig;
    if (r.frames) return PP_OK;
    const size_t cap = (size_t)PP_RIG_MAX_SOURCES * e->B;
    const size_t nf = (size_t)std::max(e->F - 3, 1);
    HIPCHK(e, r.h_frames.alloc(e->ring, cap));
    HIPCHK(e, r.h_src.alloc(e->ring, cap));
    HIPCHK(e, r.h_feats.alloc(e->ring, cap * nf));
    r.sources_cap = (int)cap;
    DevAlloc A{e};
    A(&r.feats, cap * nf);
    A(&r.src, cap); A(&r.finite, cap); A(&r.kept, cap); A(&r.out_base, cap); A(&r.frames, cap);     // (frames last: the ready flag)
    return A.st;
}

// Flips to the other input buffer (as set_offsets does) and queues bytes -> staging -> points + offsets on `stream`
// (the main stream, or the copy stream: it first waits for the pass that last read that buffer).  A plain call has one
// record per frame and one configuration `c`; a rig call (plan.rig not empty) one record and one RigSource per source, in
// the rig's own tables.
template <typename Frame>
int enqueue_ingest(pp_engine* e, const uint8_t* data, const int64_t* bo, int batch, const pp_ingest_config* c,
                   const IngestPlanT<Frame>& plan, hipStream_t stream) {
    int st;
    const bool rig = !plan.rig.empty();
    const int records = (int)plan.frames.size();          // frames, or sources
    if ((st = ensure_ing(e))) return st;
    if (rig && (st = ensure_rig(e))) return st;
    if (rig && records > e->ing.rig.sources_cap)
        return fail(e, PP_ERR_ARG, "%d sources, the handle holds %d", records, e->ing.rig.sources_cap);
    const size_t tables = 2 * (size_t)records * plan.stride;
    if ((size_t)plan.bytes > e->ing.cap_raw || tables > e->ing.cap_chunks) {
        // an ingest queued earlier on the copy stream may still read what dgrow frees (it waits for the main stream only)
        HIPCHK(e, hipStreamSynchronize(e->copy_stream));
        if ((st = dgrow(e, &e->ing.raw, &e->ing.cap_raw, (size_t)plan.bytes))) return st;
        if ((st = dgrow(e, &e->ing.chunks, &e->ing.cap_chunks, tables))) return st;
    }
    e->zc = false;
    int slot;
    HIPCHK(e, e->ring.take(&slot));
    // a plain call's records travel through the handle's per-frame tables, a rig call's through the rig's per-source ones
    pp_engine::Ing& G = e->ing;
    pp_engine::Ing::Rig& R = G.rig;
    Frame* h_frames = (Frame*)(rig ? R.h_frames : G.h_ring).at(slot);      // (a call packs its own record type tightly)
    pp_engine::Ing::Slot* d_frames = rig ? R.frames : G.frames;
    const RingArray<IngFeat>& h_feats = rig ? R.h_feats : G.h_feats;
    IngFeat* d_feats = rig ? R.feats : G.feats;
    memcpy(h_frames, plan.frames.data(), (size_t)records * sizeof(Frame));
    // the kept counts are device values: everything behind this call is sized from the frames' bounds
    set_resident(e, batch, plan.bound_off.data(), plan.max_bound, false);
    e->ing.batch = batch;
    R.sources = rig ? records : 0;
    if ((st = flip_for_write(e, stream))) return st;
    if (plan.bytes) HIPCHK(e, hipMemcpyAsync(e->ing.raw, data + bo[0], (size_t)plan.bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(e, hipMemcpyAsync(d_frames, h_frames, (size_t)records * sizeof(Frame), hipMemcpyHostToDevice, stream));
    if (rig) {
        memcpy(R.h_src.at(slot), plan.rig.data(), (size_t)records * sizeof(RigSource));
        HIPCHK(e, R.h_src.send(slot, R.src, (size_t)records, stream));
    }
    // the feature columns of a _fields call: a table beside the records, through the same ring slot on the same stream
    if (plan.nfeat) {
        const size_t nfe = (size_t)records * plan.nfeat;
        memcpy(h_feats.at(slot), plan.feats.data(), nfe * sizeof(IngFeat));
        HIPCHK(e, h_feats.send(slot, d_feats, nfe, stream));
    }
    HIPCHK(e, e->ring.sent(slot, stream));
    IngestParamsT<Frame> p;
    memset(&p, 0, sizeof(p));
    p.raw = e->ing.raw; p.frames = (const Frame*)d_frames; p.records = records; p.batch = batch; p.stride = plan.stride;
    if (rig) {
        p.src = R.src; p.src_finite = R.finite; p.src_kept = R.kept; p.out_base = R.out_base;
    } else {
        p.first = c->first; p.decimate = c->decimate;
        memcpy(p.r, c->r, sizeof(p.r)); memcpy(p.r2, c->r2, sizeof(p.r2)); memcpy(p.lift, c->lift, sizeof(p.lift));
    }
    p.chunk_cnt = e->ing.chunks; p.chunk_base = e->ing.chunks + (size_t)records * plan.stride;
    p.finite = e->ing.finite; p.kept = e->ing.kept; p.offsets = e->d_offsets; p.out = e->d_points;
    p.out_rows = (long long)e->B * e->NMAX;
    p.feats = d_feats; p.nfeat = plan.nfeat;
    ProfScope ps(e, nullptr);
    launch_ingest(p, stream);
    HIPCHK(e, hipGetLastError());
    return PP_OK;
}

// the synchronous call of either feed: queue on the main stream, wait, hand out the parity tap
template <typename Frame>
int ingest_sync(pp_engine* e, const char* who, const uint8_t* data, const int64_t* byte_offsets, int batch,
                const pp_ingest_config* cfg, const IngestPlanT<Frame>& plan, float* points_out, int64_t points_out_capacity) {
    int st;
    // an asynchronous ingest still running on the copy stream uses the same staging and chunk tables
    HIPCHK(e, hipStreamWaitEvent(e->stream, e->ev_up, 0));
    prof_reset(e);
    if ((st = enqueue_ingest(e, data, byte_offsets, batch, cfg, plan, e->stream))) return st;
    e->up_pending = false;
    HIPCHK(e, hipStreamSynchronize(e->stream));      // the host buffers may be pageable / reused by the caller
    if (points_out) {
        int total = 0;
        HIPCHK(e, hipMemcpy(&total, e->d_offsets + batch, sizeof(int), hipMemcpyDeviceToHost));
        if (points_out_capacity < total)
            return fail(e, PP_ERR_ARG, "%s: points_out holds %lld points, %d were kept", who, (long long)points_out_capacity, total);
        if (total) HIPCHK(e, hipMemcpy(points_out, e->d_points, (size_t)total * (3 + plan.nfeat) * sizeof(float), hipMemcpyDeviceToHost));
    }
    return PP_OK;
}

// Every exported ingest: the checks, then the synchronous tail or the asynchronous one (as pp_upload_points_async does).
template <typename Layout>
int ingest_call(pp_engine* e, const char* who, const IngestArgs<Layout>& a) {
    if (!e) return PP_ERR_ARG;
    (void)hipSetDevice(e->device);
    if ((a.kind & ING_FIELDS) && a.nfeat < 0) return fail(e, PP_ERR_ARG, "%s: nfeat %d < 0", who, a.nfeat);
    IngestPlanT<typename FrameOf<Layout>::type> plan;
    int st = check_call(e, who, a, &plan);
    if (st) return st;
    if (!(a.kind & ING_ASYNC))
        return ingest_sync(e, who, a.data, a.bo, a.batch, a.cfgs, plan, a.points_out, a.points_out_capacity);
    prof_reset(e);
    if ((st = enqueue_ingest(e, a.data, a.bo, a.batch, a.cfgs, plan, e->copy_stream))) return st;
    return finish_async_upload(e, a.batch);
}

// the counts of the last ingest, once it has run: n of each table (NULL: not wanted)
int read_counts(pp_engine* e, int32_t* finite_counts, const int* d_finite, int32_t* kept_counts, const int* d_kept, int n) {
    (void)hipSetDevice(e->device);
    if (int st = quiesce(e)) return st;              // (an asynchronous ingest runs on the copy stream)
    if (finite_counts) HIPCHK(e, hipMemcpy(finite_counts, d_finite, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (kept_counts) HIPCHK(e, hipMemcpy(kept_counts, d_kept, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return PP_OK;
}

typedef IngestArgs<pp_pc2_layout> Pc2Args;
typedef IngestArgs<pp_depth_layout> DepthArgs;

}  // namespace

extern "C" {

int pp_ingest_pointcloud2(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                          int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_pointcloud2", Pc2Args{data, byte_offsets, layouts, cfg, nullptr, 0, batch, nullptr, 0,
                                                           points_out, points_out_capacity, 0});
}

int pp_ingest_pointcloud2_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                const pp_pc2_layout* layouts, int32_t batch, const pp_ingest_config* cfg) {
    return ingest_call(e, "pp_ingest_pointcloud2_async", Pc2Args{data_pinned, byte_offsets, layouts, cfg, nullptr, 0, batch,
                                                                 nullptr, 0, nullptr, 0, ING_ASYNC});
}

int pp_ingest_depth(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_depth_layout* layouts,
                    int32_t batch, const pp_ingest_config* cfg, float* points_out, int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_depth", DepthArgs{data, byte_offsets, layouts, cfg, nullptr, 0, batch, nullptr, 0,
                                                       points_out, points_out_capacity, 0});
}

int pp_ingest_depth_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                          const pp_depth_layout* layouts, int32_t batch, const pp_ingest_config* cfg) {
    return ingest_call(e, "pp_ingest_depth_async", DepthArgs{data_pinned, byte_offsets, layouts, cfg, nullptr, 0, batch,
                                                             nullptr, 0, nullptr, 0, ING_ASYNC});
}

int pp_ingest_rig_depth(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_depth_layout* layouts,
                        const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                        float* points_out, int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_rig_depth", DepthArgs{data, byte_offsets, layouts, cfgs, source_frame, sources, batch,
                                                           nullptr, 0, points_out, points_out_capacity, ING_RIG});
}

int pp_ingest_rig_depth_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                              const pp_depth_layout* layouts, const pp_ingest_config* cfgs, const int32_t* source_frame,
                              int32_t sources, int32_t batch) {
    return ingest_call(e, "pp_ingest_rig_depth_async", DepthArgs{data_pinned, byte_offsets, layouts, cfgs, source_frame, sources,
                                                                 batch, nullptr, 0, nullptr, 0, ING_RIG | ING_ASYNC});
}

int pp_ingest_rig_pointcloud2(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                              const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                              float* points_out, int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_rig_pointcloud2", Pc2Args{data, byte_offsets, layouts, cfgs, source_frame, sources, batch,
                                                               nullptr, 0, points_out, points_out_capacity, ING_RIG});
}

int pp_ingest_rig_pointcloud2_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                    const pp_pc2_layout* layouts, const pp_ingest_config* cfgs, const int32_t* source_frame,
                                    int32_t sources, int32_t batch) {
    return ingest_call(e, "pp_ingest_rig_pointcloud2_async", Pc2Args{data_pinned, byte_offsets, layouts, cfgs, source_frame,
                                                                     sources, batch, nullptr, 0, nullptr, 0, ING_RIG | ING_ASYNC});
}

int pp_ingest_pointcloud2_fields(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                                 int32_t batch, const pp_ingest_config* cfg, const pp_pc2_feature* features, int32_t nfeat,
                                 float* points_out, int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_pointcloud2_fields", Pc2Args{data, byte_offsets, layouts, cfg, nullptr, 0, batch, features,
                                                                  nfeat, points_out, points_out_capacity, ING_FIELDS});
}

int pp_ingest_pointcloud2_fields_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                       const pp_pc2_layout* layouts, int32_t batch, const pp_ingest_config* cfg,
                                       const pp_pc2_feature* features, int32_t nfeat) {
    return ingest_call(e, "pp_ingest_pointcloud2_fields_async", Pc2Args{data_pinned, byte_offsets, layouts, cfg, nullptr, 0, batch,
                                                                        features, nfeat, nullptr, 0, ING_FIELDS | ING_ASYNC});
}

int pp_ingest_rig_pointcloud2_fields(pp_handle e, const uint8_t* data, const int64_t* byte_offsets, const pp_pc2_layout* layouts,
                                     const pp_ingest_config* cfgs, const int32_t* source_frame, int32_t sources, int32_t batch,
                                     const pp_pc2_feature* features, int32_t nfeat, float* points_out,
                                     int64_t points_out_capacity) {
    return ingest_call(e, "pp_ingest_rig_pointcloud2_fields",
                       Pc2Args{data, byte_offsets, layouts, cfgs, source_frame, sources, batch, features, nfeat, points_out,
                               points_out_capacity, ING_RIG | ING_FIELDS});
}

int pp_ingest_rig_pointcloud2_fields_async(pp_handle e, const uint8_t* data_pinned, const int64_t* byte_offsets,
                                           const pp_pc2_layout* layouts, const pp_ingest_config* cfgs,
                                           const int32_t* source_frame, int32_t sources, int32_t batch,
                                           const pp_pc2_feature* features, int32_t nfeat) {
    return ingest_call(e, "pp_ingest_rig_pointcloud2_fields_async",
                       Pc2Args{data_pinned, byte_offsets, layouts, cfgs, source_frame, sources, batch, features, nfeat, nullptr, 0,
                               ING_RIG | ING_FIELDS | ING_ASYNC});
}

int pp_ingest_rig_info(pp_handle e, int32_t* finite_counts, int32_t* kept_counts, int32_t sources) {
    if (!e) return PP_ERR_ARG;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_ingest_rig_info: a training step is in flight");
    if (e->ing.batch < 1 || e->ing.rig.sources < 1) return fail(e, PP_ERR_STATE, "pp_ingest_rig_info: the last ingest was no rig call");
    if (sources != e->ing.rig.sources)
        return fail(e, PP_ERR_ARG, "pp_ingest_rig_info: the last rig ingest had %d sources, sources is %d", e->ing.rig.sources, sources);
    return read_counts(e, finite_counts, e->ing.rig.finite, kept_counts, e->ing.rig.kept, sources);
}

int pp_ingest_info(pp_handle e, int32_t* finite_counts, int32_t* kept_counts, int32_t batch) {
    if (!e) return PP_ERR_ARG;
    if (int st = check_last_run(e, "pp_ingest_info", e->ing.batch, batch, false, "no ingest has run", "ingest", "frames")) return st;
    return read_counts(e, finite_counts, e->ing.finite, kept_counts, e->ing.kept, batch);
}

}  // extern "C"
