// C-ABI, detection during training: pp_publish_train_weights folds a trainer's flat parameter / state buffers
// (pp_train_layout) into the detector's weight arrays on the device (weight_publish.hip) -- what pp_set_weight x 82 +
// pp_finalize_weights do through the host.  The first publish on a handle (or the first after a pp_finalize_weights)
// allocates the arrays; later ones write the same allocations and leave the captured inference graphs alone, unless the
// set of layers on the float32 fallback changed.
#include "pp_engine.h"

namespace {

template <typename Tp>
int walloc(pp_engine* e, Tp** p, size_t count) {
    void* q = nullptr;
    HIPCHK(e, hipMalloc(&q, (count ? count : 1) * sizeof(Tp)));
    e->wallocs.push_back(q);       // released by the next pp_finalize_weights / pp_destroy
    *p = (Tp*)q;
    return PP_OK;
}

// the layers that can run on float16 pieces at all (pp_finalize_weights' conditions besides the range)
bool wt16_eligible(const LayerDesc& L) { return L.kind != LAYER_HEAD && L.cin % 16 == 0; }
bool head16_eligible(const LayerDesc& L) { return L.kind == LAYER_DECONV && L.head_mode != 0 && L.cout % 32 == 0; }

struct TaskList {
    std::vector<PubTask> t;
    int blocks = 0;
    PubTask& add(int kind, int n) {
        PubTask q;
        memset(&q, 0, sizeof(q));
        q.kind = kind; q.n = n; q.block0 = blocks;
        blocks += publish_blocks(n);
        t.push_back(q);
        return t.back();
    }
};

// the weight arrays of every layer, the task tables that fill them and the flags; the stream is idle (graphs dropped)
int publish_allocate(pp_engine* e) {
    pp_engine::Publish& pb = e->pub;
    const TrainPlan& plan = e->train->plan;
    for (void* p : e->wallocs) (void)hipFree(p);
    e->wallocs.clear();
    const size_t NL = e->layers.size();
    pb.wt16.assign(NL, nullptr);
    pb.head_wt16.assign(NL, nullptr);
    pb.h_flags.assign(2 * NL, 0);
    pb.head.box_k = plan.box_k; pb.head.box_b = plan.box_b; pb.head.cls_k = plan.cls_k; pb.head.cls_b = plan.cls_b;
    pb.head.dir_k = plan.dir_k; pb.head.dir_b = plan.dir_b;
    pb.head.nb = e->napl * 7; pb.head.nc = e->napl * e->ncls; pb.head.nd = e->use_dir ? e->napl * 2 : 0;
    TaskList fold, split;
    int st;
    auto bn = [](PubTask& q, int64_t gamma, int64_t beta, int64_t mean, int64_t var) {
        q.gamma = gamma; q.beta = beta; q.mean = mean; q.var = var;
    };
    auto split_task = [&](int kind, const float* wt, float** slot, int n_total, int cin, int flag) -> int {
        unsigned short* w16 = nullptr;
        if (int r = walloc(e, &w16, (size_t)n_total * cin * PP_NPIECE)) return r;
        *slot = (float*)w16;
        PubTask& q = split.add(kind, n_total * (cin / 16));
        q.cin = cin; q.n_total = n_total; q.wt = wt; q.out16 = w16; q.flag = flag;
        return PP_OK;
    };
    // PFN
    {
        if ((st = walloc(e, &e->d_pfn_w, (size_t)e->FA * e->C))) return st;
        if ((st = walloc(e, &e->d_pfn_b, (size_t)e->C))) return st;
        PubTask& w = fold.add(PUB_PFN_W, e->FA * e->C);
        w.src = plan.pfn_w; w.cout = e->C; w.out = e->d_pfn_w;
        bn(w, plan.pfn_gamma, plan.pfn_beta, plan.pfn_mean, plan.pfn_var);
        PubTask& b = fold.add(PUB_SHIFT, e->C);
        b.out = e->d_pfn_b;
        bn(b, plan.pfn_gamma, plan.pfn_beta, plan.pfn_mean, plan.pfn_var);
    }
    // separable layers and transposed convolutions, in the plan's (= the table's) order
    for (const TrainLayer& tl : plan.layers) {
        LayerDesc& L = e->layers[tl.layer];
        L.d_wt16 = nullptr;          // which layers run on their float16 arrays: apply_pattern, once the flags are known
        L.d_head_wt16 = nullptr;
        if ((st = walloc(e, &L.d_wt, (size_t)L.n_total * L.cin))) return st;
        if ((st = walloc(e, &L.d_bias, (size_t)L.cout))) return st;
        if (L.kind == LAYER_SEP) {
            if ((st = walloc(e, &L.d_dw, (size_t)9 * L.cin))) return st;
            PubTask& d = fold.add(PUB_COPY, 9 * L.cin);
            d.src = tl.dw; d.out = L.d_dw;
        }
        PubTask& w = fold.add(L.kind == LAYER_SEP ? PUB_SEP_WT : PUB_DEC_WT, L.n_total * L.cin);
        w.src = tl.pw; w.cin = L.cin; w.cout = L.cout; w.out = L.d_wt;
        bn(w, tl.gamma, tl.beta, tl.mean, tl.var);
        PubTask& b = fold.add(PUB_SHIFT, L.cout);
        b.out = L.d_bias;
        bn(b, tl.gamma, tl.beta, tl.mean, tl.var);
        if (wt16_eligible(L) && (st = split_task(PUB_SPLIT, L.d_wt, &pb.wt16[tl.layer], L.n_total, L.cin, 2 * tl.layer)))
            return st;
        if (L.kind == LAYER_DECONV && L.head_mode != 0) {   // this branch's [PP_HEAD_COLS][cout] slice of the head matrix
            if ((st = walloc(e, &L.d_head_wt, (size_t)PP_HEAD_COLS * L.cout))) return st;
            if ((st = walloc(e, &L.d_head_bias, (size_t)PP_HEAD_COLS))) return st;
            PubTask& h = fold.add(PUB_HEAD_WT, PP_HEAD_COLS * L.cout);
            h.cout = L.cout; h.co_off = L.co_off; h.out = L.d_head_wt;
            fold.add(PUB_HEAD_BIAS, PP_HEAD_COLS).out = L.d_head_bias;
            if (head16_eligible(L) &&
                (st = split_task(PUB_SPLIT_HEAD, L.d_head_wt, &pb.head_wt16[tl.layer], PP_HEAD_COLS, L.cout, 2 * tl.layer + 1)))
                return st;
        }
    }
    // the unfused head layer: the whole [PP_HEAD_COLS][CC] matrix and its bias
    for (LayerDesc& L : e->layers) {
        if (L.kind != LAYER_HEAD) continue;
        L.d_wt16 = nullptr;
        if ((st = walloc(e, &L.d_wt, (size_t)PP_HEAD_COLS * e->CC))) return st;
        if ((st = walloc(e, &L.d_bias, (size_t)PP_HEAD_COLS))) return st;
        PubTask& h = fold.add(PUB_HEAD_WT, PP_HEAD_COLS * e->CC);
        h.cout = e->CC; h.co_off = 0; h.out = L.d_wt;
        fold.add(PUB_HEAD_BIAS, PP_HEAD_COLS).out = L.d_bias;
    }
    if ((st = walloc(e, &pb.d_flags, 2 * NL))) return st;
    if ((st = walloc(e, &pb.d_fold, fold.t.size()))) return st;
    if ((st = walloc(e, &pb.d_split, split.t.size()))) return st;
    HIPCHK(e, hipMemcpy(pb.d_fold, fold.t.data(), fold.t.size() * sizeof(PubTask), hipMemcpyHostToDevice));
    if (!split.t.empty())
        HIPCHK(e, hipMemcpy(pb.d_split, split.t.data(), split.t.size() * sizeof(PubTask), hipMemcpyHostToDevice));
    pb.n_fold = (int)fold.t.size(); pb.fold_blocks = fold.blocks;
    pb.n_split = (int)split.t.size(); pb.split_blocks = split.blocks;
    return PP_OK;
}

// Point every layer at its float16 array, or at none: forced float32, not eligible, or out of range at the last
// publish -- the launchers then pick the float32 instantiation, as after pp_finalize_weights.  A change drops the
// captured graphs (they hold the other instantiation).  `fresh`: the arrays were just allocated, the graphs are gone.
void apply_pattern(pp_engine* e, bool fresh) {
    pp_engine::Publish& pb = e->pub;
    bool changed = false;
    int fallback = 0;
    std::vector<float*> w16(e->layers.size(), nullptr), h16(e->layers.size(), nullptr);
    for (size_t i = 0; i < e->layers.size(); ++i) {
        const LayerDesc& L = e->layers[i];
        if (L.kind == LAYER_HEAD) continue;
        if (!e->force_f32 && !pb.h_flags[2 * i]) w16[i] = pb.wt16[i];
        if (!e->force_f32 && !pb.h_flags[2 * i + 1]) h16[i] = pb.head_wt16[i];
        if (w16[i] == nullptr) ++fallback;
        changed = changed || w16[i] != L.d_wt16 || h16[i] != L.d_head_wt16;
    }
    e->f32_fallback_layers = fallback;
    if (!changed && !fresh) return;
    drop_detect_graphs(e);
    if (!fresh) ++pb.graph_invalidations;
    for (size_t i = 0; i < e->layers.size(); ++i) {
        if (e->layers[i].kind == LAYER_HEAD) continue;
        e->layers[i].d_wt16 = w16[i];
        e->layers[i].d_head_wt16 = h16[i];
    }
    decide_sparse_canvas(e);      // layer 0's kernel may have changed
    e->tag_batch = -1;
}

}  // namespace

int publish_reapply(pp_engine* e) {
    (void)hipSetDevice(e->device);
    apply_pattern(e, false);
    return PP_OK;
}

extern "C" {

int pp_publish_train_weights(pp_handle e, const float* params_dev, const float* state_dev) {
    if (!e) return PP_ERR_ARG;
    if (!params_dev || !state_dev) return fail(e, PP_ERR_ARG, "pp_publish_train_weights: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_publish_train_weights: a training step is in flight");
    (void)hipSetDevice(e->device);
    int st = pp_train_layout(e, nullptr, nullptr, nullptr);      // the plan holds every tensor's offset
    if (st) return st;
    pp_engine::Publish& pb = e->pub;
    const bool fresh = !pb.live;
    if (fresh) {
        drop_detect_graphs(e);        // waits for the stream; the captured graphs hold the old weight pointers
        e->weights_ready = false;
        pb.live = false;
        if ((st = publish_allocate(e))) return st;
        ++pb.reallocations;
        ++pb.graph_invalidations;
    }
    HIPCHK(e, hipMemsetAsync(pb.d_flags, 0, pb.h_flags.size() * sizeof(int), e->stream));
    prof_reset(e);
    {
        ProfScope ps(e, nullptr);     // pp_set_profiling: the two launches' own times (pp_get_kernel_times)
        launch_publish_fold(pb.d_fold, pb.n_fold, pb.fold_blocks, pb.head, params_dev, state_dev, e->stream);
        launch_publish_split(pb.d_split, pb.n_split, pb.split_blocks, pb.d_flags, e->stream);
    }
    HIPCHK(e, hipGetLastError());
    HIPCHK(e, hipMemcpyAsync(pb.h_flags.data(), pb.d_flags, pb.h_flags.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    pb.live = true;
    apply_pattern(e, fresh);
    e->weights_ready = true;
    ++pb.publishes;
    return PP_OK;
}

int pp_publish_info(pp_handle e, pp_publish_stats* out) {
    if (!e) return PP_ERR_ARG;
    if (!out) return fail(e, PP_ERR_ARG, "pp_publish_info: null argument");
    out->publishes = e->pub.publishes;
    out->reallocations = e->pub.reallocations;
    out->graph_invalidations = e->pub.graph_invalidations;
    out->f32_fallback_layers = e->f32_fallback_layers;
    return PP_OK;
}

}  // extern "C"
