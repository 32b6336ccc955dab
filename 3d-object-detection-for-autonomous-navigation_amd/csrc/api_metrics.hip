// C-ABI, training metrics: the counts of metrics.hip on the handle's head map or on logits
// handed in (pp_head_metrics), and as part of every training step (pp_set_train_metrics: api_train.hip's
// train_step_launch adds the launch to the step's second half).
#include "pp_engine.h"

int ensure_metrics(pp_engine* e) {
    pp_engine::Metrics& m = e->metrics;
    if (m.h_counts) return PP_OK;
    int st = ensure_loss_buffers(e);      // (the labels live with the loss's)
    if (st) return st;
    DevAlloc A{e};
    A(&m.partials, (size_t)e->B * metrics_blocks(e->head_h * e->head_w) * PP_METRICS_COUNTS);
    A(&m.counts, (size_t)PP_METRICS_COUNTS);
    if (A.st) return A.st;
    HIPCHK(e, hipHostMalloc((void**)&m.h_counts, PP_METRICS_COUNTS * sizeof(long long)));   // (last: the group's ready flag)
    return PP_OK;
}

void fill_metrics_params(pp_engine* e, int batch, MetricsParams& p) {
    memset(&p, 0, sizeof(p));
    p.batch = batch; p.A = e->A; p.npx = e->head_h * e->head_w; p.napl = e->napl; p.ncls = e->ncls;
    p.logits = e->d_head; p.row_stride = PP_HEAD_COLS; p.col_off = e->napl * 7;
    p.labels = e->loss.labels; p.partials = e->metrics.partials; p.counts = e->metrics.counts;
}

extern "C" {

int pp_head_metrics(pp_handle e, const int32_t* labels, int32_t batch, const float* cls_preds, int64_t* counts) {
    if (!e) return PP_ERR_ARG;
    if (!labels || !counts) return fail(e, PP_ERR_ARG, "pp_head_metrics: null argument");
    if (!e->anchors_ready) return fail(e, PP_ERR_STATE, "pp_head_metrics: anchors not set");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_head_metrics: a training step is in flight");
    int st = check_batch(e, batch);
    if (st) return st;
    (void)hipSetDevice(e->device);
    if ((st = ensure_metrics(e))) return st;
    pp_engine::Metrics& m = e->metrics;
    prof_reset(e);
    const size_t n = (size_t)batch * e->A;
    HIPCHK(e, hipMemcpyAsync(e->loss.labels, labels, n * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    MetricsParams p;
    fill_metrics_params(e, batch, p);
    if (cls_preds) {
        if (!m.logits && (st = dalloc(e, &m.logits, (size_t)e->B * e->A * e->ncls))) return st;
        HIPCHK(e, hipMemcpyAsync(m.logits, cls_preds, n * e->ncls * sizeof(float), hipMemcpyHostToDevice, e->stream));
        p.logits = m.logits; p.row_stride = e->napl * e->ncls; p.col_off = 0;
    }
    {
        ProfScope ps(e, nullptr);      // (each launch under its own name)
        if ((st = launch_head_metrics(p, e->stream)))
            return fail(e, st, "pp_head_metrics: %d anchors per pixel x %d classes not supported", e->napl, e->ncls);
    }
    HIPCHK(e, hipGetLastError());
    static_assert(sizeof(long long) == sizeof(int64_t), "counts are int64");
    HIPCHK(e, hipMemcpyAsync(counts, m.counts, PP_METRICS_COUNTS * sizeof(int64_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(e, hipStreamSynchronize(e->stream));
    return PP_OK;
}

int pp_set_train_metrics(pp_handle e, int32_t on) {
    if (!e) return PP_ERR_ARG;
    if (on != 0 && on != 1) return fail(e, PP_ERR_ARG, "pp_set_train_metrics: %d is neither 0 nor 1", on);
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_train_metrics: a training step is in flight");
    e->metrics.on = on != 0;      // (a captured step is keyed on it: the next one captures once more)
    return PP_OK;
}

int pp_get_train_metrics_enabled(pp_handle e, int32_t* on) {
    if (!e) return PP_ERR_ARG;
    if (!on) return fail(e, PP_ERR_ARG, "pp_get_train_metrics_enabled: null argument");
    *on = e->metrics.on ? 1 : 0;
    return PP_OK;
}

int pp_get_train_metrics(pp_handle e, int64_t* counts) {
    if (!e) return PP_ERR_ARG;
    if (!counts) return fail(e, PP_ERR_ARG, "pp_get_train_metrics: null argument");
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_get_train_metrics: the step has not been waited for");
    if (!e->train || e->train->last_batch < 1) return fail(e, PP_ERR_STATE, "pp_get_train_metrics: no training step has run");
    if (!e->metrics.step_counted)
        return fail(e, PP_ERR_STATE, "pp_get_train_metrics: the last step ran with the metrics off (pp_set_train_metrics)");
    memcpy(counts, e->metrics.h_counts, PP_METRICS_COUNTS * sizeof(int64_t));
    return PP_OK;
}

}  // extern "C"
