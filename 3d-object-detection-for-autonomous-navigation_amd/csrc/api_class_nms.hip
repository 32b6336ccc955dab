// C-ABI, joint or per-class suppression: the mode of the detector's post-process (per handle; the kernel instantiations and
// the gather kernel are in postprocess.hip) and the result rows per frame that follow from it.
#include "pp_engine.h"

extern "C" {

int pp_set_class_nms(pp_handle e, int32_t mode) {
    if (!e) return PP_ERR_ARG;
    if (mode != PP_CLASS_NMS_JOINT && mode != PP_CLASS_NMS_PER_CLASS) return fail(e, PP_ERR_ARG, "pp_set_class_nms: unknown mode %d", mode);
    if (mode == e->rule.class_nms) return PP_OK;
    if (e->train_pending) return fail(e, PP_ERR_STATE, "pp_set_class_nms: a training step is in flight");
    // results of a pass in the other mode have the other row stride: the getters compare results_rows with det_rows and
    // refuse them
    e->rule.class_nms = mode;
    return PP_OK;
}

int pp_get_class_nms(pp_handle e, int32_t* mode) {
    if (!e || !mode) return PP_ERR_ARG;
    *mode = e->rule.class_nms;
    return PP_OK;
}

int pp_get_detection_rows(pp_handle e, int32_t* rows) {
    if (!e || !rows) return PP_ERR_ARG;
    *rows = det_rows(e);
    return PP_OK;
}

}  // extern "C"
