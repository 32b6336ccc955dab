"""The backbone's kernel planner without a device (pp_plan_layer_name): which template instantiation launch_layer would
run one layer under.  Tests and tuning tools ask it; a pass never does."""
import ctypes

from . import _lib

KINDS = {"sep": 0, "deconv": 1, "head": 2}
MI355X_CUS = 256


def plan_layer_name(layer, batch, compute_units=MI355X_CUS):
    """layer: a dict with kind ('sep' / 'deconv' / 'head'), cin, cout, n_total, stride, k, in_h, in_w, out_h, out_w,
    head_mode and the flags has_wt16, has_head_wt16, sparse_input (missing keys are 0).  Returns the full instantiation
    name, e.g. 'k_sep_u<64,1,3,1,0,0,1>'.  The process-start switches apply as they do to a pass."""
    d = _lib.PPLayerPlanDesc()
    for name, _ in d._fields_:
        v = layer.get(name, 0)
        setattr(d, name, KINDS[v] if name == "kind" else int(v))
    buf = ctypes.create_string_buffer(64)
    st = _lib.lib().pp_plan_layer_name(ctypes.byref(d), int(batch), int(compute_units), buf, 64)
    if st != 0:
        raise ValueError(f"pp_plan_layer_name: status {st} for {layer} at batch {batch}, {compute_units} CUs")
    return buf.value.decode()
