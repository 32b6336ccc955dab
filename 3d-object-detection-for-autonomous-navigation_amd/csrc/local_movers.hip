// The movers' table of the local planner from the tracker's slots (pp_local_plan_movers_async; local_planner.py states
// the rule as `movers_np`): one kernel in front of the rollout of local_plan.hip, and the one place of that stage with
// floating point.  One wave per stream, lane = slot: the slot's position, velocity and size -- carried into the fixed frame
// by the pose of the stream's last posed tracking step for the occupancy source, with the very expressions k_track_step
// uses for its fixed-frame rows -- become six integers in sub-cells; the slots that qualify are compacted in ascending
// slot order by ballot and prefix popcount, as k_costmap_objects compacts its footprints.  Float64, every operation
// rounded on its own (the library is built with -ffp-contract=off); floor, rint and ceil are the only roundings, there is
// no sqrt and no trig, and no atomics of any kind.
#include "pp_common.h"

namespace {

constexpr int LOC_MOVER_POS = 1 << 29;                   // |mx|, |my| at most
static_assert(PP_LOCAL_MAX_MOVERS == 64 && PP_TRACK_MAX == 64 && PP_WAVE == 64, "one lane per track slot, a mover per slot at most");
static_assert(LOC_MOVER_POS < (1ll << 31) && PP_LOCAL_MAX_MOVER_SPEED < (1ll << 31) && PP_LOCAL_MAX_MOVER_RADIUS < (1ll << 31),
              "what passes the range checks converts to int32 exactly");

__device__ __forceinline__ bool loc_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // (false for a NaN)

// The table of one stream's movers from its track slots: float64, every operation rounded on its own (the library is
// built with -ffp-contract=off), floor / rint / ceil the only roundings
__global__ __launch_bounds__(64) void k_local_movers(LocalMoverParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int* table = p.movers + (size_t)b * PP_LOCAL_MAX_MOVERS * 6;
    int* info = p.mover_info + b;
    const TrkPose* pv = p.pose_prev + b;
    if (p.fixed && pv->has == 0) {                       // no posed step yet: no fixed frame (the whole wave)
#pragma unroll
        for (int q = 0; q < 6; ++q) table[6 * lane + q] = 0;
        if (lane == 0) { info[LOC_M_COUNT * p.info_stride] = -1; info[LOC_M_SKIPPED * p.info_stride] = 0; }
        return;
    }
    const TrkSlot* t = p.slots + (size_t)b * PP_TRACK_MAX + lane;
    const LocalFrame f = p.frame[b];
    const bool use = t->live != 0 && (!p.confirmed_only || t->confirmed != 0);
    int m[6] = {0, 0, 0, 0, 0, 0};
    bool ok = false;
    if (use) {
        double x[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = t->x[q];
        if (p.fixed) {                                   // the expressions of k_track_step's out_fixed
            const double* R = pv->m;
            double y[6];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                y[i] = ((R[i * 4] * x[0] + R[i * 4 + 1] * x[1]) + R[i * 4 + 2] * x[2]) + R[i * 4 + 3];
                y[3 + i] = (R[i * 4] * x[3] + R[i * 4 + 1] * x[4]) + R[i * 4 + 2] * x[5];
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) x[q] = y[q];
        }
        const double w = t->size[0], l = t->size[1];
        ok = loc_finite(w) && loc_finite(l);
#pragma unroll
        for (int q = 0; q < 6; ++q) ok = ok && loc_finite(x[q]);
        if (ok) {
            const double MX = floor(((x[0] - f.ox) / f.res) * 1024.0), MY = floor(((x[1] - f.oy) / f.res) * 1024.0);
            const double MVX = rint(((x[3] * f.dt) / f.res) * 1024.0), MVY = rint(((x[4] * f.dt) / f.res) * 1024.0);
            const double half = fmax(w, l) * 0.5;
            const double RH = ceil(((half + p.pad_hard) / f.res) * 1024.0), RS = ceil(((half + p.pad_soft) / f.res) * 1024.0);
            // (written so that a NaN, which finite inputs cannot give, would skip the slot)
            ok = fabs(MX) <= (double)LOC_MOVER_POS && fabs(MY) <= (double)LOC_MOVER_POS &&
                 fabs(MVX) <= (double)PP_LOCAL_MAX_MOVER_SPEED && fabs(MVY) <= (double)PP_LOCAL_MAX_MOVER_SPEED;
            if (ok) {
                m[0] = (int)MX; m[1] = (int)MY; m[2] = (int)MVX; m[3] = (int)MVY;
                m[4] = (int)fmin(fmax(RH, 0.0), (double)PP_LOCAL_MAX_MOVER_RADIUS);
                m[5] = (int)fmin(fmax(RS, 0.0), (double)PP_LOCAL_MAX_MOVER_RADIUS);
            }
        }
    }
    const unsigned long long taken = __ballot(ok);
    const int cnt = __popcll(taken);
    if (ok) {
        int* d = table + 6 * __popcll(taken & ((1ull << lane) - 1ull));
#pragma unroll
        for (int q = 0; q < 6; ++q) d[q] = m[q];
    }
    if (lane >= cnt) {                                   // zeros behind the movers
#pragma unroll
        for (int q = 0; q < 6; ++q) table[6 * lane + q] = 0;
    }
    const int skipped = __popcll(__ballot(use && !ok));
    if (lane == 0) { info[LOC_M_COUNT * p.info_stride] = cnt; info[LOC_M_SKIPPED * p.info_stride] = skipped; }
}

}  // namespace

void launch_local_movers(const LocalMoverParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_local_movers", k_local_movers, dim3(p.batch), dim3(64), 0, s, p);
}
