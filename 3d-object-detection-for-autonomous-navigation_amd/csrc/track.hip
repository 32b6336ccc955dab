// Tracking across frames (pp_set_tracking / pp_track_update; tracking.py restates the rule and the tests hold this kernel
// to it bit for bit): one step of one stream's track table per wavefront, lane = track slot.
//
// All arithmetic is float64 with + - * / and comparisons, written in the restatement's order; the library is built with
// -ffp-contract=off, so no product is fused into a sum and every intermediate is the restatement's.
//
// Association is greedy by the global minimum of (d2, slot, row).  Every lane keeps the best (d2, row) of its own track
// over the rows still free (ascending scan, strict <: the lowest row among equals); a round takes the wave's minimum
// (d2, slot) with an xor butterfly (the total order makes every lane agree), retires that track and that row, and only
// the lanes whose best row has just been taken scan again -- rows only ever leave, so every other lane's best stands.
// The free rows are a 2 x 64-bit mask in registers (PP_TRACK_MASK_ROWS); births and the compacted output positions come
// from ballots and popcounts.  No LDS, no atomics; the rounds' dependent cross-lane chain is what the kernel costs.
//
// Ego motion (pp_set_track_pose): a stream that was given a pose for this step first carries its live tracks from the sensor
// frame of its previous posed step into the current one (stage 0), and its rows go out a second time in the fixed frame.
// The poses and psi = atan2(R10, R00) come from the host; the kernel multiplies, adds and subtracts.
#include "pp_common.h"

namespace {

constexpr int TRK_NONE = 0x7fffffff;

// smaller value, then smaller index; an index of TRK_NONE is "no candidate"
__device__ __forceinline__ void wave_min_pair(double& v, int& idx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m, PP_WAVE);
        const int oi = __shfl_xor(idx, m, PP_WAVE);
        const bool take = oi != TRK_NONE && (idx == TRK_NONE || ov < v || (ov == v && oi < idx));
        if (take) { v = ov; idx = oi; }
    }
}

__device__ __forceinline__ bool row_bit(unsigned long long lo, unsigned long long hi, int r) {
    return ((r < 64 ? lo >> r : hi >> (r - 64)) & 1ull) != 0ull;
}

// index of the k-th (from 0) set bit of the 128-bit mask (lo, hi); the caller guarantees it exists
__device__ __forceinline__ int kth_set_bit(unsigned long long lo, unsigned long long hi, int k) {
    const int c = __popcll(lo);
    unsigned long long m = lo;
    int base = 0;
    if (k >= c) { k -= c; m = hi; base = 64; }
    for (int i = 0; i < k; ++i) m &= m - 1ull;
    return base + (int)__ffsll((long long)m) - 1;
}

__global__ __launch_bounds__(PP_WAVE) void k_track_step(TrackParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int raw = p.n_dets[b];
    if (raw & PP_NDETS_NONFINITE) {              // the whole wave: the stream's table and outputs stay as they are
        if (lane == 0) {                         // ... but the step's dt and pose are spent: they must not reach a later
            p.dt[b] = 0.0;                       // pass (the previous pose stays: the next posed step carries over the
            p.pose_q[b].has = 0;                 // whole motion since the last step that ran)
        }
        return;
    }
    const int n = min(max(raw, 0), p.rows);
    const pp_track_config cfg = *p.cfg;
    double dt = p.dt[b];
    if (!(dt > 0.0)) dt = cfg.period;
    const pp_detection* dets = p.dets + (size_t)b * p.rows;
    TrkSlot* slot = p.state + (size_t)b * PP_TRACK_MAX + lane;
    TrkSlot t = *slot;
    bool live = t.live != 0;

    // ---- 0. ego motion: carry the live tracks from the previous posed sensor frame into this step's ----
    // Every address below is the stream's alone, so the pose, M, u and the yaw step are the same in every lane.  Every lane
    // has read the previous pose into registers here, long before lane 0 rewrites it in the closing block.  A step without
    // a pose runs none of this -- not even with an identity, which would turn -0.0 into +0.0.
    const bool posed = p.pose_q[b].has != 0;
    double R[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, psi = 0.0;
    if (posed) {
        const TrkPose* q = p.pose_q + b;
#pragma unroll
        for (int i = 0; i < 12; ++i) R[i] = q->m[i];
        psi = q->psi;
        const TrkPose* pv = p.pose_prev + b;
        if (pv->has != 0) {
            double S[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) S[i] = pv->m[i];
            const double dpsi = psi - pv->psi;
            // sweeps.relative_transform(P_c, prev): M = R_c^T R_s, u = R_c^T (t_s - t_c), in that function's order
            const double d0 = S[3] - R[3], d1 = S[7] - R[7], d2 = S[11] - R[11];
            double M[9], u[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int j = 0; j < 3; ++j) M[i * 3 + j] = (R[i] * S[j] + R[4 + i] * S[4 + j]) + R[8 + i] * S[8 + j];
                u[i] = (R[i] * d0 + R[4 + i] * d1) + R[8 + i] * d2;
            }
            if (live) {
                const double x = t.x[0], y = t.x[1], z = t.x[2], vx = t.x[3], vy = t.x[4], vz = t.x[5];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    t.x[i] = ((M[i * 3] * x + M[i * 3 + 1] * y) + M[i * 3 + 2] * z) + u[i];
                    t.x[3 + i] = (M[i * 3] * vx + M[i * 3 + 1] * vy) + M[i * 3 + 2] * vz;
                }
                t.yaw = t.yaw + dpsi;
            }
        }
    }

    // ---- 1. predict ----
    if (live) {
        t.x[0] = t.x[0] + t.x[3] * dt;
        t.x[1] = t.x[1] + t.x[4] * dt;
        t.x[2] = t.x[2] + t.x[5] * dt;
        const double dt2 = dt * dt;
        const double a = t.p[1] + dt * t.p[2];
        const double p00 = (t.p[0] + dt * t.p[1]) + dt * a;
        t.p[0] = p00 + cfg.q_acc * (dt2 * dt2 * 0.25);
        t.p[1] = a + cfg.q_acc * (dt2 * dt * 0.5);
        t.p[2] = t.p[2] + cfg.q_acc * dt2;
    }

    // ---- 2. associate ----
    unsigned long long free_lo = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
    unsigned long long free_hi = n <= 64 ? 0ull : (n >= 128 ? ~0ull : ((1ull << (n - 64)) - 1ull));
    const double gate2 = cfg.gate * cfg.gate;
    int mrow = -1;                  // the row this lane's track is matched with
    bool rescan = live;
    double best = 0.0;
    int best_row = -1;
    for (int round = 0; round < PP_TRACK_MAX; ++round) {
        if (rescan) {
            best_row = -1;
            for (int r = 0; r < n; ++r) {
                if (!row_bit(free_lo, free_hi, r)) continue;
                if (cfg.class_aware && dets[r].label != t.label) continue;
                const double dx = t.x[0] - (double)dets[r].box3d_lidar[0];
                const double dy = t.x[1] - (double)dets[r].box3d_lidar[1];
                const double d2 = dx * dx + dy * dy;
                if (d2 <= gate2 && (best_row < 0 || d2 < best)) { best = d2; best_row = r; }
            }
            rescan = false;
        }
        const bool cand = live && mrow < 0 && best_row >= 0;
        double v = cand ? best : 0.0;
        int w = cand ? lane : TRK_NONE;
        wave_min_pair(v, w);
        if (w == TRK_NONE) break;               // wave-uniform: every lane holds the same winner
        const int rw = __shfl(best_row, w, PP_WAVE);
        if (lane == w) mrow = rw;
        else if (cand && best_row == rw) rescan = true;
        if (rw < 64) free_lo &= ~(1ull << rw); else free_hi &= ~(1ull << (rw - 64));
    }

    // ---- 3. update the matched, 4. age the others ----
    int det_row = -1;
    if (live && mrow >= 0) {
        const pp_detection d = dets[mrow];
        const double s = t.p[0] + cfg.r_pos;
        const double k0 = t.p[0] / s, k1 = t.p[1] / s;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double y = (double)d.box3d_lidar[q] - t.x[q];
            t.x[q] = t.x[q] + k0 * y;
            t.x[q + 3] = t.x[q + 3] + k1 * y;
        }
        const double omk = 1.0 - k0;
        t.p[2] = t.p[2] - k1 * t.p[1];
        t.p[1] = omk * t.p[1];
        t.p[0] = omk * t.p[0];
        const double oma = 1.0 - cfg.size_alpha;
#pragma unroll
        for (int q = 0; q < 3; ++q) t.size[q] = oma * t.size[q] + cfg.size_alpha * (double)d.box3d_lidar[3 + q];
        t.yaw = (double)d.box3d_lidar[6];
        t.score = d.score;
        t.label = d.label;
        t.hits += 1;
        t.misses = 0;
        if (t.hits >= cfg.min_hits) t.confirmed = 1;
        det_row = mrow;
    } else if (live) {
        t.misses += 1;
        if (t.misses > cfg.max_misses) live = false;
    }

    // ---- 5. births: the k-th unmatched row that may open a track takes the k-th lowest free slot ----
    const bool e0 = lane < n && row_bit(free_lo, free_hi, lane) && (double)dets[lane].score >= cfg.birth_score;
    const bool e1 = lane + 64 < n && row_bit(free_lo, free_hi, lane + 64) && (double)dets[lane + 64].score >= cfg.birth_score;
    const unsigned long long born_lo = __ballot(e0), born_hi = __ballot(e1);
    const int nborn = __popcll(born_lo) + __popcll(born_hi);
    const unsigned long long free_slots = __ballot(!live);
    const int nfree = __popcll(free_slots);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int next_id = p.next_id[b];
    if (!live) {
        const int k = __popcll(free_slots & below);
        if (k < nborn) {
            const int r = kth_set_bit(born_lo, born_hi, k);
            const pp_detection d = dets[r];
#pragma unroll
            for (int q = 0; q < 3; ++q) { t.x[q] = (double)d.box3d_lidar[q]; t.x[q + 3] = 0.0; t.size[q] = (double)d.box3d_lidar[3 + q]; }
            t.p[0] = cfg.p0_pos; t.p[1] = 0.0; t.p[2] = cfg.p0_vel;
            t.yaw = (double)d.box3d_lidar[6];
            t.score = d.score;
            t.id = next_id + k;
            t.label = d.label;
            t.hits = 1;
            t.misses = 0;
            t.confirmed = 1 >= cfg.min_hits ? 1 : 0;
            live = true;
            det_row = r;
        }
    }
    const int opened = min(nborn, nfree);
    const int overflow = p.overflow[b] + (nborn - opened);

    // ---- 6. the table back, and the live tracks compacted in slot order ----
    t.live = live ? 1 : 0;
    *slot = t;
    const unsigned long long alive = __ballot(live);
    if (live) {
        pp_track o;
#pragma unroll
        for (int q = 0; q < 6; ++q) o.state[q] = t.x[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) o.size[q] = t.size[q];
        o.yaw = t.yaw;
        o.score = t.score;
        o.id = t.id; o.label = t.label; o.hits = t.hits; o.misses = t.misses; o.confirmed = t.confirmed;
        o.det_row = det_row;
        o.reserved = 0;
        const size_t at = (size_t)b * PP_TRACK_MAX + __popcll(alive & below);
        p.out[at] = o;
        if (posed) {                             // the same row in the fixed frame of this step's pose
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                o.state[i] = ((R[i * 4] * t.x[0] + R[i * 4 + 1] * t.x[1]) + R[i * 4 + 2] * t.x[2]) + R[i * 4 + 3];
                o.state[3 + i] = (R[i * 4] * t.x[3] + R[i * 4 + 1] * t.x[4]) + R[i * 4 + 2] * t.x[5];
            }
            o.yaw = t.yaw + psi;
            p.out_fixed[at] = o;
        }
    }
    if (lane == 0) {
        const int cnt = __popcll(alive);
        p.next_id[b] = next_id + opened;
        p.overflow[b] = overflow;
        p.dt[b] = 0.0;                           // consumed: the next step uses the period unless pp_set_track_dt speaks again
        p.n_out[b] = cnt;
        p.overflow_out[b] = overflow;
        p.n_out_fixed[b] = posed ? cnt : -1;
        if (posed) {                             // consumed likewise; this step's pose is the next posed step's previous one
            TrkPose* pv = p.pose_prev + b;
#pragma unroll
            for (int i = 0; i < 12; ++i) pv->m[i] = R[i];
            pv->psi = psi;
            pv->has = 1;
            p.pose_q[b].has = 0;
        }
    }
}

}  // namespace

void launch_track_step(const TrackParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_track_step", k_track_step, dim3(p.batch), dim3(PP_WAVE), 0, s, p);
}
