// Local planner over an inflated int8 OccupancyGrid and its cost-to-go field (pp_set_local_plan / pp_local_plan_async /
// pp_local_plan_grids; local_planner.py states the rule): a window of nv * nw (v, w) samples rolled forward from one pose
// per grid, each scored on the field, and the least key's sample as the command.  Integer adds, multiplies, shifts,
// compares and minima only; cos and sin are looked up in a table the host made.  Two kernels:
//   rollout  grid x = chunks of LOC_BLOCK samples, grid y = grid index, lane = sample.  The workgroup stages the trig table
//            in LDS (16 KiB: C and S are int16 halves of one word); a lane walks its steps with one LDS read and one byte
//            load of the grid per step, X, Y, h and occ in registers.  A sample that leaves the grid or meets a blocked
//            cell ENDS: the lane loads nothing more, but it never leaves the loop's wave-wide vote nor the reductions
//            behind it -- no lane returns once the stream's state is known, and that state is the same in every lane of
//            the launch's workgroups of a grid.  Each lane forms its key (2^64 - 1: invalid) and stores it if asked; the
//            wave's least key comes from lane shuffles, the workgroup's goes to its slot of `partial`; the reason counts
//            are ballot popcounts, one integer atomic per wave and reason.
//   finish   one wave per grid: the least of the partial keys (lane = chunk), the result words, and the winner rolled
//            once more by lane 0 to write its trajectory.
// Keys are unique (the sample index is their low 14 bits), so the minimum does not depend on any order; the counts are
// integer sums.  No cooperative launch, no workgroup waits on another's memory, no float atomics.  Every loop is bounded
// by an argument the host has checked (api_local_plan.hip).
//
// MOVERS (pp_local_plan_movers_async, pp_local_plan_grids_movers): rollout and finish are templates on <bool MOVERS>, and
// the instantiation without them is the code above, unchanged.  With them the workgroup also stages the grid's table of at
// most 64 movers in LDS (1.5 KiB) behind a cull by its first wave (lane = mover): the robot moves at most 1024 sub-cells
// along an axis per step, so a mover farther than 1024 * k + r_soft from the start pose along either axis at every step k
// <= min(steps, horizon) touches no sample and is dropped -- no result depends on it.  A lane that is alive behind the
// static test of step k <= horizon walks the staged movers (every lane reads the same entry: an LDS broadcast), rejects
// one on 32-bit |dx| > r_soft || |dy| > r_soft, behind which d2 fits 32 bits; d2 <= r_hard^2 ends it as DYNAMIC exactly as
// a blocked cell would, d2 <= r_soft^2 raises its `near`.  Finish recomputes the winner's near on the whole table, a
// mover per lane.  The
// table itself comes from the host (pp_local_plan_grids_movers) or from the track slots (k_local_movers, local_movers.hip:
// the one place of the stage that is not integer arithmetic, and so a file of its own).
//
// FOOTPRINT (pp_set_local_footprint, pp_local_plan_grids_footprint): the bodies of rollout and finish carry a second flag,
// <bool MOVERS, bool FOOT>, four instantiations; the two without a footprint are the code above, unchanged, under their
// old launch names.  With one, the workgroup also stages the probe table in LDS (256 words of two int16 halves: 1 KiB) and
// a sample is rolled by a GROUP of LOC_FOOT_GROUP neighbouring lanes of one wave instead of one lane: X, Y, h, occ and
// near are replicated in the group (every lane of it takes the same step and reads the same centre cell), and behind the
// centre's static test lane j of the group walks the probes q = j, j + G, ... under the heading after the step's turn,
// stopping at its first probe that is not free.  The group's verdict is the minimum of (q << 1) | blocked over its lanes
// by lane shuffles (all ones: every probe free), taken by every lane of the wave at once, so the FIRST failing probe of
// the table decides OUTSIDE against FOOTPRINT as the rule's table order does.  A workgroup rolls LOC_BLOCK / G samples;
// the workgroups of one chunk of LOC_BLOCK samples lower the chunk's slot of `partial` (all ones before the launch) with
// one 64-bit integer atomic min each -- keys are unique, so the order does not matter -- and finish reads the slots as
// before.  The group's first lane alone stores the key and counts.  State 5 and start_probe come from loc_foot_start in
// both kernels: a lane takes a probe, a ballot, the lowest set bit, 64 probes a trip; each wave of the rollout runs it on
// its own and gets the same answer.  The winner's re-roll in finish tests no probe: the winner passed them all.
#include "pp_common.h"

namespace {

constexpr unsigned LOC_U = PP_NAVFN_UNREACHED;
constexpr unsigned long long LOC_INVALID = ~0ull;
constexpr int LOC_SHIFT = 10, LOC_HMASK = PP_LOCAL_HEADINGS - 1;
constexpr int LOC_R_OK = 0, LOC_R_OUTSIDE = 1, LOC_R_COLLISION = 2, LOC_R_UNREACHED = 3, LOC_R_DYNAMIC = 4;     // why a sample ended
constexpr int LOC_R_FOOTPRINT = 5;                       // ... on a blocked probe of the footprint
constexpr int LOC_FOOT_FREE = 0x7FFFFFFF;                // a verdict: no probe failed (above every (q << 1) | blocked)
constexpr int LOC_MOVER_POS = 1 << 29;                   // |mx|, |my| at most
static_assert((1 << LOC_SHIFT) == PP_LOCAL_SUB && (PP_LOCAL_HEADINGS & LOC_HMASK) == 0, "cells and ticks by shift and mask");
static_assert(PP_LOCAL_MAX_SAMPLES == (1 << 14), "a key's low 14 bits are the sample index");
static_assert(LOC_MAX_CHUNKS <= 64 && LOC_BLOCK % 64 == 0, "finish reads a grid's partial keys with one wave");
// the score: pot < 2^32 - 1 by weight <= 255, occ <= 100, 1024 - |sv| <= 1024 and |sw| <= 512 by weights <= 65535; with
// movers, near <= horizon <= PP_LOCAL_MAX_STEPS by a weight <= 65535
static_assert(255ull * 0xFFFFFFFEull + 65535ull * 100ull + 65535ull * 1024ull + 65535ull * 512ull + 65535ull * PP_LOCAL_MAX_STEPS < (1ull << 41),
              "a score stays below 2^41, so (score << 14) | s never reaches the invalid key");
// X and Y: a pose that is rolled lies in the grid (< 2^20 cells on a side), a step moves at most one cell along an axis and
// the sample ends at its first cell outside; the scored point adds the lookahead
static_assert(((long long)PP_OCC_MAX_CELLS + 1) * PP_LOCAL_SUB + PP_LOCAL_MAX_LOOKAHEAD < (1ll << 31), "X and Y fit int32");
static_assert(1024 * 16384 + 8192 < (1ll << 31) && (long long)PP_LOCAL_MAX_LOOKAHEAD * 16384 + 8192 < (1ll << 31),
              "a step's and the lookahead's product fit int32");
// a mover: its position at step k <= 256 fits int32, and so does dx = X - position, because X is only compared behind the
// static test, which left it inside the grid: 0 <= X < 2^20 cells; dx * dx + dy * dy then fits int64
constexpr long long LOC_MAX_MPOS = (long long)LOC_MOVER_POS + (long long)PP_LOCAL_MAX_STEPS * PP_LOCAL_MAX_MOVER_SPEED;
constexpr long long LOC_MAX_DX = (long long)PP_OCC_MAX_CELLS * PP_LOCAL_SUB + LOC_MAX_MPOS;
static_assert(LOC_MAX_MPOS < (1ll << 31) && LOC_MAX_DX < (1ll << 31), "a mover's position and dx fit int32");
static_assert(LOC_MAX_DX < (1ll << 31) && 2 * (LOC_MAX_DX * LOC_MAX_DX) < (1ull << 63), "d2 fits int64");
static_assert((long long)PP_LOCAL_MAX_MOVER_RADIUS * PP_LOCAL_MAX_MOVER_RADIUS < (1ll << 31), "r * r fits int32");
static_assert(PP_LOCAL_MAX_MOVERS == 64 && PP_WAVE == 64, "the cull: one lane per mover");
static_assert(PP_LOCAL_MAX_STEPS * 1024 + PP_LOCAL_MAX_MOVER_RADIUS < (1 << 30), "the cull's bound fits int32");
// a probe: |fx|, |fy| <= 32767 are int16 halves of one word; its rotation fx * C - fy * S (and fx * S + fy * C) with |C|,
// |S| <= 16384 fits int32, and so does X + rx: a pose whose probes are looked at lies in the grid
static_assert(PP_LOCAL_MAX_PROBE == 32767 && PP_LOCAL_MAX_PROBES == 256, "a probe is two int16; 256 of them are 1 KiB of LDS");
static_assert(32767ll * 16384 * 2 + 8192 < (1ll << 31), "a probe's rotation fits int32");
static_assert(((long long)PP_OCC_MAX_CELLS + 1) * PP_LOCAL_SUB + 2ll * PP_LOCAL_MAX_PROBE + 1 < (1ll << 31), "X + rx and Y + ry fit int32");
static_assert(((PP_LOCAL_MAX_PROBES - 1) << 1 | 1) < LOC_FOOT_FREE, "every failing verdict lies below the free one");
static_assert(LOC_FOOT_GROUP >= 1 && LOC_FOOT_GROUP <= PP_WAVE && (LOC_FOOT_GROUP & (LOC_FOOT_GROUP - 1)) == 0 && LOC_BLOCK % LOC_FOOT_GROUP == 0,
              "a group is a power of two of neighbouring lanes of one wave, and the groups of a workgroup lie in one chunk");
static_assert(PP_LOCAL_FOOT_INFO == 4 && LOC_F_RESERVED == 3, "a grid's footprint words are the foot_info fields");

__device__ __forceinline__ int loc_round(int a) { return (a + 8192) >> 14; }         // (arithmetic shift: floor)
__device__ __forceinline__ int loc_cos(unsigned t) { return (int)(short)(t & 0xFFFFu); }
__device__ __forceinline__ int loc_sin(unsigned t) { return (int)t >> 16; }

// what the rule reads of cell (cx, cy): -2 outside the grid, -1 blocked, else the value occ takes
__device__ __forceinline__ int loc_cell(const LocalParams& p, const int8_t* grid, bool known, int cx, int cy) {
    if (cx < 0 || cx >= p.width || cy < 0 || cy >= p.height) return -2;
    const int g = known ? (int)grid[(size_t)cy * p.pitch + cx] : -1;
    if (g >= p.lethal) return -1;
    if (g < 0) return p.allow_unknown ? p.unknown_cost : -1;
    return g;
}

// the part of cmd_state that needs no sample: 4, 3, 2 or 0 -- the same in every lane of every workgroup of grid b
__device__ __forceinline__ int loc_stream_state(const LocalParams& p, int b, const LocalCall& c, const int8_t* grid,
                                                const unsigned* pot, bool known) {
    if ((c.flags & LOC_NO_GOAL) || (p.nav_state && p.nav_state[NAV_GOAL_STATE * p.nav_state_stride + b] != 0)) return 4;
    const int cx = c.X >> LOC_SHIFT, cy = c.Y >> LOC_SHIFT;
    if (loc_cell(p, grid, known, cx, cy) < 0) return 3;
    const unsigned v = pot[(size_t)cy * p.pitch + cx];
    return v == LOC_U ? 3 : v == 0 ? 2 : 0;
}

__device__ __forceinline__ unsigned long long loc_wave_min(unsigned long long key) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
    }
    return key;
}

// One mover against a pose (X, Y) at step k: bit 0 within r_hard, bit 1 within r_soft.  A mover with |dx| > r_soft or
// |dy| > r_soft is rejected on those 32-bit values; what passes has |dx|, |dy| <= 32767, so d2 <= 2 * 32767^2 < 2^32 and
// needs no 64-bit product at all (for a rejected mover the unsigned products may wrap: they are not looked at).  The
// rollout's staged table ends in entries with r_soft = -1, which nothing passes.
static_assert(2ull * PP_LOCAL_MAX_MOVER_RADIUS * PP_LOCAL_MAX_MOVER_RADIUS < (1ull << 32), "d2 of a mover that passes the reject fits 32 bits");
__device__ __forceinline__ unsigned loc_mover_test(int mx, int my, int mvx, int mvy, int rh, int rs, int X, int Y, int k) {
    const int dx = X - (mx + k * mvx), dy = Y - (my + k * mvy);
    const bool in = abs(dx) <= rs && abs(dy) <= rs;
    const unsigned d2 = (unsigned)dx * (unsigned)dx + (unsigned)dy * (unsigned)dy;
    return ((in & (d2 <= (unsigned)(rh * rh))) ? 1u : 0u) | ((in & (d2 <= (unsigned)(rs * rs))) ? 2u : 0u);
}

// The movers' test of a pose (X, Y) that passed the static test of step k, 1 <= k <= horizon, against the n entries of
// the staged table, four at a time (their LDS reads issue together; the table is padded to a multiple of four): true if
// one ends the sample, else *near raised -- by the same amount whichever mover came near, so one flag per step serves.
__device__ __forceinline__ bool loc_movers_hit(const int* mv, int n, int X, int Y, int k, int horizon, int* near) {
    unsigned seen = 0;
    for (int m0 = 0; m0 < n; m0 += 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int* e = mv + 6 * (m0 + j);
            seen |= loc_mover_test(e[0], e[1], e[2], e[3], e[4], e[5], X, Y, k);
        }
        if (seen & 1u) return true;
    }
    if (seen & 2u) *near = max(*near, horizon + 1 - k);
    return false;
}

// What the rule reads of the cell of probe word w at the pose (X, Y) under the heading whose table word is t: -1 free, 0
// outside the grid, 1 blocked -- so (q << 1) | answer is probe q's verdict where it is not free.
__device__ __forceinline__ int loc_probe(const LocalParams& p, const int8_t* grid, bool known, unsigned w, unsigned t, int X, int Y) {
    const int fx = (int)(short)(w & 0xFFFFu), fy = (int)w >> 16, C = loc_cos(t), S = loc_sin(t);
    const int cx = (X + loc_round(fx * C - fy * S)) >> LOC_SHIFT, cy = (Y + loc_round(fx * S + fy * C)) >> LOC_SHIFT;
    if (cx < 0 || cx >= p.width || cy < 0 || cy >= p.height) return 0;
    const int g = known ? (int)grid[(size_t)cy * p.pitch + cx] : -1;
    return (g >= p.foot_lethal || (g < 0 && !p.allow_unknown)) ? 1 : -1;
}

// The first probe that is not free at the start pose (which lies in the grid: the stream's state is 0), -1 if none: a
// lane takes a probe, 64 a trip.  The whole wave is here, and every lane returns the same answer.
__device__ __forceinline__ int loc_foot_start(const LocalParams& p, const LocalCall& c, const int8_t* grid, bool known, int lane) {
    const unsigned t = p.trig[c.h & LOC_HMASK];
    for (int q0 = 0; q0 < p.n_probes; q0 += 64) {
        const int q = q0 + lane;
        const bool bad = q < p.n_probes && loc_probe(p, grid, known, p.probes[q], t, c.X, c.Y) >= 0;
        const unsigned long long m = __ballot(bad);
        if (m) return q0 + __ffsll((long long)m) - 1;
    }
    return -1;
}

template <bool MOVERS, bool FOOT>
__device__ __forceinline__ void loc_rollout(const LocalParams& p) {
    constexpr int G = FOOT ? LOC_FOOT_GROUP : 1, PER = LOC_BLOCK / G;       // lanes of a sample, samples of a workgroup
    __shared__ unsigned s_trig[PP_LOCAL_HEADINGS];
    __shared__ unsigned long long s_min[LOC_BLOCK / 64];
    __shared__ int s_mov[MOVERS ? PP_LOCAL_MAX_MOVERS * 6 : 1];
    __shared__ int s_nmov;
    __shared__ unsigned s_probe[FOOT ? PP_LOCAL_MAX_PROBES : 1];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = tid & (G - 1);                       // the lane's place in its sample's group (0: it stores and counts)
    const LocalCall c = p.call[b];
    const int8_t* grid = p.grid + (size_t)b * p.stride;
    const unsigned* pot = p.pot + (size_t)b * p.stride;
    const bool known = !p.nav_call || (p.nav_call[b].flags & NAV_KNOWN) != 0;
    const int n = p.nv * p.nw, s = (int)blockIdx.x * PER + tid / G;
    const bool live = s < n, lead = live && sub == 0;
    unsigned long long* partial = p.partial + (size_t)b * LOC_MAX_CHUNKS + blockIdx.x / G;
    if constexpr (FOOT) {                                // states 4, 3, 2, then 5: no sample is rolled (the whole workgroup returns)
        const int state = loc_stream_state(p, b, c, grid, pot, known);
        if (state >= 2 || loc_foot_start(p, c, grid, known, lane) >= 0) {
            if (p.keys && lead) p.keys[(size_t)b * n + s] = LOC_INVALID;
            return;                                      // (the chunk's slot of `partial` holds all ones already)
        }
    } else if (loc_stream_state(p, b, c, grid, pot, known) >= 2) {      // no sample is rolled (the whole workgroup returns)
        if (p.keys && live) p.keys[(size_t)b * n + s] = LOC_INVALID;
        if (tid == 0) *partial = LOC_INVALID;
        return;
    }
    for (int i = tid; i < PP_LOCAL_HEADINGS; i += LOC_BLOCK) s_trig[i] = p.trig[i];
    if (FOOT)
        for (int i = tid; i < p.n_probes; i += LOC_BLOCK) s_probe[i] = p.probes[i];
    if (MOVERS && wave == 0) {                           // the cull: lane = mover (the whole first wave is here)
        const int nm = min(max(p.mover_info[LOC_M_COUNT * p.state_stride + b], 0), PP_LOCAL_MAX_MOVERS);
        const int* e = p.movers + ((size_t)b * PP_LOCAL_MAX_MOVERS + lane) * 6;
        int m[6] = {0, 0, 0, 0, 0, 0};
        bool keep = false;
        if (lane < nm) {
#pragma unroll
            for (int q = 0; q < 6; ++q) m[q] = e[q];
            const int kmax = min(p.steps, p.horizon);
            for (int k = 1; k <= kmax && !keep; ++k) {
                const int reach = 1024 * k + m[5];
                keep = abs(c.X - (m[0] + k * m[2])) <= reach && abs(c.Y - (m[1] + k * m[3])) <= reach;
            }
        }
        const unsigned long long kept = __ballot(keep);
        const int cnt = __popcll(kept);
        if (keep) {
            int* d = s_mov + 6 * __popcll(kept & ((1ull << lane) - 1ull));
#pragma unroll
            for (int q = 0; q < 6; ++q) d[q] = m[q];
        }
        if (lane >= cnt) {                               // behind the kept ones: entries that nothing passes
#pragma unroll
            for (int q = 0; q < 6; ++q) s_mov[6 * lane + q] = q < 4 ? 0 : -1;
        }
        if (lane == 0) s_nmov = cnt;
    }
    __syncthreads();
    const int nmov = MOVERS ? s_nmov : 0;

    const int sv = c.v0 + (live ? s / p.nw : 0) * c.dv, sw = c.w0 + (live ? s % p.nw : 0) * c.dw;
    int X = c.X, Y = c.Y, h = c.h & LOC_HMASK, occ = 0, near = 0;
    int reason = LOC_R_OK;
    bool alive = live;                                   // an ended lane loads nothing more and stays in the wave
    for (int k = 0; k < p.steps; ++k) {
        int bad = LOC_FOOT_FREE;                         // with a footprint: this lane's first probe that is not free
        if (alive) {
            const unsigned t = s_trig[h];
            X += loc_round(sv * loc_cos(t));
            Y += loc_round(sv * loc_sin(t));
            h = (h + sw) & LOC_HMASK;
            const int g = loc_cell(p, grid, known, X >> LOC_SHIFT, Y >> LOC_SHIFT);
            if (g < 0) { reason = g == -2 ? LOC_R_OUTSIDE : LOC_R_COLLISION; alive = false; }
            else {
                occ = max(occ, g);
                if (!FOOT && MOVERS && k < p.horizon && loc_movers_hit(s_mov, nmov, X, Y, k + 1, p.horizon, &near)) {
                    reason = LOC_R_DYNAMIC;
                    alive = false;
                }
                if (FOOT) {                              // the lane's share of the probes, under the heading after the turn
                    const unsigned th = s_trig[h];
                    for (int q = sub; q < p.n_probes && bad == LOC_FOOT_FREE; q += G) {
                        const int r = loc_probe(p, grid, known, s_probe[q], th, X, Y);
                        if (r >= 0) bad = (q << 1) | r;
                    }
                }
            }
        }
        if (FOOT) {                                      // the group's verdict: every lane of the wave is here
#pragma unroll
            for (int m = G / 2; m >= 1; m >>= 1) bad = min(bad, __shfl_xor(bad, m));
            if (bad != LOC_FOOT_FREE) { reason = (bad & 1) ? LOC_R_FOOTPRINT : LOC_R_OUTSIDE; alive = false; }
            else if (MOVERS && alive && k < p.horizon && loc_movers_hit(s_mov, nmov, X, Y, k + 1, p.horizon, &near)) {
                reason = LOC_R_DYNAMIC;
                alive = false;
            }
        }
        if (!__any(alive)) break;                        // (the same answer in every lane of the wave)
    }
    unsigned long long key = LOC_INVALID;
    if (alive) {                                         // every step taken: the scored point
        const unsigned t = s_trig[h];
        const int lx = X + loc_round(p.lookahead * loc_cos(t)), ly = Y + loc_round(p.lookahead * loc_sin(t));
        const int cx = lx >> LOC_SHIFT, cy = ly >> LOC_SHIFT;
        unsigned v = LOC_U;
        if (loc_cell(p, grid, known, cx, cy) >= 0) v = pot[(size_t)cy * p.pitch + cx];
        if (v == LOC_U) reason = LOC_R_UNREACHED;
        else {
            unsigned long long score = (unsigned long long)p.pot_w * v + (unsigned long long)(p.occ_w * occ) +
                                       (unsigned long long)(p.speed_w * (1024 - abs(sv))) + (unsigned long long)(p.turn_w * abs(sw));
            if (MOVERS) score += (unsigned long long)(p.mover_w * near);
            key = (score << 14) | (unsigned)s;
        }
    }
    if (p.keys && lead) p.keys[(size_t)b * n + s] = key;

    int* st = p.state + b;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cnt = __popcll(__ballot(lead && reason == r));
        if (lane == 0 && cnt) atomicAdd(st + (LOC_N_OK + r) * p.state_stride, cnt);
    }
    if (MOVERS) {
        const int cnt = __popcll(__ballot(lead && reason == LOC_R_DYNAMIC));
        if (lane == 0 && cnt) atomicAdd(p.mover_info + LOC_M_DYNAMIC * p.state_stride + b, cnt);
    }
    if (FOOT) {
        const int cnt = __popcll(__ballot(lead && reason == LOC_R_FOOTPRINT));
        if (lane == 0 && cnt) atomicAdd(p.foot_info + LOC_F_FOOTPRINT * p.state_stride + b, cnt);
    }
    key = loc_wave_min(key);
    if (lane == 0) s_min[wave] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < LOC_BLOCK / 64; ++w) key = s_min[w] < key ? s_min[w] : key;
        if (FOOT) atomicMin(partial, key);               // (one of the chunk's G workgroups)
        else *partial = key;
    }
}

template <bool MOVERS>
__global__ __launch_bounds__(LOC_BLOCK) void k_local_rollout(LocalParams p) { loc_rollout<MOVERS, false>(p); }
template <bool MOVERS>
__global__ __launch_bounds__(LOC_BLOCK) void k_local_rollout_foot(LocalParams p) { loc_rollout<MOVERS, true>(p); }

template <bool MOVERS, bool FOOT>
__device__ __forceinline__ void loc_finish(const LocalParams& p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const LocalCall c = p.call[b];
    const int8_t* grid = p.grid + (size_t)b * p.stride;
    const unsigned* pot = p.pot + (size_t)b * p.stride;
    const bool known = !p.nav_call || (p.nav_call[b].flags & NAV_KNOWN) != 0;
    const int n = p.nv * p.nw, chunks = (n + LOC_BLOCK - 1) / LOC_BLOCK, ss = p.state_stride;
    int state = loc_stream_state(p, b, c, grid, pot, known);
    if (FOOT) {                                          // state 5 and start_probe, as the rollout's workgroups found them
        const int start = state == 0 ? loc_foot_start(p, c, grid, known, lane) : -1;
        if (start >= 0) state = 5;
        if (lane == 0) {
            p.foot_info[LOC_F_COUNT * ss + b] = p.n_probes;
            p.foot_info[LOC_F_START * ss + b] = start;
            p.foot_info[LOC_F_RESERVED * ss + b] = 0;
        }
    }
    unsigned long long key = state == 0 && lane < chunks ? p.partial[(size_t)b * LOC_MAX_CHUNKS + lane] : LOC_INVALID;
    key = loc_wave_min(key);
    if (state == 0 && key == LOC_INVALID) state = 1;
    int* st = p.state + b;
    const int words = (p.steps + 1) * 3;
    int* traj = p.traj + (size_t)b * words;
    if (state != 0) {                                    // (the same answer in every lane)
        for (int i = lane; i < words; i += 64) traj[i] = 0;
        if (lane == 0) {
            st[LOC_CMD_STATE * ss] = state;
            st[LOC_BEST * ss] = -1;
            st[LOC_SV * ss] = 0;
            st[LOC_SW * ss] = 0;
            p.score[b] = 0;
            if (MOVERS) p.mover_info[LOC_M_NEAR * ss + b] = 0;
        }
        return;
    }
    // Without movers lane 0 alone rolls the winner.  With them every lane rolls it, the same values in each, and lane m
    // holds mover m of the grid's whole table against it: the winner's near is the wave's greatest.
    if (!MOVERS && lane != 0) return;
    const int s = (int)(key & (PP_LOCAL_MAX_SAMPLES - 1));
    const int sv = c.v0 + (s / p.nw) * c.dv, sw = c.w0 + (s % p.nw) * c.dw;
    if (lane == 0) {
        st[LOC_CMD_STATE * ss] = 0;
        st[LOC_BEST * ss] = s;
        st[LOC_SV * ss] = sv;
        st[LOC_SW * ss] = sw;
        p.score[b] = key >> 14;
    }
    int m[6] = {0, 0, 0, 0, -1, -1};
    if (MOVERS && lane < min(max(p.mover_info[LOC_M_COUNT * ss + b], 0), PP_LOCAL_MAX_MOVERS)) {
        const int* e = p.movers + ((size_t)b * PP_LOCAL_MAX_MOVERS + lane) * 6;
#pragma unroll
        for (int q = 0; q < 6; ++q) m[q] = e[q];
    }
    int X = c.X, Y = c.Y, h = c.h & LOC_HMASK, near = 0;
    if (lane == 0) { traj[0] = X; traj[1] = Y; traj[2] = h; }
    for (int k = 1; k <= p.steps; ++k) {                 // the winner took every step inside the grid
        const unsigned t = p.trig[h];
        X += loc_round(sv * loc_cos(t));
        Y += loc_round(sv * loc_sin(t));
        h = (h + sw) & LOC_HMASK;
        if (lane == 0) { traj[3 * k] = X; traj[3 * k + 1] = Y; traj[3 * k + 2] = h; }
        if (MOVERS && k <= p.horizon && (loc_mover_test(m[0], m[1], m[2], m[3], m[4], m[5], X, Y, k) & 2u))     // (none ended it)
            near = max(near, p.horizon + 1 - k);
    }
    if (MOVERS) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) near = max(near, __shfl_xor(near, d));
        if (lane == 0) p.mover_info[LOC_M_NEAR * ss + b] = near;
    }
}

template <bool MOVERS>
__global__ __launch_bounds__(64) void k_local_finish(LocalParams p) { loc_finish<MOVERS, false>(p); }
template <bool MOVERS>
__global__ __launch_bounds__(64) void k_local_finish_foot(LocalParams p) { loc_finish<MOVERS, true>(p); }

}  // namespace

void launch_local_rollout(const LocalParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int chunks = (p.nv * p.nw + LOC_BLOCK - 1) / LOC_BLOCK;
    if (p.probes) {                                      // a workgroup rolls LOC_BLOCK / LOC_FOOT_GROUP samples
        const int groups = (p.nv * p.nw + LOC_BLOCK / LOC_FOOT_GROUP - 1) / (LOC_BLOCK / LOC_FOOT_GROUP);
        if (p.movers) PP_LAUNCH("k_local_rollout_movers_foot", k_local_rollout_foot<true>, dim3(groups, p.batch), dim3(LOC_BLOCK), 0, s, p);
        else PP_LAUNCH("k_local_rollout_foot", k_local_rollout_foot<false>, dim3(groups, p.batch), dim3(LOC_BLOCK), 0, s, p);
    } else if (p.movers) PP_LAUNCH("k_local_rollout_movers", k_local_rollout<true>, dim3(chunks, p.batch), dim3(LOC_BLOCK), 0, s, p);
    else PP_LAUNCH("k_local_rollout", k_local_rollout<false>, dim3(chunks, p.batch), dim3(LOC_BLOCK), 0, s, p);
}

void launch_local_finish(const LocalParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    if (p.probes) {
        if (p.movers) PP_LAUNCH("k_local_finish_movers_foot", k_local_finish_foot<true>, dim3(p.batch), dim3(64), 0, s, p);
        else PP_LAUNCH("k_local_finish_foot", k_local_finish_foot<false>, dim3(p.batch), dim3(64), 0, s, p);
    } else if (p.movers) PP_LAUNCH("k_local_finish_movers", k_local_finish<true>, dim3(p.batch), dim3(64), 0, s, p);
    else PP_LAUNCH("k_local_finish", k_local_finish<false>, dim3(p.batch), dim3(64), 0, s, p);
}
