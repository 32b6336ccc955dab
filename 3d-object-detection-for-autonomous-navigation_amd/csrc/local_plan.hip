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
// integer sums.  No cooperative launch, no workgroup waits on another's memory, no float.  Every loop is bounded by an
// argument the host has checked (api_local_plan.hip).
#include "pp_common.h"

namespace {

constexpr unsigned LOC_U = PP_NAVFN_UNREACHED;
constexpr unsigned long long LOC_INVALID = ~0ull;
constexpr int LOC_SHIFT = 10, LOC_HMASK = PP_LOCAL_HEADINGS - 1;
constexpr int LOC_R_OK = 0, LOC_R_OUTSIDE = 1, LOC_R_COLLISION = 2, LOC_R_UNREACHED = 3;     // why a sample ended
static_assert((1 << LOC_SHIFT) == PP_LOCAL_SUB && (PP_LOCAL_HEADINGS & LOC_HMASK) == 0, "cells and ticks by shift and mask");
static_assert(PP_LOCAL_MAX_SAMPLES == (1 << 14), "a key's low 14 bits are the sample index");
static_assert(LOC_MAX_CHUNKS <= 64 && LOC_BLOCK % 64 == 0, "finish reads a grid's partial keys with one wave");
// the score: pot < 2^32 - 1 by weight <= 255, occ <= 100, 1024 - |sv| <= 1024 and |sw| <= 512 by weights <= 65535
static_assert(255ull * 0xFFFFFFFEull + 65535ull * 100ull + 65535ull * 1024ull + 65535ull * 512ull < (1ull << 41),
              "a score stays below 2^41, so (score << 14) | s never reaches the invalid key");
// X and Y: a pose that is rolled lies in the grid (< 2^20 cells on a side), a step moves at most one cell along an axis and
// the sample ends at its first cell outside; the scored point adds the lookahead
static_assert(((long long)PP_OCC_MAX_CELLS + 1) * PP_LOCAL_SUB + PP_LOCAL_MAX_LOOKAHEAD < (1ll << 31), "X and Y fit int32");
static_assert(1024 * 16384 + 8192 < (1ll << 31) && (long long)PP_LOCAL_MAX_LOOKAHEAD * 16384 + 8192 < (1ll << 31),
              "a step's and the lookahead's product fit int32");

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

__global__ __launch_bounds__(LOC_BLOCK) void k_local_rollout(LocalParams p) {
    __shared__ unsigned s_trig[PP_LOCAL_HEADINGS];
    __shared__ unsigned long long s_min[LOC_BLOCK / 64];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const LocalCall c = p.call[b];
    const int8_t* grid = p.grid + (size_t)b * p.stride;
    const unsigned* pot = p.pot + (size_t)b * p.stride;
    const bool known = !p.nav_call || (p.nav_call[b].flags & NAV_KNOWN) != 0;
    const int n = p.nv * p.nw, s = (int)blockIdx.x * LOC_BLOCK + tid;
    const bool live = s < n;
    unsigned long long* partial = p.partial + (size_t)b * LOC_MAX_CHUNKS + blockIdx.x;
    if (loc_stream_state(p, b, c, grid, pot, known) >= 2) {      // no sample is rolled (the whole workgroup returns)
        if (p.keys && live) p.keys[(size_t)b * n + s] = LOC_INVALID;
        if (tid == 0) *partial = LOC_INVALID;
        return;
    }
    for (int i = tid; i < PP_LOCAL_HEADINGS; i += LOC_BLOCK) s_trig[i] = p.trig[i];
    __syncthreads();

    const int sv = c.v0 + (live ? s / p.nw : 0) * c.dv, sw = c.w0 + (live ? s % p.nw : 0) * c.dw;
    int X = c.X, Y = c.Y, h = c.h & LOC_HMASK, occ = 0;
    int reason = LOC_R_OK;
    bool alive = live;                                   // an ended lane loads nothing more and stays in the wave
    for (int k = 0; k < p.steps; ++k) {
        if (alive) {
            const unsigned t = s_trig[h];
            X += loc_round(sv * loc_cos(t));
            Y += loc_round(sv * loc_sin(t));
            h = (h + sw) & LOC_HMASK;
            const int g = loc_cell(p, grid, known, X >> LOC_SHIFT, Y >> LOC_SHIFT);
            if (g < 0) { reason = g == -2 ? LOC_R_OUTSIDE : LOC_R_COLLISION; alive = false; }
            else occ = max(occ, g);
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
            const unsigned long long score = (unsigned long long)p.pot_w * v + (unsigned long long)(p.occ_w * occ) +
                                             (unsigned long long)(p.speed_w * (1024 - abs(sv))) + (unsigned long long)(p.turn_w * abs(sw));
            key = (score << 14) | (unsigned)s;
        }
    }
    if (p.keys && live) p.keys[(size_t)b * n + s] = key;

    int* st = p.state + b;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int cnt = __popcll(__ballot(live && reason == r));
        if (lane == 0 && cnt) atomicAdd(st + (LOC_N_OK + r) * p.state_stride, cnt);
    }
    key = loc_wave_min(key);
    if (lane == 0) s_min[wave] = key;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < LOC_BLOCK / 64; ++w) key = s_min[w] < key ? s_min[w] : key;
        *partial = key;
    }
}

__global__ __launch_bounds__(64) void k_local_finish(LocalParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const LocalCall c = p.call[b];
    const int8_t* grid = p.grid + (size_t)b * p.stride;
    const unsigned* pot = p.pot + (size_t)b * p.stride;
    const bool known = !p.nav_call || (p.nav_call[b].flags & NAV_KNOWN) != 0;
    const int n = p.nv * p.nw, chunks = (n + LOC_BLOCK - 1) / LOC_BLOCK, ss = p.state_stride;
    int state = loc_stream_state(p, b, c, grid, pot, known);
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
        }
        return;
    }
    if (lane != 0) return;
    const int s = (int)(key & (PP_LOCAL_MAX_SAMPLES - 1));
    const int sv = c.v0 + (s / p.nw) * c.dv, sw = c.w0 + (s % p.nw) * c.dw;
    st[LOC_CMD_STATE * ss] = 0;
    st[LOC_BEST * ss] = s;
    st[LOC_SV * ss] = sv;
    st[LOC_SW * ss] = sw;
    p.score[b] = key >> 14;
    int X = c.X, Y = c.Y, h = c.h & LOC_HMASK;
    traj[0] = X; traj[1] = Y; traj[2] = h;
    for (int k = 1; k <= p.steps; ++k) {                 // the winner took every step inside the grid
        const unsigned t = p.trig[h];
        X += loc_round(sv * loc_cos(t));
        Y += loc_round(sv * loc_sin(t));
        h = (h + sw) & LOC_HMASK;
        traj[3 * k] = X; traj[3 * k + 1] = Y; traj[3 * k + 2] = h;
    }
}

}  // namespace

void launch_local_rollout(const LocalParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int chunks = (p.nv * p.nw + LOC_BLOCK - 1) / LOC_BLOCK;
    PP_LAUNCH("k_local_rollout", k_local_rollout, dim3(chunks, p.batch), dim3(LOC_BLOCK), 0, s, p);
}

void launch_local_finish(const LocalParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_local_finish", k_local_finish, dim3(p.batch), dim3(64), 0, s, p);
}
