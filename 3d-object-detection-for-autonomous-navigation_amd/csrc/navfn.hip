// Navigation function over an int8 OccupancyGrid (pp_set_navfn / pp_navfn_async / pp_navfn_grids; navfn.py states the
// rule): the cost-to-go field from one goal cell per grid, and the path that descends it from a start cell.  Integer adds,
// multiplies, compares and minima only.  Three kernels, grid y = grid index whatever the batch:
//   init     the cell costs (uint16, 0 = blocked) from the grid, both potential buffers UNREACHED except 0 at a valid
//            goal, the grid's flags and counters
//   relax    one ROUND.  A workgroup owns a tile of 32 x 32 cells: it stages the tile and a one-cell halo of potentials
//            and costs in LDS (6.8 KiB), relaxes the tile there against the frozen halo until a __syncthreads_or says
//            nothing moved -- at most cells + 1 iterations, each finalises a cell -- and writes every cell of the tile to
//            the OTHER potential buffer: round r reads pot[r & 1] (tile and halo) and writes pot[(r + 1) & 1], so no
//            workgroup reads what another writes in the same launch.  A tile that changed a cell adds to its grid's
//            `changed` slot of this round; the slots rotate over three by round index (this round's is written, the last
//            round's read, the next round's cleared), and the workgroups of a grid whose last round changed nothing return
//            at once -- its two buffers are then equal, and stay so.
//   finish   `reached` by ballot popcounts and one integer atomic per wave; one wave per grid walks the path: lanes 0 .. 7
//            load the eight neighbours, a minimum over (value, lane) picks the step -- the first neighbour in the rule's
//            order on a tie -- and the walk is bounded by max_path.
// The field is the unique fixed point of the relaxation (every cost is positive), so neither the tiling nor the order in
// which lanes see each other's LDS writes nor the number of rounds shows in a byte of it.  A potential read while another
// lane lowers it is the old or the new value, and either is the length of a real chain of moves.  No potential can
// overflow: a step costs at most 7 * 550 and a chain never visits a cell twice (pp_hip.h).  Every loop has a compile-time
// or argument bound; the host decides how many rounds run (api_navfn.hip).
#include "pp_common.h"

namespace {

constexpr int NAV_TW = 32, NAV_TH = 32, NAV_BLOCK = 256;
constexpr int NAV_LW = NAV_TW + 2, NAV_LH = NAV_TH + 2;          // the tile and its halo
constexpr int NAV_CPT = NAV_TW * NAV_TH / NAV_BLOCK;             // cells of a lane: a column of NAV_CPT rows
constexpr unsigned NAV_U = PP_NAVFN_UNREACHED;
constexpr int NAV_A = 5, NAV_D = 7;
static_assert(NAV_TW <= 64 && NAV_TH <= 64, "a tile is at most 64 cells on a side");
static_assert(NAV_BLOCK % NAV_TW == 0 && NAV_CPT * NAV_BLOCK == NAV_TW * NAV_TH, "a lane owns a column of NAV_CPT rows");
static_assert(NAV_LW * NAV_LH * 6 <= 8192, "the staged tile stays under 8 KiB of LDS");
static_assert(7ull * 550ull * (unsigned long long)PP_OCC_MAX_CELLS < 0xFFFFFFFFull, "a uint32 potential cannot overflow");

// neighbour l of the rule's order E N W S NE NW SW SE: two bits per entry hold dx + 1 and dy + 1
__device__ __forceinline__ int nav_dx(int l) { return ((0x8246 >> (2 * l)) & 3) - 1; }
__device__ __forceinline__ int nav_dy(int l) { return ((0x0A19 >> (2 * l)) & 3) - 1; }

__device__ __forceinline__ int nav_cost(int g, const NavParams& p) {
    if (g >= p.lethal) return 0;
    if (g < 0) return p.allow_unknown ? p.neutral + p.factor * p.unknown_cost : 0;
    return p.neutral + p.factor * g;
}

__global__ __launch_bounds__(NAV_BLOCK) void k_navfn_init(NavParams p) {
    const int b = blockIdx.y;
    const int W = p.width, H = p.height;
    const NavCall c = p.call[b];
    const bool known = (c.flags & NAV_KNOWN) != 0;
    const int8_t* grid = p.grid + (size_t)b * p.stride;
    const int n = p.pitch * H, i = (int)blockIdx.x * NAV_BLOCK + (int)threadIdx.x;
    if (i < n) {
        const int x = i % p.pitch, y = i / p.pitch;
        const int cost = x < W ? nav_cost(known ? (int)grid[i] : -1, p) : 0;     // right of the width: no cell
        const unsigned v = cost && x == c.gx && y == c.gy ? 0u : NAV_U;
        const size_t at = (size_t)b * p.stride + i;
        p.cost[at] = (uint16_t)cost;
        p.pot[0][at] = v;
        p.pot[1][at] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int* st = p.state + b;
        const int ss = p.state_stride;
        int gs = 2;
        if (c.gx >= 0 && c.gx < W && c.gy >= 0 && c.gy < H)
            gs = nav_cost(known ? (int)grid[(size_t)c.gy * p.pitch + c.gx] : -1, p) ? 0 : 1;
        for (int k = 0; k < 3; ++k) st[(NAV_CHANGED + k) * ss] = 0;
        st[NAV_ROUNDS * ss] = 0;
        st[NAV_REACHED * ss] = 0;
        st[NAV_GOAL_STATE * ss] = gs;
        st[NAV_PATH_STATE * ss] = 4;
        st[NAV_PATH_LEN * ss] = 0;
    }
}

__global__ __launch_bounds__(NAV_BLOCK) void k_navfn_relax(NavParams p, int round) {
    __shared__ unsigned s_pot[NAV_LH * NAV_LW];
    __shared__ unsigned short s_c[NAV_LH * NAV_LW];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int W = p.width, H = p.height, ss = p.state_stride;
    int* st = p.state + b;
    const int cur = round % 3, nxt = (round + 1) % 3, prv = (round + 2) % 3;
    if (blockIdx.x == 0 && tid == 0) st[(NAV_CHANGED + nxt) * ss] = 0;       // nobody reads or adds to that slot in this launch
    if (round > 0 && st[(NAV_CHANGED + prv) * ss] == 0) return;             // the field stands (the same answer in every lane)
    if (blockIdx.x == 0 && tid == 0) st[NAV_ROUNDS * ss] += 1;

    const int tiles_x = (W + NAV_TW - 1) / NAV_TW;
    const int x0 = ((int)blockIdx.x % tiles_x) * NAV_TW, y0 = ((int)blockIdx.x / tiles_x) * NAV_TH;
    const unsigned* pin = p.pot[round & 1] + (size_t)b * p.stride;
    unsigned* pout = p.pot[(round + 1) & 1] + (size_t)b * p.stride;
    const uint16_t* cost = p.cost + (size_t)b * p.stride;
    for (int i = tid; i < NAV_LH * NAV_LW; i += NAV_BLOCK) {
        const int gx = x0 - 1 + i % NAV_LW, gy = y0 - 1 + i / NAV_LW;
        const bool inside = gx >= 0 && gx < W && gy >= 0 && gy < H;
        const size_t at = inside ? (size_t)gy * p.pitch + gx : 0;
        s_pot[i] = inside ? pin[at] : NAV_U;                                 // a cell outside the grid does not exist
        s_c[i] = inside ? cost[at] : (uint16_t)0;
    }
    __syncthreads();

    // this lane's cells: column lx, rows ly0 .. ly0 + NAV_CPT - 1 of the staged tile
    const int lx = 1 + (tid % NAV_TW), ly0 = 1 + (tid / NAV_TW) * NAV_CPT;
    unsigned first[NAV_CPT];
    int wa[NAV_CPT], wd[NAV_CPT], diag[NAV_CPT];         // the step weights times c(p) (0: blocked), the admissible diagonals
#pragma unroll
    for (int k = 0; k < NAV_CPT; ++k) {
        const int li = (ly0 + k) * NAV_LW + lx;
        const int c = s_c[li];
        first[k] = s_pot[li];
        wa[k] = NAV_A * c;
        wd[k] = NAV_D * c;
        const bool e = s_c[li + 1] != 0, w = s_c[li - 1] != 0, n = s_c[li + NAV_LW] != 0, s = s_c[li - NAV_LW] != 0;
        diag[k] = p.conn == 8 ? (e && n ? 1 : 0) | (w && n ? 2 : 0) | (w && s ? 4 : 0) | (e && s ? 8 : 0) : 0;
    }
    volatile unsigned* vp = s_pot;                       // other lanes lower these between the barriers
    for (int it = 0; it <= NAV_TW * NAV_TH; ++it) {
        int moved = 0;
#pragma unroll
        for (int k = 0; k < NAV_CPT; ++k) {
            if (!wa[k]) continue;
            const int li = (ly0 + k) * NAV_LW + lx;
            const unsigned was = vp[li];
            unsigned best = was, v;
            v = vp[li + 1];          if (v != NAV_U) best = min(best, v + (unsigned)wa[k]);
            v = vp[li + NAV_LW];     if (v != NAV_U) best = min(best, v + (unsigned)wa[k]);
            v = vp[li - 1];          if (v != NAV_U) best = min(best, v + (unsigned)wa[k]);
            v = vp[li - NAV_LW];     if (v != NAV_U) best = min(best, v + (unsigned)wa[k]);
            if (diag[k] & 1) { v = vp[li + NAV_LW + 1]; if (v != NAV_U) best = min(best, v + (unsigned)wd[k]); }
            if (diag[k] & 2) { v = vp[li + NAV_LW - 1]; if (v != NAV_U) best = min(best, v + (unsigned)wd[k]); }
            if (diag[k] & 4) { v = vp[li - NAV_LW - 1]; if (v != NAV_U) best = min(best, v + (unsigned)wd[k]); }
            if (diag[k] & 8) { v = vp[li - NAV_LW + 1]; if (v != NAV_U) best = min(best, v + (unsigned)wd[k]); }
            if (best < was) { vp[li] = best; moved = 1; }
        }
        if (!__syncthreads_or(moved)) break;
    }

    int changed = 0;
#pragma unroll
    for (int k = 0; k < NAV_CPT; ++k) {
        const int gx = x0 + lx - 1, gy = y0 + ly0 - 1 + k;
        if (gx < W && gy < H) {
            const unsigned v = s_pot[(ly0 + k) * NAV_LW + lx];
            pout[(size_t)gy * p.pitch + gx] = v;
            changed |= v != first[k];
        }
    }
    if (__syncthreads_or(changed) && tid == 0) atomicAdd(st + (NAV_CHANGED + cur) * ss, 1);
}

__global__ __launch_bounds__(NAV_BLOCK) void k_navfn_finish(NavParams p, int buf) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int W = p.width, H = p.height, ss = p.state_stride;
    const unsigned* pot = p.pot[buf] + (size_t)b * p.stride;
    const uint16_t* cost = p.cost + (size_t)b * p.stride;
    int* st = p.state + b;
    int n_reached = 0;
    for (int y = (int)blockIdx.x * (NAV_BLOCK / 64) + wave; y < H; y += (int)gridDim.x * (NAV_BLOCK / 64))
        for (int xb = 0; xb < W; xb += 64) {             // (the same trip count in every lane of a wave)
            const int x = xb + lane;
            n_reached += __popcll(__ballot(x < W && pot[(size_t)y * p.pitch + x] != NAV_U));
        }
    if (lane == 0 && n_reached) atomicAdd(st + NAV_REACHED * ss, n_reached);
    if (blockIdx.x != 0 || wave != 0) return;

    // the path: one wave; lane l & 7 looks at neighbour l & 7 (the lanes from 8 on repeat the first eight)
    const NavCall c = p.call[b];
    int* path = p.paths + (size_t)b * p.max_path * 2;
    int state = 3, n = 0;
    if (!(c.flags & NAV_HAS_START)) state = 4;
    else if (c.sx < 0 || c.sx >= W || c.sy < 0 || c.sy >= H) state = 2;
    else if (pot[(size_t)c.sy * p.pitch + c.sx] == NAV_U) state = 1;
    else {
        const int l = lane & 7, dx = nav_dx(l), dy = nav_dy(l);
        int x = c.sx, y = c.sy;
        for (int step = 0; step < p.max_path; ++step) {
            const unsigned pv = pot[(size_t)y * p.pitch + x];
            if (lane == 0) { path[2 * n] = x; path[2 * n + 1] = y; }
            ++n;
            if (pv == 0) { state = 0; break; }
            if (n == p.max_path) break;                  // cut: state 3
            const int qx = x + dx, qy = y + dy;
            const bool in = l < p.conn && qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t at = in ? (size_t)qy * p.pitch + qx : 0;
            const unsigned qv = in ? pot[at] : NAV_U;
            const int qc = in ? (int)cost[at] : 0;
            const int pc = cost[(size_t)y * p.pitch + x];
            const int ce = __shfl(qc, 0), cn = __shfl(qc, 1), cw = __shfl(qc, 2), cs = __shfl(qc, 3);
            const bool adm = l < 4 || (l == 4 ? ce && cn : l == 5 ? cw && cn : l == 6 ? cw && cs : ce && cs);
            unsigned long long key = ~0ull;
            if (in && adm && qv != NAV_U) key = ((unsigned long long)(qv + (unsigned)((l < 4 ? NAV_A : NAV_D) * pc)) << 3) | (unsigned)l;
#pragma unroll
            for (int m = 1; m < 8; m <<= 1) {
                const unsigned long long o = __shfl_xor(key, m);
                key = o < key ? o : key;
            }
            if (key == ~0ull) { state = 1; n = 0; break; }       // no field of this grid: cannot happen behind the rounds
            x += nav_dx((int)(key & 7));
            y += nav_dy((int)(key & 7));
        }
    }
    if (lane == 0) {
        st[NAV_PATH_STATE * ss] = state;
        st[NAV_PATH_LEN * ss] = n;
    }
}

}  // namespace

int navfn_tiles(int width, int height, int* tiles_x) {
    const int tx = (width + NAV_TW - 1) / NAV_TW, ty = (height + NAV_TH - 1) / NAV_TH;
    if (tiles_x) *tiles_x = tx;
    return tx * ty;
}

void launch_navfn_init(const NavParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const int blocks = (p.pitch * p.height + NAV_BLOCK - 1) / NAV_BLOCK;
    PP_LAUNCH("k_navfn_init", k_navfn_init, dim3(blocks, p.batch), dim3(NAV_BLOCK), 0, s, p);
}

void launch_navfn_relax(const NavParams& p, int round, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_navfn_relax", k_navfn_relax, dim3(navfn_tiles(p.width, p.height, nullptr), p.batch), dim3(NAV_BLOCK), 0, s, p, round);
}

void launch_navfn_finish(const NavParams& p, int rounds, hipStream_t s) {
    if (p.batch <= 0) return;
    const int blocks = std::min(64, (p.height + NAV_BLOCK / 64 - 1) / (NAV_BLOCK / 64));
    PP_LAUNCH("k_navfn_finish", k_navfn_finish, dim3(blocks, p.batch), dim3(NAV_BLOCK), 0, s, p, rounds & 1);
}
