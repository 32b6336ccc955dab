// GT-database sampling into the resident frames: the first step of the reference's
// prep_pointcloud training branch (load_data.py:2702-2751; sample_all :1690-1921), restated in gt_sampler.py
// (sample_all_np), whose docstring lists the rules.  Which stored objects are candidates, and the `low` coin of every
// slot, are drawn on the host (gt_sampler.draw_candidates); everything here is decided in float64 in the reference's
// operation order (the build has -ffp-contract=off).  The database stays in device memory (pp_gtdb_load).
//
// k_gts_select   a workgroup per frame: 2-D corners of the frame's boxes and of the candidates in LDS, the candidates'
//                rows of the collision matrix as bit masks, then the ordered walk per round and class group (one
//                thread: <= 32 steps on masks).  Writes each slot's status and the survivors' plane equations.
// k_gts_count    a thread per ORIGINAL frame point, grid over (point chunk, frame): the frame's survivors are
//                wave-uniform; per survivor one ballot + popcount per wave and one integer atomic add per wave.
// k_gts_decide   one workgroup: the acceptance rule per frame (a frame without boxes: the first round that accepts
//                anything), then the new point and box offsets.
// k_gts_paste    a thread per output point: the accepted objects' points (centre added in float64, rounded once),
//                then the frame's own; each frame's first workgroup also writes the boxes / classes / flags.
#include <math.h>

#include <algorithm>

#include "pp_common.h"
#include "pp_geom.h"

namespace {

constexpr int kSelThreads = 256;
constexpr int kMaxBoxes = PP_MAX_GT_PER_FRAME + PP_GTS_MAX_CAND;
constexpr int kPending = -1;      // survived the box test; k_gts_decide settles it

static_assert(PP_GTS_MAX_CAND == 32, "the walk keeps a frame's candidates in one 32-bit mask");

__device__ __forceinline__ int slot_round(const int* cc, int slot) {
    int s0 = 0;
    for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) {
        s0 += cc[r];
        if (slot < s0) return r;
    }
    return PP_GTS_MAX_ROUNDS;
}

__global__ __launch_bounds__(kSelThreads) void k_gts_select(GtsParams p) {
    __shared__ double cx[kMaxBoxes][4], cy[kMaxBoxes][4];
    __shared__ unsigned s_row[PP_GTS_MAX_CAND];
    __shared__ unsigned s_hitframe;
    __shared__ int s_status[PP_GTS_MAX_CAND];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int G = p.cnt_in[b];
    int g0 = 0;
    for (int i = 0; i < b; ++i) g0 += p.cnt_in[i];
    const int* cc = p.cand_counts + (size_t)b * PP_GTS_MAX_ROUNDS;
    const pp_gts_cand* cand = p.cands + (size_t)b * PP_GTS_MAX_CAND;
    int NC = 0;
    for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) NC += cc[r];
    for (int g = tid; g < G; g += kSelThreads) {
        const float* q = p.gt_in + (size_t)(g0 + g) * 7;
        corners2(q[0], q[1], q[3], q[4], q[6], cx[g], cy[g]);
    }
    if (tid < NC) {
        const double* q = p.db_box + (size_t)cand[tid].object * 7;
        corners2(q[0], q[1], q[3], q[4], q[6], cx[G + tid], cy[G + tid]);
    }
    if (tid < PP_GTS_MAX_CAND) s_row[tid] = 0u;
    if (tid == 0) s_hitframe = 0u;
    __syncthreads();
    // rows of the collision matrix: candidate i against the frame's boxes and against the candidates of its round
    const int W = G + NC;
    for (int t = tid; t < NC * W; t += kSelThreads) {
        const int i = t / W, j = t - i * W;
        const int ri = slot_round(cc, i);
        if (G > 0 && ri != 0) continue;       // a frame that has boxes uses its first round only
        if (j < G) {
            if (collide(cx[G + i], cy[G + i], cx[j], cy[j])) atomicOr(&s_hitframe, 1u << i);
        } else {
            const int jj = j - G;
            if (jj != i && slot_round(cc, jj) == ri && collide(cx[G + i], cy[G + i], cx[G + jj], cy[G + jj]))
                atomicOr(&s_row[i], 1u << jj);
        }
    }
    __syncthreads();
    if (tid == 0) {
        int s0 = 0;
        for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) {
            const int s1 = s0 + cc[r];
            unsigned accepted = 0u;           // accepted for the round's earlier groups
            int i = s0;
            while (i < s1) {
                int e = i + 1;
                while (e < s1 && cand[e].group == cand[i].group) ++e;
                // the group's candidates not dropped so far: a dropped one's row AND column are cleared
                unsigned alive = (e - i == 32 ? 0xffffffffu : ((1u << (e - i)) - 1u)) << i;
                for (int k = i; k < e; ++k) {
                    const bool hit = ((s_hitframe >> k) & 1u) != 0u || (s_row[k] & (accepted | alive)) != 0u;
                    if (hit) alive &= ~(1u << k);
                    s_status[k] = (G > 0 && r > 0) ? PP_GTS_ROUND_NOT_USED : hit ? PP_GTS_BOX_COLLISION : kPending;
                }
                accepted |= alive;
                i = e;
            }
            s0 = s1;
        }
        for (int k = NC; k < PP_GTS_MAX_CAND; ++k) s_status[k] = PP_GTS_ROUND_NOT_USED;
    }
    __syncthreads();
    if (tid < PP_GTS_MAX_CAND) {
        const size_t o = (size_t)b * PP_GTS_MAX_CAND + tid;
        p.status[o] = s_status[tid];
        p.counts[o] = 0;
        if (s_status[tid] == kPending) {
            const double* q = p.db_box + (size_t)cand[tid].object * 7;
            GtsPlane& pl = p.planes[o];
            box_planes3(q, pl.n, pl.d);
        }
    }
}

__global__ __launch_bounds__(256) void k_gts_count(GtsParams p) {
    const int b = blockIdx.y;
    const int o0 = p.offsets[b];
    const int n = p.offsets[b + 1] - o0;
    if ((int)(blockIdx.x * 256) >= n) return;          // uniform across the workgroup
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    double x = 0.0, y = 0.0, z = 0.0;
    if (live) {
        const float* in = p.pts_in + ((size_t)o0 + i) * p.F;
        x = in[0]; y = in[1]; z = in[2];
    }
    const int* st = p.status + (size_t)b * PP_GTS_MAX_CAND;
    const GtsPlane* pls = p.planes + (size_t)b * PP_GTS_MAX_CAND;
    for (int s = 0; s < PP_GTS_MAX_CAND; ++s) {
        if (st[s] != kPending) continue;               // uniform
        const GtsPlane& r = pls[s];
        bool inside = live;
        for (int f = 0; f < 6 && inside; ++f)
            if (((x * r.n[f][0] + y * r.n[f][1]) + z * r.n[f][2]) + r.d[f] >= 0.0) inside = false;
        const unsigned long long m = __ballot(inside);
        if ((threadIdx.x & (PP_WAVE - 1)) == 0 && m != 0ull)
            atomicAdd(&p.counts[(size_t)b * PP_GTS_MAX_CAND + s], __popcll(m));
    }
}

__global__ __launch_bounds__(256) void k_gts_decide(GtsParams p) {
    const int tid = threadIdx.x;
    for (int b = tid; b < p.batch; b += 256) {
        const int G = p.cnt_in[b];
        const int* cc = p.cand_counts + (size_t)b * PP_GTS_MAX_ROUNDS;
        const pp_gts_cand* cand = p.cands + (size_t)b * PP_GTS_MAX_CAND;
        int* st = p.status + (size_t)b * PP_GTS_MAX_CAND;
        int* cnt = p.counts + (size_t)b * PP_GTS_MAX_CAND;
        int* slots = p.acc_slot + (size_t)b * PP_GTS_MAX_CAND;
        int* pstart = p.acc_pstart + (size_t)b * (PP_GTS_MAX_CAND + 1);
        int acc = 0, used = -1, pasted = 0, s0 = 0;
        pstart[0] = 0;
        for (int r = 0; r < PP_GTS_MAX_ROUNDS; ++r) {
            const int s1 = s0 + cc[r];
            if (used >= 0 || (G > 0 && r > 0)) {        // behind the round that was taken
                for (int s = s0; s < s1; ++s) { st[s] = PP_GTS_ROUND_NOT_USED; cnt[s] = 0; }
                s0 = s1;
                continue;
            }
            int k = 0;                                   // survivors of the box test so far: the k-th takes the k-th coin
            for (int s = s0; s < s1; ++s) {
                if (st[s] != kPending) continue;
                const bool low = cand[s0 + k].low != 0;
                ++k;
                const int obj = cand[s].object;
                const double* q = p.db_box + (size_t)obj * 7;
                const int npts = p.db_off[obj + 1] - p.db_off[obj];
                const int c = cnt[s];
                const double dist = sqrt(fabs(q[0]) * fabs(q[0]) + fabs(q[1]) * fabs(q[1]));
                int v;
                if (!(c < p.max_pc)) v = PP_GTS_TOO_MANY_POINTS;
                else if (!(c >= p.min_pc || (dist < 2.5 && low))) v = PP_GTS_TOO_FEW_POINTS;
                else if (npts <= 0) v = PP_GTS_EMPTY_OBJECT;
                else v = PP_GTS_ACCEPTED;
                st[s] = v;
                if (v == PP_GTS_ACCEPTED) {
                    slots[acc] = s;
                    pasted += npts;
                    pstart[++acc] = pasted;
                }
            }
            if (acc > 0) used = r;                       // (a frame without boxes goes on to its next round otherwise)
            s0 = s1;
        }
        for (int s = s0; s < PP_GTS_MAX_CAND; ++s) { st[s] = PP_GTS_ROUND_NOT_USED; cnt[s] = 0; }
        p.round_used[b] = used;
        p.acc_n[b] = acc;
        p.cnt_out[b] = G + acc;
    }
    __syncthreads();
    int* in_off = p.box_off;
    int* out_off = p.box_off + (p.batch + 1);
    if (tid == 0) {
        int po = 0, bi = 0, bo = 0;
        for (int b = 0; b < p.batch; ++b) {
            p.offsets_out[b] = po;
            in_off[b] = bi;
            out_off[b] = bo;
            const int* pstart = p.acc_pstart + (size_t)b * (PP_GTS_MAX_CAND + 1);
            po += (p.offsets[b + 1] - p.offsets[b]) + pstart[p.acc_n[b]];
            bi += p.cnt_in[b];
            bo += p.cnt_out[b];
        }
        p.offsets_out[p.batch] = po;
        in_off[p.batch] = bi;
        out_off[p.batch] = bo;
    }
}

__global__ __launch_bounds__(256) void k_gts_paste(GtsParams p) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0) {      // the frame's first workgroup also writes its boxes: the frame's own, then the accepted objects'
        const int* in_off = p.box_off;
        const int* out_off = p.box_off + (p.batch + 1);
        const int G = p.cnt_in[b], K = p.cnt_out[b];
        const int* slots = p.acc_slot + (size_t)b * PP_GTS_MAX_CAND;
        const pp_gts_cand* cand = p.cands + (size_t)b * PP_GTS_MAX_CAND;
        for (int t = threadIdx.x; t < K; t += 256) {
            float* dst = p.gt_out + (size_t)(out_off[b] + t) * 7;
            if (t < G) {
                const float* src = p.gt_in + (size_t)(in_off[b] + t) * 7;
                for (int k = 0; k < 7; ++k) dst[k] = src[k];
                p.cls_out[out_off[b] + t] = p.cls_in ? p.cls_in[in_off[b] + t] : 1;
                p.valid_out[out_off[b] + t] = p.valid_in ? p.valid_in[in_off[b] + t] : (uint8_t)1;
            } else {
                const int obj = cand[slots[t - G]].object;
                const double* src = p.db_box + (size_t)obj * 7;
                for (int k = 0; k < 7; ++k) dst[k] = (float)src[k];
                p.cls_out[out_off[b] + t] = p.db_cls[obj];
                p.valid_out[out_off[b] + t] = 1;
            }
        }
    }
    const int o0 = p.offsets_out[b];
    const int n = p.offsets_out[b + 1] - o0;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int acc = p.acc_n[b];
    const int* pstart = p.acc_pstart + (size_t)b * (PP_GTS_MAX_CAND + 1);
    const int pasted = pstart[acc];
    float* out = p.pts_out + ((size_t)o0 + i) * p.F;
    if (i >= pasted) {
        const float* in = p.pts_in + ((size_t)p.offsets[b] + (i - pasted)) * p.F;
        for (int k = 0; k < p.F; ++k) out[k] = in[k];
        return;
    }
    int k = 0;
    while (k + 1 < acc && pstart[k + 1] <= i) ++k;
    const int obj = p.cands[(size_t)b * PP_GTS_MAX_CAND + p.acc_slot[(size_t)b * PP_GTS_MAX_CAND + k]].object;
    const float* in = p.db_pts + ((size_t)p.db_off[obj] + (i - pstart[k])) * p.F;
    const double* q = p.db_box + (size_t)obj * 7;
    // a float32 array += float64 centre: the sum in float64, rounded once
    out[0] = (float)((double)in[0] + q[0]);
    out[1] = (float)((double)in[1] + q[1]);
    out[2] = (float)((double)in[2] + q[2]);
    for (int f = 3; f < p.F; ++f) out[f] = in[f];
}

}  // namespace

void launch_gt_sample(const GtsParams& p, int max_n, int max_out_n, hipStream_t s) {
    if (p.batch <= 0) return;
    PP_LAUNCH("k_gts_select", k_gts_select, dim3((unsigned)p.batch), dim3(kSelThreads), 0, s, p);
    if (max_n > 0)
        PP_LAUNCH("k_gts_count", k_gts_count, dim3((unsigned)((max_n + 255) / 256), (unsigned)p.batch), dim3(256), 0, s, p);
    PP_LAUNCH("k_gts_decide", k_gts_decide, dim3(1), dim3(256), 0, s, p);
    PP_LAUNCH("k_gts_paste", k_gts_paste, dim3((unsigned)std::max(1, (max_out_n + 255) / 256), (unsigned)p.batch), dim3(256), 0, s, p);
}
