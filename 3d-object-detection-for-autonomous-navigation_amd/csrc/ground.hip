// Ground plane per frame (pp_set_ground / pp_ground_async, pp_ground_points; ground.py states the rule and the order of
// every operation, and this file copies it).  Plain launches whatever the batch (grid y = frame):
//   k_ground_hyp      one workgroup per frame, a lane per hypothesis: its three rows -> a 32-byte record (a, b, c, valid);
//                     the valid records once more, compacted in order of k by ballot with k in their spare word, and
//                     their number; clears the frame's counts, sums and info words
//   k_ground_score    one workgroup per tile of GR_TILE rows: a lane holds GR_RPL rows as float64 in registers with their
//                     candidate flags; the COMPACT table goes through LDS in chunks and is read at one address per wave
//                     (a broadcast), so no lane ever looks at an invalid record; per hypothesis a ballot and pop-count
//                     per held row, one lane adds to the LDS counter of the record's k; at the end the non-zero counters
//                     go out as one integer atomicAdd each
//   k_ground_pick     one wave per frame: the least key ((2^31 - count) << 32) | k by lane shuffles -> status, winner, plane
//   k_ground_moments  (refine) a lane per row: the nine int64 sums of the winner's inliers, reduced by shuffles, one 64-bit
//                     integer atomic per wave and sum
//   k_ground_refit    (refine) one wave per frame: the plane from the sums, in ground.py's order
//   k_ground_class    a lane per row: its class from the final plane; two ballots are two 64-bit stores by one lane, the
//                     class counts integer atomics
// All arithmetic of the rule is float64 with + - * / and comparisons (-ffp-contract=off keeps the products and sums apart;
// a float64 division is correctly rounded).  No floating-point atomic, no transcendental call, no inline assembly: two runs
// give the same bytes, and they are ground_np's.
// BOUNDS.  A triple's row (u * n) >> 32 lies below n because u < 2^32, and is formed only with n > 0; a row is read only
// with i < n, the frame's own count; hypothesis k is read and written only with k < K <= PP_GROUND_MAX_HYP, which is also
// the size of the LDS counters; a compact record lands below the frame's count of valid ones, itself at most K, and the k
// it carries is clamped to K - 1 before it indexes a counter; word w of a frame is stored only with w < stride.
#include "pp_common.h"

namespace {

constexpr int GR_BLOCK = 256;
constexpr int GR_HYP_BLOCK = PP_GROUND_MAX_HYP;   // k_ground_hyp: every hypothesis of a frame in one workgroup
constexpr int GR_RPL = 4;                     // rows a lane of k_ground_score holds
constexpr int GR_TILE = GR_BLOCK * GR_RPL;    // rows of its workgroup
constexpr int GR_CHUNK = 128;                 // records of the table in LDS at a time: 4 KB
constexpr int GR_HYP_WORDS = (int)(sizeof(GrHyp) / 4);
constexpr int GR_OK = 0, GR_FALLBACK = 1;
static_assert(sizeof(GrHyp) == 32, "GrHyp: 3 doubles, 2 int32 (copied into LDS as 32-bit words)");
static_assert(PP_GROUND_INFO == 12 && PP_GROUND_SUMS == 9, "ground.py's INFO and SUMS");
static_assert(PP_GROUND_MAX_HYP % GR_CHUNK == 0, "whole chunks");
static_assert(GR_HYP_BLOCK <= 1024 && GR_HYP_BLOCK % 64 == 0, "k_ground_hyp compacts a frame's records in one workgroup of whole waves");

__device__ __forceinline__ bool gr_finite(double v) { return (v - v) == 0.0; }

__device__ __forceinline__ bool gr_candidate(const pp_ground_config& c, double x, double y, double z) {
    return gr_finite(x) && gr_finite(y) && gr_finite(z) && (x * x + y * y) <= c.max_range * c.max_range && z <= c.cand_z_max;
}

// the slope and height tests of step 2 (a NaN fails)
__device__ __forceinline__ bool gr_plane_ok(const pp_ground_config& c, double a, double b, double c0) {
    return (a * a + b * b) <= c.max_slope * c.max_slope && c.h_min <= -c0 && -c0 <= c.h_max;
}

__device__ __forceinline__ double gr_residual(double a, double b, double c0, double x, double y, double z) {
    return z - (((a * x) + (b * y)) + c0);
}

__global__ __launch_bounds__(GR_HYP_BLOCK) void k_ground_hyp(GrParams p) {
    const int b = blockIdx.x, tid = threadIdx.x, k = tid, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_wave[GR_HYP_BLOCK / 64];
    const pp_ground_config& c = p.cfg;
    const int o0 = p.offsets[b], n = max(p.offsets[b + 1] - o0, 0);
    {                                                      // what the later launches add to
        if (tid < PP_GROUND_INFO) p.info[(size_t)b * PP_GROUND_INFO + tid] = tid == PP_GROUND_INFO - 1 ? n : 0;
        if (tid < PP_GROUND_SUMS) p.sums[(size_t)b * PP_GROUND_SUMS + tid] = 0ll;
    }
    const bool mine = k < p.K;
    if (mine) p.counts[(size_t)b * p.K + k] = 0;
    GrHyp h;
    h.a = 0.0; h.b = 0.0; h.c = 0.0; h.valid = 0; h.pad = k;
    if (mine && n > 0) {
        const unsigned* t = p.triples + ((size_t)b * p.K + k) * 3;
        double x[3], y[3], z[3];
        bool ok = true;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int j = (int)(((unsigned long long)t[q] * (unsigned long long)n) >> 32);      // < n
            const float* r = p.points + (size_t)(o0 + j) * p.F;
            x[q] = (double)r[0]; y[q] = (double)r[1]; z[q] = (double)r[2];
            ok = ok && gr_candidate(c, x[q], y[q], z[q]);
        }
        if (ok) {
            const double e1x = x[1] - x[0], e1y = y[1] - y[0], e1z = z[1] - z[0];
            const double e2x = x[2] - x[0], e2y = y[2] - y[0], e2z = z[2] - z[0];
            const double nx = (e1y * e2z) - (e1z * e2y);
            const double ny = (e1z * e2x) - (e1x * e2z);
            const double nz = (e1x * e2y) - (e1y * e2x);
            if (!(nz == 0.0)) {
                const double a = -nx / nz;
                const double bb = -ny / nz;
                const double c0 = z[0] - ((a * x[0]) + (bb * y[0]));
                if (gr_plane_ok(c, a, bb, c0)) { h.a = a; h.b = bb; h.c = c0; h.valid = 1; }
            }
        }
    }
    if (mine) p.hyp[(size_t)b * p.K + k] = h;
    // the valid records in order of k, back to back: what k_ground_score walks
    const unsigned long long m = __ballot(h.valid != 0);
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();                                       // (also: the info words are cleared before tid 0 writes one)
    int off = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < GR_HYP_BLOCK / 64; ++q) {
        if (q < wave) off += s_wave[q];
        tot += s_wave[q];
    }
    if (h.valid) p.chyp[(size_t)b * p.K + off + __popcll(m & ((1ull << lane) - 1ull))] = h;      // off + ... < tot <= K
    if (tid == 0) p.info[(size_t)b * PP_GROUND_INFO + 4] = tot;
}

__global__ __launch_bounds__(GR_BLOCK) void k_ground_score(GrParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_ground_config& c = p.cfg;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    const int base = blockIdx.x * GR_TILE;
    if (base >= n) return;                                 // (the whole workgroup)
    __shared__ GrHyp s_h[GR_CHUNK];
    __shared__ int s_cnt[PP_GROUND_MAX_HYP];
    const int K = min(p.K, PP_GROUND_MAX_HYP);
    double x[GR_RPL], y[GR_RPL], z[GR_RPL];
    bool cand[GR_RPL];
    int nc = 0;                                            // the wave's candidates
#pragma unroll
    for (int q = 0; q < GR_RPL; ++q) {
        const int i = base + q * GR_BLOCK + tid;
        x[q] = 0.0; y[q] = 0.0; z[q] = 0.0; cand[q] = false;
        if (i < n) {
            const float* r = p.points + (size_t)(o0 + i) * p.F;
            x[q] = (double)r[0]; y[q] = (double)r[1]; z[q] = (double)r[2];
            cand[q] = gr_candidate(c, x[q], y[q], z[q]);
        }
        nc += __popcll(__ballot(cand[q]));
    }
    for (int k = tid; k < K; k += GR_BLOCK) s_cnt[k] = 0;
    if (lane == 0 && nc) atomicAdd(p.info + (size_t)b * PP_GROUND_INFO + 3, nc);
    const double dist = c.inlier_dist;
    const int nv = min(p.info[(size_t)b * PP_GROUND_INFO + 4], K);     // k_ground_hyp's count of valid records
    for (int k0 = 0; k0 < nv; k0 += GR_CHUNK) {
        __syncthreads();                                   // the last chunk is consumed (first trip: the counters are zero)
        const int m = min(GR_CHUNK, nv - k0);
        {
            const unsigned* src = reinterpret_cast<const unsigned*>(p.chyp + (size_t)b * p.K + k0);
            unsigned* dst = reinterpret_cast<unsigned*>(s_h);
            for (int w = tid; w < m * GR_HYP_WORDS; w += GR_BLOCK) dst[w] = src[w];
        }
        __syncthreads();
        if (nc == 0) continue;                             // (the whole wave) no candidate: nothing to count
        for (int j = 0; j < m; ++j) {
            const GrHyp& h = s_h[j];                       // one address in every lane: an LDS broadcast
            const double a = h.a, bb = h.b, c0 = h.c;
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < GR_RPL; ++q)
                cnt += __popcll(__ballot(cand[q] && fabs(gr_residual(a, bb, c0, x[q], y[q], z[q])) <= dist));
            if (lane == 0 && cnt) atomicAdd(&s_cnt[min(max(h.pad, 0), K - 1)], cnt);       // pad: the record's k, < K
        }
    }
    __syncthreads();
    for (int k = tid; k < K; k += GR_BLOCK) {
        const int v = s_cnt[k];
        if (v) atomicAdd(p.counts + (size_t)b * p.K + k, v);
    }
}

__global__ __launch_bounds__(64) void k_ground_pick(GrParams p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const pp_ground_config& c = p.cfg;
    const GrHyp* hyp = p.hyp + (size_t)b * p.K;
    const int* counts = p.counts + (size_t)b * p.K;
    unsigned long long key = ~0ull;
    int nvalid = 0;
    for (int k = lane; k < p.K; k += 64)
        if (hyp[k].valid) {
            const unsigned long long q = ((unsigned long long)(0x80000000ll - (long long)counts[k]) << 32) | (unsigned long long)k;
            key = q < key ? q : key;
            ++nvalid;
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
        nvalid += __shfl_xor(nvalid, m);
    }
    if (lane == 0) {
        int* info = p.info + (size_t)b * PP_GROUND_INFO;
        double* plane = p.plane + (size_t)b * 3;
        int winner = -1, inl = 0;
        if (nvalid > 0) {
            winner = (int)(key & 0xFFFFFFFFull);
            inl = counts[winner];
        }
        const bool ok = winner >= 0 && inl >= c.min_inliers;
        info[0] = ok ? GR_OK : GR_FALLBACK;
        info[1] = winner;
        info[2] = inl;
        info[4] = nvalid;
        if (ok) { plane[0] = hyp[winner].a; plane[1] = hyp[winner].b; plane[2] = hyp[winner].c; }
        else { plane[0] = 0.0; plane[1] = 0.0; plane[2] = c.fallback_c; }
    }
}

__global__ __launch_bounds__(GR_BLOCK) void k_ground_moments(GrParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_ground_config& c = p.cfg;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    if ((int)blockIdx.x * GR_BLOCK >= n) return;           // (the whole workgroup)
    if (p.info[(size_t)b * PP_GROUND_INFO] != GR_OK) return;       // the fallback plane takes no refit
    const int i = blockIdx.x * GR_BLOCK + tid;
    const double a = p.plane[(size_t)b * 3], bb = p.plane[(size_t)b * 3 + 1], c0 = p.plane[(size_t)b * 3 + 2];
    long long v[PP_GROUND_SUMS];
#pragma unroll
    for (int j = 0; j < PP_GROUND_SUMS; ++j) v[j] = 0ll;
    if (i < n) {
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const double x = (double)r[0], y = (double)r[1], z = (double)r[2];
        if (gr_candidate(c, x, y, z) && fabs(gr_residual(a, bb, c0, x, y, z)) <= c.inlier_dist) {
            // |x|, |y|, |z| < 64 under pp_set_ground's bounds for refine: |q| <= 2^14
            const long long qx = (long long)floor(x * 256.0), qy = (long long)floor(y * 256.0), qz = (long long)floor(z * 256.0);
            v[0] = 1ll; v[1] = qx; v[2] = qy; v[3] = qz;
            v[4] = qx * qx; v[5] = qx * qy; v[6] = qy * qy; v[7] = qx * qz; v[8] = qy * qz;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
        for (int j = 0; j < PP_GROUND_SUMS; ++j) v[j] += __shfl_xor(v[j], m);
    if (lane == 0 && v[0] != 0ll) {
        unsigned long long* sums = reinterpret_cast<unsigned long long*>(p.sums + (size_t)b * PP_GROUND_SUMS);
#pragma unroll
        for (int j = 0; j < PP_GROUND_SUMS; ++j)
            if (v[j] != 0ll) atomicAdd(sums + j, (unsigned long long)v[j]);        // two's complement: a negative sum adds as it should
    }
}

__global__ __launch_bounds__(64) void k_ground_refit(GrParams p) {
    const int b = blockIdx.x;
    const pp_ground_config& c = p.cfg;
    if (threadIdx.x != 0) return;
    int* info = p.info + (size_t)b * PP_GROUND_INFO;
    if (info[0] != GR_OK) return;
    const long long* s = p.sums + (size_t)b * PP_GROUND_SUMS;
    const double N = (double)s[0], Sx = (double)s[1], Sy = (double)s[2], Sz = (double)s[3], Sxx = (double)s[4], Sxy = (double)s[5],
                 Syy = (double)s[6], Sxz = (double)s[7], Syz = (double)s[8];
    const double cxx = (N * Sxx) - (Sx * Sx);
    const double cxy = (N * Sxy) - (Sx * Sy);
    const double cyy = (N * Syy) - (Sy * Sy);
    const double cxz = (N * Sxz) - (Sx * Sz);
    const double cyz = (N * Syz) - (Sy * Sz);
    const double det = (cxx * cyy) - (cxy * cxy);
    if (!(det > 0.0)) return;
    const double a = ((cxz * cyy) - (cyz * cxy)) / det;
    const double bb = ((cyz * cxx) - (cxz * cxy)) / det;
    const double c0 = (((Sz - (a * Sx)) - (bb * Sy)) / N) / 256.0;
    if (!gr_plane_ok(c, a, bb, c0)) return;
    double* plane = p.plane + (size_t)b * 3;
    plane[0] = a; plane[1] = bb; plane[2] = c0;
    info[10] = 1;
}

__global__ __launch_bounds__(GR_BLOCK) void k_ground_class(GrParams p) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const pp_ground_config& c = p.cfg;
    const int o0 = p.offsets[b], n = p.offsets[b + 1] - o0;
    const int i = blockIdx.x * GR_BLOCK + tid;
    const int w = i >> 6;                                  // the wave's word: rows 64 w .. 64 w + 63 of the frame
    int cls = -1;                                          // 0 ignored, 1 ground, 2 obstacle, 3 overhead, 4 below; -1: no row
    if (i < n) {
        const double a = p.plane[(size_t)b * 3], bb = p.plane[(size_t)b * 3 + 1], c0 = p.plane[(size_t)b * 3 + 2];
        const float* r = p.points + (size_t)(o0 + i) * p.F;
        const double res = gr_residual(a, bb, c0, (double)r[0], (double)r[1], (double)r[2]);
        if (!(res == res)) cls = 0;
        else if (fabs(res) <= c.ground_dist) cls = 1;
        else if (res > c.ground_dist) cls = res <= c.overhead_max ? 2 : 3;
        else cls = 4;
    }
    const unsigned long long ign = __ballot(cls == 0), gnd = __ballot(cls == 1), obs = __ballot(cls == 2), ovh = __ballot(cls == 3),
                             bel = __ballot(cls == 4);
    if (lane == 0) {
        if (w < p.stride) {
            p.gnd[(size_t)b * p.stride + w] = gnd;
            p.obs[(size_t)b * p.stride + w] = obs;
        }
        int* info = p.info + (size_t)b * PP_GROUND_INFO;
        if (gnd) atomicAdd(info + 5, __popcll(gnd));
        if (obs) atomicAdd(info + 6, __popcll(obs));
        if (ovh) atomicAdd(info + 7, __popcll(ovh));
        if (bel) atomicAdd(info + 8, __popcll(bel));
        if (ign) atomicAdd(info + 9, __popcll(ign));
    }
}

}  // namespace

int ground_launches(const GrParams& p) {
    if (p.batch <= 0) return 0;
    return p.max_n > 0 ? (p.cfg.refine ? 6 : 4) : 2;
}

void launch_ground(const GrParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const bool rows = p.max_n > 0;
    PP_LAUNCH("k_ground_hyp", k_ground_hyp, dim3(p.batch), dim3(GR_HYP_BLOCK), 0, s, p);
    if (rows) PP_LAUNCH("k_ground_score", k_ground_score, dim3((p.max_n + GR_TILE - 1) / GR_TILE, p.batch), dim3(GR_BLOCK), 0, s, p);
    PP_LAUNCH("k_ground_pick", k_ground_pick, dim3(p.batch), dim3(64), 0, s, p);
    if (rows && p.cfg.refine) {
        PP_LAUNCH("k_ground_moments", k_ground_moments, dim3((p.max_n + GR_BLOCK - 1) / GR_BLOCK, p.batch), dim3(GR_BLOCK), 0, s, p);
        PP_LAUNCH("k_ground_refit", k_ground_refit, dim3(p.batch), dim3(64), 0, s, p);
    }
    if (rows) PP_LAUNCH("k_ground_class", k_ground_class, dim3((p.max_n + GR_BLOCK - 1) / GR_BLOCK, p.batch), dim3(GR_BLOCK), 0, s, p);
}
