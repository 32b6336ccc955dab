// Detection post-process: mask -> top-100 -> decode -> stand-up AABB -> NMS -> flip -> camera.
//
// Replaces VoxelNet.predict for one frame per workgroup (reference
// model/voxelnet.py:1105-1379) and the functions it calls:
//   anchors_mask gather, argmax(dir), sigmoid           model/voxelnet.py:1120-1150
//   top-100 by score (np.argpartition)                  model/voxelnet.py:1207-1214
//   second_box_decode                                   libraries/eval_helper_functions.py:388-461
//   center_to_corner_box2d + corner_to_standup_nd_jit   load_data.py:1525-1593, :1330-1340
//   nms -> nms_gpu -> nms_kernel / iou_device / nms_postprocess
//                                                       libraries/eval_helper_functions.py:463-598
//   direction flip, box_lidar_to_camera                 model/voxelnet.py:1305-1310; eval_helper_functions.py:728-740
// The reference pulls the head maps to the host and bounces the <=100 boxes to
// the GPU and back for a numba NMS kernel (1.4-2.2 ms per call); here the head
// maps never leave HBM and the whole tail is one launch.
//
// Selection is done on the logit, not on the score, with a 64-bit key (comp_key):
// the float's bits mapped to an order-preserving unsigned integer in the high
// word, the complemented anchor index in the low word.  The order it implements:
//   1. logit descending, as a float value;
//   2. +0.0 above -0.0 (their bit patterns differ, their float values do not);
//   3. anchor index ascending.
// The reference orders float32 *scores* with np.argpartition / argsort, whose
// tie order is implementation-defined.  Sigmoid is monotone, so descending logit
// is non-increasing score: this order is a deterministic refinement of the
// reference's.  It is finer where float32 sigmoid maps different logits to one
// score (every logit above about 17 scores 1.0): those are ordered by logit.
// tests/postprocess_ref.py restates the rule; tests/test_gpu_select.py holds the
// kernel to it.  NMS IoU follows iou_device exactly: AABB with `+1`
// on widths (pixel convention applied to metres), differences in float32, the
// rest in float64, strict `>` threshold.
//
// NMS rule (template parameter, pp_set_nms_mode): PP_NMS_STANDUP is the above.  PP_NMS_ROTATED replaces only the
// mask computation by rotate_nms_kernel's (second/core/non_max_suppression/nms_gpu.py:419-452, which the reference
// ships but never wires in): devRotateIoU of the decoded [x, y, w, l, r] before the direction flip (boxes_for_nms,
// model/voxelnet.py:1233), the higher-scoring box as first argument, float32, strict `>`.  The <= 100 * 99 / 2 pairs
// are spread over the workgroup; the clip's polygon scratch ([8][1024] x 3 floats, riou_dev.h) lies on s_ckey, whose
// candidate keys are dead once the top set is in s_key -- the footprint grows by the corner table only.
//
// PP_NMS_SOFT replaces the masks and the sweep by the rounds of soft_nms_jit (second/core/non_max_suppression/nms_cpu.py:
// 79-169, soft_nms_dev.h; pp_set_soft_nms) on the same stand-up boxes: wave 0 holds boxes `lane` and `lane + 64` with their
// current scores in registers, a round is an argmax butterfly, a broadcast read of the selected box and one float64
// overlap per lane; a kept row's score is its decayed score.  Method hard with a floor below every score is the default
// rule, byte for byte.
//
// Image boxes (template parameter, pp_set_projection): the lane that assembles a kept detection's box3d_camera also
// projects it (box3d_to_bbox of second/core/box_np_ops.py:849-857, box_project_dev.h) with the frame's P2 and stores the
// four doubles beside the detections.  The reference's predict() has this commented out and returns a constant
// (model/voxelnet.py:1336-1360); off (the default) is the instantiation without a trace of it.
//
// Per-class suppression (template parameter, pp_set_class_nms): the branch model.second.use_multi_class_nms names and the
// reference leaves as `pass` (model/voxelnet.py:1170-1171).  The grid is (batch, num_class); workgroup (b, c) runs the very
// same pass with class c's logit as the anchor's score and c as its label -- threshold, top-100, NMS and the caps are per
// class -- and stores its kept rows into segment (b, c) of a scratch buffer.  k_gather_classes, one workgroup per frame
// behind it on the stream, lays the segments end to end (class 0's rows first) and writes the frame's total.
#include <type_traits>

#include "box_project_dev.h"
#include "riou_dev.h"
#include "soft_nms_dev.h"

#define PT 1024
#define KMAX 128   // >= the reference's hard-coded top-100
#define CCAP 12288 // candidate keys kept in LDS (96 KB); more candidates -> re-read the head map per pass

__device__ __forceinline__ unsigned long long comp_key(float logit, unsigned a) {
    unsigned u = __float_as_uint(logit);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(~a);
}

template <int NMS, bool PROJ, bool PERCLS>
__global__ __launch_bounds__(PT) void k_postprocess(PostParams p) {
    __shared__ int s_hist[256];
    __shared__ int s_cum[256];
    __shared__ int s_wsum[4];
    __shared__ unsigned long long s_ckey[CCAP];   // compacted candidate keys (order irrelevant: keys are unique)
    __shared__ int s_ncand;
    __shared__ unsigned long long s_prefix;
    __shared__ int s_need, s_shift, s_done, s_cnt;
    __shared__ unsigned long long s_key[KMAX];
    __shared__ int s_order[KMAX];
    __shared__ float s_box[KMAX][7];
    __shared__ float s_aabb[KMAX][4];
    __shared__ float s_score[KMAX];
    __shared__ int s_dir[KMAX];
    __shared__ int s_label[KMAX];
    __shared__ int s_anchor[KMAX];
    __shared__ unsigned long long s_mask[KMAX][2];
    __shared__ int s_keep[KMAX];
    __shared__ int s_nkeep;
    __shared__ int s_bad;      // a non-finite class logit anywhere in the frame, or a non-finite value in a selected row

    float (*s_rc)[9] = nullptr;     // rotated rule only: corners + area of the decoded boxes (riou_box_corners)
    if constexpr (NMS == PP_NMS_ROTATED) {
        __shared__ float s_corners[KMAX][9];
        s_rc = s_corners;
    }

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int kc = PERCLS ? (int)blockIdx.y : 0;   // per-class rule: the class this workgroup scores and suppresses
    const long long A = p.A;
    const int napl = p.napl;
    const int ncls = p.ncls;
    const int nb = napl * 7, nc = napl * ncls;
    // fused head map row of pixel px: [box napl*7 | cls napl*ncls | dir napl*2 | pad]; anchor a = px*napl + r,
    // class logit k of that anchor at column nb + r*ncls + k (the reference reshapes cls_preds to
    // [B, -1, num_class], model/voxelnet.py:1090).  More than one class: the anchor's score is its largest
    // class score and its label the argmax (model/voxelnet.py:1183-1185; sigmoid is monotone, so the
    // selection runs on the largest logit)
    const float* head = p.head + (size_t)b * (A / napl) * PP_HEAD_COLS;
    const uint8_t* msk = p.mask + (size_t)b * A;
    // candidate scan source: the compact class-logit plane the last deconv left (napl*ncls floats per pixel,
    // consecutive anchors = consecutive words) or, without it, the cls columns of the 128-byte head rows
    const float* cplane = (p.cls != nullptr) ? p.cls + (size_t)b * A * ncls : nullptr;
    // Non-finite head outputs (the split-precision GEMMs carry an operand as two float16 pieces: an activation beyond
    // +-65504 becomes inf - inf = NaN in the product; the ReLUs of the backbone keep a NaN, relu_keep_nan) must not
    // turn into boxes: every class logit of the frame passes through here, masked or not, and the frame is flagged.
    bool bad = false;
    auto cls_of = [&](long long a) -> float {
        const long long px = a / napl;
        const float* q = (cplane != nullptr) ? cplane + a * ncls
                                             : head + px * PP_HEAD_COLS + nb + (int)(a - px * napl) * ncls;
        float m = q[0];
        bad |= !pp_finite(m);
        for (int k = 1; k < ncls; ++k) {
            bad |= !pp_finite(q[k]);
            if constexpr (PERCLS) m = (k == kc) ? q[k] : m; else m = fmaxf(m, q[k]);
        }
        return m;
    };
    const float thr = p.score_thr;
    const int KTOP = 100;  // model/voxelnet.py:1207 (hard-coded)

    auto is_cand = [&](long long a, float& logit) -> bool {
        if (msk[a] != 1) return false;
        logit = cls_of(a);
        if (thr > 0.f) {
            const float sc = 1.f / (1.f + expf(-logit));
            if (!(sc >= thr)) return false;
        }
        return true;
    };

    // ---- candidates -> LDS once (the head map is read a single time; the select passes run on LDS) ----
    if (tid == 0) { s_cnt = 0; s_ncand = 0; s_bad = 0; }
    __syncthreads();
    // One pass over the frame's anchors: emit(anchor, logit) for every candidate (mask byte 1, score >= threshold).
    //   * compact class-logit plane and A % 16 == 0 (every shipped grid): a thread takes 16 consecutive anchors -- one
    //     16-byte load of their mask bytes, 4 * ncls 16-byte loads of their logits, all issued before the first use: 9
    //     loads per 16 anchors on the KITTI-shaped head (two classes) instead of 48 (the scan of 107 136 anchors by one
    //     workgroup was 110 us per launch of 32 frames, load-issue bound);
    //   * otherwise 16 strided anchors per thread at a time (the logit loads do not wait for the mask bytes).
    auto scan_candidates = [&](auto&& emit) {
        if (cplane != nullptr && (A & 15) == 0 && ncls <= 4) {
            const uint4* m16 = reinterpret_cast<const uint4*>(msk);
            const float4* l4 = reinterpret_cast<const float4*>(cplane);
            auto fast = [&](auto NC) {                                // the class count as a compile-time constant: the
                constexpr int nc = decltype(NC)::value;               // 16 * nc logits of a thread stay in registers
                for (long long c = tid; c < (A >> 4); c += PT) {
                    const uint4 mk4 = m16[c];
                    float4 lg[4 * nc];
#pragma unroll
                    for (int j = 0; j < 4 * nc; ++j) lg[j] = l4[c * (4 * nc) + j];
                    const unsigned mw[4] = {mk4.x, mk4.y, mk4.z, mk4.w};
                    float lf[16 * nc];
#pragma unroll
                    for (int j = 0; j < 4 * nc; ++j) { lf[4 * j] = lg[j].x; lf[4 * j + 1] = lg[j].y; lf[4 * j + 2] = lg[j].z; lf[4 * j + 3] = lg[j].w; }
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        float m = lf[i * nc];
                        bad |= !pp_finite(m);
#pragma unroll
                        for (int k = 1; k < nc; ++k) {
                            const float v = lf[i * nc + k];
                            bad |= !pp_finite(v);
                            if constexpr (PERCLS) m = (k == kc) ? v : m; else m = fmaxf(m, v);   // (a select: lf stays in registers)
                        }
                        if (((mw[i >> 2] >> (8 * (i & 3))) & 0xffu) != 1u) continue;
                        if (thr > 0.f) {
                            const float sc = 1.f / (1.f + expf(-m));
                            if (!(sc >= thr)) continue;
                        }
                        emit((unsigned)(c * 16 + i), m);
                    }
                }
            };
            if (ncls == 1) fast(std::integral_constant<int, 1>{});
            else if (ncls == 2) fast(std::integral_constant<int, 2>{});
            else if (ncls == 3) fast(std::integral_constant<int, 3>{});
            else fast(std::integral_constant<int, 4>{});
            return;
        }
        for (long long ab = 0; ab < A; ab += 16 * PT) {
            const long long a0 = ab + tid;
            uint8_t mk[16];
            float lgs[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const long long a = a0 + (long long)k * PT;
                mk[k] = (a < A) ? msk[a] : (uint8_t)0;
                lgs[k] = (a < A) ? cls_of(a) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (mk[k] != 1) continue;
                if (thr > 0.f) {
                    const float sc = 1.f / (1.f + expf(-lgs[k]));
                    if (!(sc >= thr)) continue;
                }
                emit((unsigned)(a0 + (long long)k * PT), lgs[k]);
            }
        }
    };
    scan_candidates([&](unsigned a, float lg) {
        const int pos = atomicAdd(&s_ncand, 1);
        if (pos < CCAP) s_ckey[pos] = comp_key(lg, a);
    });
    if (bad) s_bad = 1;
    __syncthreads();
    int ncand = s_ncand;
    bool in_lds = ncand <= CCAP;

    // ---- radix select of the KTOP largest composite keys (8 bits per pass, MSB first) ----
    // over the `n` keys in LDS (lds) or over the frame's candidates re-read from the head map
    auto run_select = [&](bool lds, int n) {
      if (tid == 0) { s_prefix = 0ull; s_need = KTOP; s_shift = 56; s_done = 0; }
      __syncthreads();
      for (int pass = 0; pass < 8; ++pass) {
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        if (s_done) break;
        const int shift = 56 - 8 * pass;
        const unsigned long long prefix = s_prefix;
        if (lds) {
            for (int i = tid; i < n; i += PT) {
                const unsigned long long key = s_ckey[i];
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255ull)], 1);
            }
        } else {
            for (long long a = tid; a < A; a += PT) {
                float lg;
                if (!is_cand(a, lg)) continue;
                const unsigned long long key = comp_key(lg, (unsigned)a);
                if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(int)((key >> shift) & 255ull)], 1);
            }
        }
        __syncthreads();
        // digit of the need-th largest key: suffix sums over the 256 bins by 256 threads (bin 255 - tid)
        if (tid < 256) {
            const int lane_ = tid & 63, wv = tid >> 6;
            const int hv = s_hist[255 - tid];
            const int incl = wave_inclusive_scan(hv);
            if (lane_ == 63) s_wsum[wv] = incl;
            s_cum[tid] = incl;   // within-wave inclusive sums; the wave offsets are added by thread 0 below
        }
        __syncthreads();
        if (tid == 0) {
            int need = s_need, cum = 0, digit = 0;
            bool found = false;
            int woff = 0;
            for (int wv = 0; wv < 4 && !found; ++wv) {
                if (woff + s_wsum[wv] >= need) {   // the bin is inside this wave's 64: binary search on its inclusive sums
                    int lo = 0, hi = 63;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (woff + s_cum[wv * 64 + mid] >= need) hi = mid; else lo = mid + 1;
                    }
                    const int t = wv * 64 + lo;
                    digit = 255 - t;
                    cum = woff + s_cum[t] - s_hist[digit];
                    need -= cum;
                    found = true;
                }
                woff += s_wsum[wv];
            }
            if (!found) {
                // fewer candidates than requested (only possible in pass 0): take them all
                s_prefix = 0ull; s_shift = 0; s_done = 1;
            } else {
                s_prefix = (prefix << 8) | (unsigned long long)digit;
                s_shift = shift;
                s_need = need;
                if (s_hist[digit] == need) s_done = 1;  // the whole bucket is taken
            }
        }
        __syncthreads();
      }
      __syncthreads();
    };
    if (in_lds) {
        run_select(true, ncand);
    } else {
        // More candidates than LDS holds (large grids: 107 k anchors on the KITTI-shaped map): the 100th largest of the
        // FIRST CCAP candidates is a lower bound of the 100th largest of all of them, so one more read of the head map
        // keeps only the keys at or above it -- a few hundred for candidates in no particular order -- and the select
        // runs on those in LDS (round 3 re-read the head map in every one of up to nine passes: 92 us per frame).
        run_select(true, CCAP);
        const unsigned long long floor_key = s_prefix << s_shift;     // every key of that top set is >= this
        __syncthreads();
        if (tid == 0) s_ncand = 0;
        __syncthreads();
        scan_candidates([&](unsigned a, float lg) {
            const unsigned long long key = comp_key(lg, a);
            if (key >= floor_key) {
                const int pos = atomicAdd(&s_ncand, 1);
                if (pos < CCAP) s_ckey[pos] = key;
            }
        });
        __syncthreads();
        const int kept = s_ncand;
        if (kept <= CCAP) { in_lds = true; ncand = kept; run_select(true, kept); }
        else run_select(false, 0);                                    // (adversarial order: the old way)
    }
    __syncthreads();
    {
        const int shift = s_shift;
        const unsigned long long prefix = s_prefix;
        if (in_lds) {
            for (int i = tid; i < ncand; i += PT) {
                const unsigned long long key = s_ckey[i];
                if ((key >> shift) >= prefix) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < KMAX) s_key[pos] = key;
                }
            }
        } else {
            for (long long a = tid; a < A; a += PT) {
                float lg;
                if (!is_cand(a, lg)) continue;
                const unsigned long long key = comp_key(lg, (unsigned)a);
                if ((key >> shift) >= prefix) {
                    const int pos = atomicAdd(&s_cnt, 1);
                    if (pos < KMAX) s_key[pos] = key;
                }
            }
        }
    }
    __syncthreads();
    const int K = min(s_cnt, KTOP);
    // ---- order by descending key (rank by counting; keys are unique) ----
    if (tid < K) {
        const unsigned long long me = s_key[tid];
        int rank = 0;
        for (int j = 0; j < K; ++j) rank += (s_key[j] > me) ? 1 : 0;
        s_order[rank] = tid;
    }
    __syncthreads();

    // ---- decode + stand-up AABB (float32, the reference's operation order) ----
    if (tid < K) {
        const unsigned long long key = s_key[s_order[tid]];
        const unsigned a = ~(unsigned)(key & 0xffffffffull);
        const unsigned apx = a / (unsigned)napl, ar = a - apx * (unsigned)napl;
        const float* hrow = head + (size_t)apx * PP_HEAD_COLS;
        const float* e = hrow + ar * 7;
        const float* an = p.anchors + (size_t)a * 7;
        const float xa = an[0], ya = an[1], wa = an[3], la = an[4], ha = an[5], ra = an[6];
        const float za = __fadd_rn(an[2], __fdiv_rn(ha, 2.f));
        const float diag = __fsqrt_rn(__fadd_rn(__fmul_rn(la, la), __fmul_rn(wa, wa)));
        const float xg = __fadd_rn(__fmul_rn(e[0], diag), xa);
        const float yg = __fadd_rn(__fmul_rn(e[1], diag), ya);
        float zg = __fadd_rn(__fmul_rn(e[2], ha), za);
        const float lg = __fmul_rn(expf(e[4]), la);
        const float wg = __fmul_rn(expf(e[3]), wa);
        const float hg = __fmul_rn(expf(e[5]), ha);
        const float rg = __fadd_rn(e[6], ra);
        zg = __fsub_rn(zg, __fdiv_rn(hg, 2.f));
        s_box[tid][0] = xg; s_box[tid][1] = yg; s_box[tid][2] = zg;
        s_box[tid][3] = wg; s_box[tid][4] = lg; s_box[tid][5] = hg; s_box[tid][6] = rg;
        float lgt = hrow[nb + ar * ncls + kc];
        int lab = kc;
        if constexpr (!PERCLS) {
            for (int k = 1; k < ncls; ++k) {
                const float v = hrow[nb + ar * ncls + k];
                if (v > lgt) { lgt = v; lab = k; }   // argmax: first maximum
            }
        }
        s_label[tid] = lab;
        s_score[tid] = 1.f / (1.f + expf(-lgt));
        // without the direction head the row has no direction pair: columns nb + nc + 2 ar (+ 1) are padding or, with 27
        // columns in use (3 anchors x (7 + 2 classes)), the first column of the NEXT pixel's row -- not read
        const float* d = hrow + nb + nc + ar * 2;
        const float d0 = p.use_dir ? d[0] : 0.f, d1 = p.use_dir ? d[1] : 0.f;
        s_dir[tid] = (d1 > d0) ? 1 : 0;  // np.argmax: first maximum
        s_anchor[tid] = (int)a;
        {
            bool rb = !pp_finite(d0) || !pp_finite(d1);
#pragma unroll
            for (int q = 0; q < 7; ++q) rb |= !pp_finite(e[q]);
            if (rb) s_bad = 1;      // (the class logits were checked by the scan)
        }
        // corners (-,-),(-,+),(+,+),(+,-) * dims, rotate by [[c,-s],[s,c]], + centre; min/max
        const float sn = sinf(rg), cs = cosf(rg);
        const float hx = __fmul_rn(wg, 0.5f), hy = __fmul_rn(lg, 0.5f);
        const float cxs[4] = {-hx, -hx, hx, hx};
        const float cys[4] = {-hy, hy, hy, -hy};
        float x0 = 0.f, y0 = 0.f, x1 = 0.f, y1 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float rx = __fadd_rn(__fadd_rn(__fmul_rn(cxs[q], cs), __fmul_rn(cys[q], sn)), xg);
            const float ry = __fadd_rn(__fadd_rn(__fmul_rn(cxs[q], -sn), __fmul_rn(cys[q], cs)), yg);
            if (q == 0) { x0 = x1 = rx; y0 = y1 = ry; }
            else { x0 = fminf(x0, rx); x1 = fmaxf(x1, rx); y0 = fminf(y0, ry); y1 = fmaxf(y1, ry); }
        }
        s_aabb[tid][0] = x0; s_aabb[tid][1] = y0; s_aabb[tid][2] = x1; s_aabb[tid][3] = y1;
        if constexpr (NMS == PP_NMS_ROTATED) riou_box_corners(xg, yg, wg, lg, rg, s_rc[tid]);
    }
    __syncthreads();

    // ---- NMS over the first min(K, pre_max) boxes (already score-descending) ----
    // suppression masks: 8 threads share a row i and take every 8th j > i (the float64 division keeps
    // iou_device's arithmetic); their partial masks meet in LDS
    const int n = min(K, p.pre_max);
    if (tid < 2 * KMAX) reinterpret_cast<unsigned long long*>(s_mask)[tid] = 0ull;
    __syncthreads();
    if constexpr (NMS == PP_NMS_SOFT) {
        // no n x n matrix (the zeroed masks stay unused): a round below forms the overlaps with its selected box
    } else if constexpr (NMS == PP_NMS_ROTATED) {
        // all (i, j) of the n x n square, 64 consecutive j of one row per wavefront; j <= i has nothing to do
        static_assert(sizeof(s_ckey) >= 3 * RIOU_MAXP * PT * sizeof(float), "the polygon scratch lies on the candidate keys");
        float* s_px = reinterpret_cast<float*>(s_ckey);
        float* s_py = s_px + RIOU_MAXP * PT;
        float* s_vs = s_py + RIOU_MAXP * PT;
        for (int q = tid; q < n * n; q += PT) {
            const int i = q / n, j = q - i * n;
            if (j <= i) continue;
            float c1[8], c2[8];      // c1: the earlier, higher-scoring box (first argument of devRotateIoU)
#pragma unroll
            for (int k = 0; k < 8; ++k) { c1[k] = s_rc[i][k]; c2[k] = s_rc[j][k]; }
            const float iou = riou_iou<PT>(c1, s_rc[i][8], c2, s_rc[j][8], s_px, s_py, s_vs, tid);
            if (iou > p.iou_thr) atomicOr(&s_mask[i][j >> 6], 1ull << (j & 63));
        }
    } else {
        const int row = tid >> 3, sub = tid & 7;
        if (row < n) {
            unsigned long long m0 = 0ull, m1 = 0ull;
            const float ax0 = s_aabb[row][0], ay0 = s_aabb[row][1], ax1 = s_aabb[row][2], ay1 = s_aabb[row][3];
            const double sa = ((double)(ax1 - ax0) + 1.0) * ((double)(ay1 - ay0) + 1.0);
            const double dthr = (double)p.iou_thr;
            for (int j = row + 1 + sub; j < n; j += 8) {
                const float bx0 = s_aabb[j][0], by0 = s_aabb[j][1], bx1 = s_aabb[j][2], by1 = s_aabb[j][3];
                const float left = fmaxf(ax0, bx0), right = fminf(ax1, bx1);
                const float top = fmaxf(ay0, by0), bottom = fminf(ay1, by1);
                const float dw = right - left, dh = bottom - top;   // float32 differences
                const double w = fmax((double)dw + 1.0, 0.0);
                const double hh = fmax((double)dh + 1.0, 0.0);
                const double inter = w * hh;
                const double sb = ((double)(bx1 - bx0) + 1.0) * ((double)(by1 - by0) + 1.0);
                const double iou = inter / (sa + sb - inter);
                if (iou > dthr) {
                    if (j < 64) m0 |= 1ull << j; else m1 |= 1ull << (j - 64);
                }
            }
            if (m0) atomicOr(&s_mask[row][0], m0);
            if (m1) atomicOr(&s_mask[row][1], m1);
        }
    }
    __syncthreads();
    // greedy sweep by wave 0: lane l holds the mask rows l and l + 64 in registers; the kept boxes are walked
    // with find-first-set over "not yet visited and not removed" (scalar), a kept row's mask comes by readlane
    if (tid < 64) {
        int nk = 0;
        if constexpr (NMS == PP_NMS_SOFT) {
            static_assert(KMAX <= 2 * 64, "wave 0 holds two boxes per lane");
            nk = snms_rounds<64, 2>(s_aabb, s_score, n, min(p.post_max, KMAX), p.soft_method, p.iou_thr, p.soft_sigma,
                                    p.soft_floor, lane, (float (*)[1])nullptr, (int (*)[1])nullptr,
                                    [&](int r, int idx, float sc) { s_keep[r] = idx; s_score[idx] = sc; });
        } else {
            const unsigned long long a0 = (lane < n) ? s_mask[lane][0] : 0ull, a1 = (lane < n) ? s_mask[lane][1] : 0ull;
            const unsigned long long b0 = (lane + 64 < n) ? s_mask[lane + 64][0] : 0ull;
            const unsigned long long b1 = (lane + 64 < n) ? s_mask[lane + 64][1] : 0ull;
            auto rdl = [](unsigned long long v, int l) -> unsigned long long {
                const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffull), l);
                const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
                return ((unsigned long long)hi << 32) | lo;
            };
            unsigned long long todo0 = (n >= 64) ? ~0ull : ((1ull << n) - 1ull);
            unsigned long long todo1 = (n <= 64) ? 0ull : ((n - 64 >= 64) ? ~0ull : ((1ull << (n - 64)) - 1ull));
            unsigned long long r0 = 0ull, r1 = 0ull;
            int k0 = 0, k1 = 0;
            while (nk < p.post_max) {
                const unsigned long long c0 = todo0 & ~r0, c1 = todo1 & ~r1;
                if ((c0 | c1) == 0ull) break;
                int i = c0 ? __builtin_ctzll(c0) : 64 + __builtin_ctzll(c1);
                i = __builtin_amdgcn_readfirstlane(i);
                if (lane == (nk & 63)) { if (nk < 64) k0 = i; else k1 = i; }   // lane l remembers kept boxes l and l + 64
                ++nk;
                if (i < 64) {
                    todo0 &= ~((2ull << i) - 1ull);       // i = 63: 2 << 63 wraps to 0, minus 1 = all ones
                    r0 |= rdl(a0, i); r1 |= rdl(a1, i);
                } else {
                    todo0 = 0ull;
                    todo1 &= ~((2ull << (i - 64)) - 1ull);
                    r0 |= rdl(b0, i - 64); r1 |= rdl(b1, i - 64);
                }
            }
            if (lane < nk) s_keep[lane] = k0;
            if (lane + 64 < nk) s_keep[lane + 64] = k1;
        }
        if (lane == 0) {
            s_nkeep = nk;
            const int flagged = nk | (s_bad ? PP_NDETS_NONFINITE : 0);   // pp_get_detections / pp_predict: PP_ERR_NUMERIC
            if constexpr (PERCLS) {
                p.cls_cnt[(size_t)b * ncls + kc] = flagged;     // k_gather_classes sums the counts and ORs the flags
            } else {
                p.n_dets[b] = flagged;
                if (p.n_dets_host != nullptr) p.n_dets_host[b] = flagged;
            }
        }
    }
    __syncthreads();

    // ---- direction flip + lidar -> camera, in keep (descending score) order ----
    const int nk = s_nkeep;
    if (tid < nk) {
        const int i = s_keep[tid];
        pp_detection d;
        float r = s_box[i][6];
        // model/voxelnet.py:1297-1310: the flip exists only with use_direction_classifier
        const bool opp = p.use_dir && ((r > 0.f) != (s_dir[i] == 1));
        if (p.use_dir) r = (float)((double)r + (opp ? 3.141592653589793 : 0.0));  // f32 += f64 (numpy in-place add)
        const float* M = p.calib + (size_t)b * 16;
        const double x = s_box[i][0], y = s_box[i][1], z = s_box[i][2];
#pragma unroll
        for (int q = 0; q < 3; ++q)
            d.box3d_camera[q] = x * (double)M[q * 4 + 0] + y * (double)M[q * 4 + 1] + z * (double)M[q * 4 + 2] +
                                (double)M[q * 4 + 3];
        d.box3d_camera[3] = (double)s_box[i][4];  // l
        d.box3d_camera[4] = (double)s_box[i][5];  // h
        d.box3d_camera[5] = (double)s_box[i][3];  // w
        d.box3d_camera[6] = (double)r;
#pragma unroll
        for (int q = 0; q < 6; ++q) d.box3d_lidar[q] = s_box[i][q];
        d.box3d_lidar[6] = r;
        d.score = s_score[i];
        d.label = s_label[i];
        d.dir_label = s_dir[i];
        d.anchor_index = s_anchor[i];
        d.reserved = 0;
        if constexpr (PERCLS) {     // segment (b, kc) of the scratch k_gather_classes reads
            p.cls_dets[((size_t)b * ncls + kc) * p.post_max + tid] = d;
        } else {
            p.dets[(size_t)b * p.post_max + tid] = d;
            if (p.dets_host != nullptr) p.dets_host[(size_t)b * p.post_max + tid] = d;
        }
        if constexpr (PROJ) {
            const double* M2 = p.p2 + (size_t)b * 16;
            double P[9], bb[4];
#pragma unroll
            for (int q = 0; q < 3; ++q) { P[3 * q] = M2[4 * q]; P[3 * q + 1] = M2[4 * q + 1]; P[3 * q + 2] = M2[4 * q + 2]; }
            box3d_to_bbox_dev(d.box3d_camera, P, bb);
            double* o = PERCLS ? p.cls_bbox + (((size_t)b * ncls + kc) * p.post_max + tid) * 4
                               : p.bbox + ((size_t)b * p.post_max + tid) * 4;
            double* oh = (!PERCLS && p.bbox_host != nullptr) ? p.bbox_host + ((size_t)b * p.post_max + tid) * 4 : nullptr;
#pragma unroll
            for (int q = 0; q < 4; ++q) { o[q] = bb[q]; if (oh != nullptr) oh[q] = bb[q]; }
        }
    }
}

// Per-class rule, second launch: one workgroup per frame lays the classes' segments end to end.  The running sum of the
// (clamped) class counts is the exclusive prefix every thread needs; rows are copied as 8-byte words, coalesced, to the
// device rows and -- the fused path -- their page-locked twins.  The frame's count is the total, flagged when any class's
// workgroup flagged the frame.
#define GT 256
static_assert(sizeof(pp_detection) % 8 == 0, "k_gather_classes copies detections as 8-byte words");
__global__ __launch_bounds__(GT) void k_gather_classes(PostParams p) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ncls = p.ncls, pm = p.post_max;
    const size_t rows = (size_t)ncls * pm;       // row stride of a frame in dets / bbox
    constexpr int DW = (int)(sizeof(pp_detection) / 8);
    unsigned long long* dd = reinterpret_cast<unsigned long long*>(p.dets + (size_t)b * rows);
    unsigned long long* dh = (p.dets_host != nullptr) ? reinterpret_cast<unsigned long long*>(p.dets_host + (size_t)b * rows) : nullptr;
    int off = 0, flag = 0;
    for (int c = 0; c < ncls; ++c) {
        const int raw = p.cls_cnt[(size_t)b * ncls + c];
        flag |= raw & PP_NDETS_NONFINITE;
        const int cnt = min(max(raw & ~PP_NDETS_NONFINITE, 0), pm);
        const size_t seg = ((size_t)b * ncls + c) * pm;
        const unsigned long long* sd = reinterpret_cast<const unsigned long long*>(p.cls_dets + seg);
        for (int w = tid; w < cnt * DW; w += GT) {
            const unsigned long long v = sd[w];
            dd[(size_t)off * DW + w] = v;
            if (dh != nullptr) dh[(size_t)off * DW + w] = v;
        }
        if (p.p2 != nullptr) {
            const double* sb = p.cls_bbox + seg * 4;
            double* ob = p.bbox + ((size_t)b * rows + off) * 4;
            double* oh = (p.bbox_host != nullptr) ? p.bbox_host + ((size_t)b * rows + off) * 4 : nullptr;
            for (int w = tid; w < cnt * 4; w += GT) {
                const double v = sb[w];
                ob[w] = v;
                if (oh != nullptr) oh[w] = v;
            }
        }
        off += cnt;
    }
    if (tid == 0) {
        p.n_dets[b] = off | flag;
        if (p.n_dets_host != nullptr) p.n_dets_host[b] = off | flag;
    }
}

template <bool PERCLS>
static void launch_post_rule(const PostParams& p, hipStream_t s) {
    const bool proj = p.p2 != nullptr;
    const dim3 grid = PERCLS ? dim3(p.batch, p.ncls) : dim3(p.batch);
    if (p.nms_mode == PP_NMS_ROTATED) {
        if (proj) PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_ROTATED, true, PERCLS>), grid, dim3(PT), 0, s, p);
        else PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_ROTATED, false, PERCLS>), grid, dim3(PT), 0, s, p);
    } else if (p.nms_mode == PP_NMS_SOFT) {
        if (proj) PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_SOFT, true, PERCLS>), grid, dim3(PT), 0, s, p);
        else PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_SOFT, false, PERCLS>), grid, dim3(PT), 0, s, p);
    } else {
        if (proj) PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_STANDUP, true, PERCLS>), grid, dim3(PT), 0, s, p);
        else PP_LAUNCH("k_postprocess", (k_postprocess<PP_NMS_STANDUP, false, PERCLS>), grid, dim3(PT), 0, s, p);
    }
}

void launch_postprocess(const PostParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    if (p.class_nms == PP_CLASS_NMS_PER_CLASS) {
        launch_post_rule<true>(p, s);
        PP_LAUNCH("k_gather_classes", k_gather_classes, dim3(p.batch), dim3(GT), 0, s, p);
    } else {
        launch_post_rule<false>(p, s);
    }
}
