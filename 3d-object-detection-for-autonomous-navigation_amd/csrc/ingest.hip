// Live-camera ingest (pp_ingest_pointcloud2*): raw sensor_msgs/PointCloud2 bytes -> the float32 [sum n_b, 3] lidar-frame
// points and the frame offsets the voxeliser reads, without the host touching a point.  Restates
// ingest.pointcloud2_to_xyz(...)[first::decimate] followed by ingest.realsense_to_lidar (load_data.py:2433-2443):
//
//   record i = row * width + col of a frame sits at row * row_step + col * point_step; x y z are read at their field
//   offsets (FLOAT32 or FLOAT64, either byte order, no alignment assumed);
//   a record is finite when its three coordinates are; rank = finite records before it in message order;
//   it is kept when finite, rank >= first and (rank - first) % decimate == 0, as output row (rank - first) / decimate;
//   a kept point becomes ((p . r) . r2) + lift in float64 -- every 3-term dot product summed left to right, no fused
//   multiply-add, which is what numpy's dot computes for these shapes -- and is rounded to float32 once.
//
// Three launches, ordered by the stream alone (no workgroup waits for another):
//   k_ingest_count    one wave per chunk of ING_CHUNK records: ballot + popcount of the finite flags -> chunk counts
//   k_ingest_scan     one workgroup: a wave per frame scans its chunk counts -> chunk bases, the frame's finite and kept
//                     counts; then the frame offsets
//   k_ingest_scatter  re-reads the chunks; a finite record's rank is its chunk's base + the finite lanes below it
//
// pp_ingest_pointcloud2_fields* (rows of F > 3 floats): the count and the scan are the same launches -- validity is x y z's
// alone --, and k_ingest_scatter_f<F> writes x y z and the frame's F - 3 feature columns (ingest_dev.h: ing_feature) as one
// row, one 16-byte store for F = 4.
//
// Depth-image ingest (pp_ingest_depth*): raw sensor_msgs/Image bytes of a depth camera (16UC1 / mono16 units of
// depth_scale, or 32FC1 metres) -> the float32 [sum n_b, 3] lidar-frame points and the frame offsets the voxeliser reads.
// The sibling of the PointCloud2 feed: it produces, from the 0.6 MB depth image, the resident points that feed produces from
// the 6-10 MB PointCloud2 message a point-cloud node computes from that image.  Restates ingest.depth_ingest_np:
//
//   pixel (v, u) of a frame sits at v * row_step + u * itemsize (either byte order, no alignment assumed);
//   16UC1: z = depth_scale * (float)d, one float32 product, valid when d != 0;
//   32FC1: z is the stored value, valid when it is finite and > 0 (depth_scale is not applied: REP 118);
//   both: valid only when z > z_min && z <= z_max (0 and +inf leave the conditions above as they are);
//   a valid pixel is the float32 point x = z * (((float)u - ppx) / fx), y = z * (((float)v - ppy) / fy), z -- every
//   operation rounded separately, IEEE division: the pinhole (no distortion) case of the camera vendor's published
//   rs2_deproject_pixel_to_point.  PARITY WITH THE BYTES THE CAMERA DRIVER'S POINT-CLOUD BLOCK PUBLISHES IS NOT PINNED:
//   neither the vendor library nor its ROS node exists where this project is built and tested.  What is pinned is
//   everything behind the point:
//   rank = valid pixels before it in row-major order; it is kept when rank >= first and (rank - first) % decimate == 0,
//   as output row (rank - first) / decimate; a kept point is widened to float64, becomes ((p . r) . r2) + lift exactly as
//   above (ingest_dev.h: ing_transform) and is rounded to float32 once.
//
// Three launches, ordered by the stream alone (no workgroup waits for another):
//   k_depth_count    one wave per chunk of ING_CHUNK pixels: ballot + popcount of the valid flags -> chunk counts
//   k_depth_scan     k_ingest_scan's body (ingest_dev.h): chunk bases, the frames' valid and kept counts, the frame offsets
//   k_depth_scatter  re-reads the chunks; a valid pixel's rank is its chunk's base + the valid lanes below it + the steps
//                    before; only kept pixels are deprojected and transformed
//
// Camera-rig ingest (pp_ingest_rig_*): S sources -- depth images, or PointCloud2 messages -- into B frames, each source
// under its own selection (first, decimate) and its own camera -> lidar transform.  The resident points of a frame are
// the kept points of its sources in source order, back to back; per source the rule is the PointCloud2 / depth one above,
// restarted: validity, rank, selection, the float64 transform and the single rounding (ingest_dev.h holds the per-record
// functions and the phase bodies all of them share).  Restates ingest.rig_depth_ingest_np / rig_ingest_np.
//
// Three launches whatever S is, ordered by the stream alone (no workgroup waits for another):
//   k_rig_count    grid (chunks, source): one wave per chunk of ING_CHUNK records -> chunk counts [S][stride]
//   k_rig_scan     one workgroup: a wave per source scans its chunk counts -> chunk bases, the source's finite and kept
//                  counts (its own first / decimate); then one thread walks the S sources and B frames once: out_base[s]
//                  = kept of the earlier sources of its frame, offsets[b] = kept of all sources in front of frame b, and the
//                  frames' sums for pp_ingest_info
//   k_rig_scatter  grid (chunks, source): a kept record of source s goes to row offsets[frame(s)] + out_base[s] +
//                  (rank - first) / decimate, transformed by the source's own matrices (read from the source table: S x 168
//                  bytes do not fit a kernel argument)
//
// pp_ingest_rig_pointcloud2_fields* (rows of F > 3 floats): the same count and scan, and k_rig_scatter_f<F>, which writes
// x y z and the source's F - 3 feature columns (ingest_dev.h: ing_feature) as one row, one 16-byte store for F = 4.
//
// The k_ingest_* / k_depth_* / k_rig_* names above are the names the launches are profiled under (IngNames below; the
// tools and DESIGN.md read them).  The kernels behind them are one per phase and record type: k_ing_count<Frame> for every
// count, k_ing_scan<Frame> / k_rig_scan<Frame>, and k_ing_scatter<Frame, F> / k_rig_scatter<Frame, F>, thin wrappers that
// say where a chunk's selection, matrices and first output row come from; the bodies are ingest_dev.h's.
#include "pp_common.h"
#include "ingest_dev.h"

namespace {

// One count kernel per record type: a plain call launches it over its frames, a rig call over its sources.
template <typename Frame>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_ing_count(const uint8_t* __restrict__ raw,
                                                                  const Frame* __restrict__ frames, int stride,
                                                                  int* __restrict__ chunk_cnt) {
    ing_count_chunk(raw, frames, stride, chunk_cnt);
}

// One workgroup of 16 waves; wave w scans frames w, w + 16, ...; thread 0 then sums the kept counts into the offsets.
template <typename Frame>
__global__ __launch_bounds__(1024) void k_ing_scan(const Frame* __restrict__ frames, int batch, int stride, int first,
                                                   int decimate, const int* __restrict__ chunk_cnt,
                                                   int* __restrict__ chunk_base, int* __restrict__ finite,
                                                   int* __restrict__ kept, int* __restrict__ offsets) {
    ingest_scan_frames(frames, batch, stride, first, decimate, chunk_cnt, chunk_base, finite, kept, offsets);
}

// One workgroup of 16 waves; wave w scans sources w, w + 16, ...; thread 0 then walks the sources and the frames once
// (S + B steps: S <= PP_RIG_MAX_SOURCES * max_batch).
template <typename Frame>
__global__ __launch_bounds__(1024) void k_rig_scan(const Frame* __restrict__ frames, const RigSource* __restrict__ src,
                                                   int sources, int batch, int stride, const int* __restrict__ chunk_cnt,
                                                   int* __restrict__ chunk_base, int* __restrict__ src_finite,
                                                   int* __restrict__ src_kept, int* __restrict__ out_base,
                                                   int* __restrict__ finite, int* __restrict__ kept,
                                                   int* __restrict__ offsets) {
    const int lane = threadIdx.x & (PP_WAVE - 1), wave = threadIdx.x >> 6;
    for (int s = wave; s < sources; s += 16) {
        const int carry = ing_scan_chunks(chunk_cnt, chunk_base, (size_t)s * stride, frames[s].nchunks);
        if (lane == 0) {
            const int first = src[s].first, decimate = src[s].decimate;
            src_finite[s] = carry;
            src_kept[s] = ing_kept(carry, first, decimate);
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        // (the host checked the frame map: it starts at 0, never decreases, skips no frame and ends at batch - 1)
        int off = 0, s = 0;
        for (int b = 0; b < batch; ++b) {
            offsets[b] = off;
            int base = 0, fin = 0;
            for (; s < sources && src[s].frame == b; ++s) {
                out_base[s] = base;
                base += src_kept[s];
                fin += src_finite[s];
            }
            finite[b] = fin;
            kept[b] = base;
            off += base;
        }
        offsets[batch] = off;
    }
}

template <int F>
__device__ __forceinline__ IngCols<F - 3> ing_cols(const IngFeat* __restrict__ feats, int y) {
    IngCols<F - 3> ft;
    if constexpr (F > 3) {
#pragma unroll
        for (int j = 0; j < F - 3; ++j) ft.c[j] = feats[(size_t)y * (F - 3) + j];
    }
    return ft;
}

// The scatter of a plain call: one selection and one transform for every frame, as kernel arguments; frame b's rows
// start at offsets[b].  feats: [batch][F - 3], not read for F = 3.
template <typename Frame, int F>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_ing_scatter(const uint8_t* __restrict__ raw,
                                                                    const Frame* __restrict__ frames, int stride,
                                                                    int first, int decimate, IngXform xf,
                                                                    const int* __restrict__ chunk_base,
                                                                    const int* __restrict__ offsets,
                                                                    float* __restrict__ out, long long out_rows,
                                                                    const IngFeat* __restrict__ feats) {
    const int b = blockIdx.y;
    const Frame f = frames[b];
    const int c = ing_wave_chunk();
    if (c >= f.nchunks) return;
    ing_scatter_chunk<Frame, F>(raw + f.byte_off, f, c, chunk_base[(size_t)b * stride + c], first, decimate, xf,
                                ing_cols<F>(feats, b), offsets[b], out, out_rows);
}

// The scatter of a rig call: source s's selection and transform come from the source table, its rows start at
// offsets[frame(s)] + out_base[s].  feats: [sources][F - 3], not read for F = 3.
template <typename Frame, int F>
__global__ __launch_bounds__(PP_WAVE * ING_WAVES) void k_rig_scatter(const uint8_t* __restrict__ raw,
                                                                    const Frame* __restrict__ frames,
                                                                    const RigSource* __restrict__ src, int batch, int stride,
                                                                    const int* __restrict__ chunk_base,
                                                                    const int* __restrict__ out_base,
                                                                    const int* __restrict__ offsets,
                                                                    float* __restrict__ out, long long out_rows,
                                                                    const IngFeat* __restrict__ feats) {
    const int s = blockIdx.y;
    const Frame f = frames[s];
    const int c = ing_wave_chunk();
    if (c >= f.nchunks) return;
    const RigSource& g = src[s];
    const int frame = g.frame;
    if (frame < 0 || frame >= batch) return;       // (never: the host checked the frame map)
    IngXform xf;
#pragma unroll
    for (int k = 0; k < 9; ++k) { xf.r[k] = g.r[k]; xf.r2[k] = g.r2[k]; }
#pragma unroll
    for (int k = 0; k < 3; ++k) xf.lift[k] = g.lift[k];
    const long long row0 = (long long)offsets[frame] + out_base[s];
    if (row0 < 0) return;                          // (never: both are sums of kept counts)
    ing_scatter_chunk<Frame, F>(raw + f.byte_off, f, c, chunk_base[(size_t)s * stride + c], g.first, g.decimate, xf,
                                ing_cols<F>(feats, s), row0, out, out_rows);
}

// the names the launches are profiled under: [rig call][count, scan, scatter, scatter of F = 4 rows]
template <typename Frame> struct IngNames;
template <> struct IngNames<IngFrame> {
    static constexpr const char* n[2][4] = {{"k_ingest_count", "k_ingest_scan", "k_ingest_scatter", "k_ingest_scatter_f<4>"},
                                            {"k_rig_count<pc2>", "k_rig_scan<pc2>", "k_rig_scatter<pc2>", "k_rig_scatter_f<4>"}};
};
template <> struct IngNames<DepthFrame> {
    static constexpr const char* n[2][4] = {{"k_depth_count", "k_depth_scan", "k_depth_scatter", nullptr},
                                            {"k_rig_count<depth>", "k_rig_scan<depth>", "k_rig_scatter<depth>", nullptr}};
};

template <typename Frame, int F>
void launch_scatter(const IngestParamsT<Frame>& p, hipStream_t s, dim3 grid, dim3 block, const char* name) {
    if (p.src)
        PP_LAUNCH(name, (k_rig_scatter<Frame, F>), grid, block, 0, s, p.raw, p.frames, p.src, p.batch, p.stride, p.chunk_base,
                  p.out_base, p.offsets, p.out, p.out_rows, p.feats);
    else
        PP_LAUNCH(name, (k_ing_scatter<Frame, F>), grid, block, 0, s, p.raw, p.frames, p.stride, p.first, p.decimate,
                  ing_xform_of(p.r, p.r2, p.lift), p.chunk_base, p.offsets, p.out, p.out_rows, p.feats);
}

// count, scan, scatter: three launches whatever the call, grid (chunks, records) for the first and the last
template <typename Frame>
void launch(const IngestParamsT<Frame>& p, hipStream_t s) {
    if (p.batch <= 0 || p.records <= 0) return;
    const char* const* name = IngNames<Frame>::n[p.src != nullptr];
    const dim3 grid((p.stride + ING_WAVES - 1) / ING_WAVES, p.records), block(PP_WAVE * ING_WAVES);
    if (p.stride > 0) PP_LAUNCH(name[0], k_ing_count<Frame>, grid, block, 0, s, p.raw, p.frames, p.stride, p.chunk_cnt);
    if (p.src)
        PP_LAUNCH(name[1], k_rig_scan<Frame>, dim3(1), dim3(1024), 0, s, p.frames, p.src, p.records, p.batch, p.stride,
                  p.chunk_cnt, p.chunk_base, p.src_finite, p.src_kept, p.out_base, p.finite, p.kept, p.offsets);
    else
        PP_LAUNCH(name[1], k_ing_scan<Frame>, dim3(1), dim3(1024), 0, s, p.frames, p.batch, p.stride, p.first, p.decimate,
                  p.chunk_cnt, p.chunk_base, p.finite, p.kept, p.offsets);
    if (p.stride <= 0) return;
    if constexpr (std::is_same<Frame, IngFrame>::value) {
        // (nfeat == 1: the C-ABI holds nfeat to F - 3 and pp_create F to 3 or 4; an image has no field)
        if (p.nfeat > 0) return launch_scatter<Frame, 4>(p, s, grid, block, name[3]);
    }
    launch_scatter<Frame, 3>(p, s, grid, block, name[2]);
}

}  // namespace

int ingest_chunks(int n_rec) { return (n_rec + ING_CHUNK - 1) / ING_CHUNK; }

void launch_ingest(const IngestParamsT<IngFrame>& p, hipStream_t s) { launch(p, s); }
void launch_ingest(const IngestParamsT<DepthFrame>& p, hipStream_t s) { launch(p, s); }
