// Depth-image ingest (pp_ingest_depth*): raw sensor_msgs/Image bytes of a depth camera (16UC1 / mono16 units of
// depth_scale, or 32FC1 metres) -> the float32 [sum n_b, 3] lidar-frame points and the frame offsets the voxeliser reads.
// The sibling of ingest.hip: it produces, from the 0.6 MB depth image, the resident points that ingest.hip produces from
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
//   in ingest.hip (ingest_dev.h: ing_transform) and is rounded to float32 once.
//
// Three launches, ordered by the stream alone (no workgroup waits for another):
//   k_depth_count    one wave per chunk of DEP_CHUNK pixels: ballot + popcount of the valid flags -> chunk counts
//   k_depth_scan     ingest.hip's scan (ingest_dev.h): chunk bases, the frames' valid and kept counts, the frame offsets
//   k_depth_scatter  re-reads the chunks; a valid pixel's rank is its chunk's base + the valid lanes below it + the steps
//                    before; only kept pixels are deprojected and transformed
#include "pp_common.h"
#include "ingest_dev.h"

namespace {

// the chunking is ingest.hip's (ingest_dev.h): rig_ingest.hip runs both feeds' records through one set of kernels
constexpr int DEP_ITER = ING_ITER;                // 64-pixel steps of a wave
constexpr int DEP_CHUNK = ING_CHUNK;              // pixels per chunk (one wave)
constexpr int DEP_WAVES = ING_WAVES;              // chunks per workgroup

// (dep_read / dep_deproject, the per-pixel decode and validity: ingest_dev.h, shared with rig_ingest.hip)

__global__ __launch_bounds__(PP_WAVE * DEP_WAVES) void k_depth_count(const uint8_t* __restrict__ raw,
                                                                    const DepthFrame* __restrict__ frames, int stride,
                                                                    int* __restrict__ chunk_cnt) {
    const int b = blockIdx.y;
    const DepthFrame f = frames[b];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * DEP_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;                    // (the same for every lane of the wave)
    const uint8_t* base = raw + f.byte_off;
    int cnt = 0;
#pragma unroll 2
    for (int k = 0; k < DEP_ITER; ++k) {
        const int i = c * DEP_CHUNK + k * PP_WAVE + lane;
        float z;
        const bool ok = i < f.n_pix && dep_read(base, f, i, z);
        cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) chunk_cnt[(size_t)b * stride + c] = cnt;
}

__global__ __launch_bounds__(1024) void k_depth_scan(const DepthFrame* __restrict__ frames, int batch, int stride,
                                                     int first, int decimate, const int* __restrict__ chunk_cnt,
                                                     int* __restrict__ chunk_base, int* __restrict__ valid,
                                                     int* __restrict__ kept, int* __restrict__ offsets) {
    ingest_scan_frames(frames, batch, stride, first, decimate, chunk_cnt, chunk_base, valid, kept, offsets);
}

__global__ __launch_bounds__(PP_WAVE * DEP_WAVES) void k_depth_scatter(const uint8_t* __restrict__ raw,
                                                                      const DepthFrame* __restrict__ frames, int stride,
                                                                      int first, int decimate, IngXform xf,
                                                                      const int* __restrict__ chunk_base,
                                                                      const int* __restrict__ offsets,
                                                                      float* __restrict__ out, long long out_rows) {
    const int b = blockIdx.y;
    const DepthFrame f = frames[b];
    const int lane = threadIdx.x & (PP_WAVE - 1);
    const int c = blockIdx.x * DEP_WAVES + (threadIdx.x >> 6);
    if (c >= f.nchunks) return;
    const uint8_t* base = raw + f.byte_off;
    const long long row0 = offsets[b];
    int run = chunk_base[(size_t)b * stride + c];
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int k = 0; k < DEP_ITER; ++k) {
        const int i = c * DEP_CHUNK + k * PP_WAVE + lane;
        float z = 0.0f;
        const bool ok = i < f.n_pix && dep_read(base, f, i, z);
        const unsigned long long m = __ballot(ok);
        const int r = run + __popcll(m & below) - first;
        run += __popcll(m);
        if (ok && r >= 0 && r % decimate == 0) {
            const long long row = row0 + r / decimate;
            if (row < out_rows) {                  // (always: the host sized the call from the frames' bounds)
                double p[3];
                float o[3];
                dep_deproject(f, i, z, p);
                ing_transform(p, xf, o);
                out[row * 3 + 0] = o[0];
                out[row * 3 + 1] = o[1];
                out[row * 3 + 2] = o[2];
            }
        }
    }
}

}  // namespace

int depth_chunks(int n_pix) { return (n_pix + DEP_CHUNK - 1) / DEP_CHUNK; }

void launch_depth_ingest(const DepthIngestParams& p, hipStream_t s) {
    if (p.batch <= 0) return;
    const dim3 grid((p.stride + DEP_WAVES - 1) / DEP_WAVES, p.batch), block(PP_WAVE * DEP_WAVES);
    if (p.stride > 0)
        PP_LAUNCH("k_depth_count", k_depth_count, grid, block, 0, s, p.raw, p.frames, p.stride, p.chunk_cnt);
    PP_LAUNCH("k_depth_scan", k_depth_scan, dim3(1), dim3(1024), 0, s, p.frames, p.batch, p.stride, p.first, p.decimate,
              p.chunk_cnt, p.chunk_base, p.finite, p.kept, p.offsets);
    if (p.stride > 0) {
        const IngXform xf = ing_xform_of(p);
        PP_LAUNCH("k_depth_scatter", k_depth_scatter, grid, block, 0, s, p.raw, p.frames, p.stride, p.first, p.decimate,
                  xf, p.chunk_base, p.offsets, p.out, p.out_rows);
    }
}
