// hpe_draw.hip — detections and pose axes drawn into video frames on the device: the last stage of the
// reference's webcam loop, drawDetections (blazeFaceDetectorH5.py:175-219, drawAxis_simo :64-77,
// EulerToMatrix :40-62), without its text.  Two stages (include/hpe.h states the rules in full):
//   hpe_pose_prims   detections -> a table of integer primitives, 11 rows per face (box outline, six
//                    keypoint disks, three axis segments, one reserved row of zeros); float64, every
//                    operation rounded on its own (contraction is off in this file); one thread per
//                    detection
//   hpe_draw(_nv12)  a small tiled rasteriser for any such table, pure integer, bit-exact: packed
//                    3-byte pixels in place, or NV12 planes (luma per pixel, chroma per 2 x 2 block)
// The rasteriser: one workgroup of DRAW_T = 256 threads per tile of DRAW_TW x DRAW_TH = 128 x 8 pixels,
// lanes along x, one thread per 2 x 2 block of pixels in both kernels, so that the NV12 kernel takes the
// luma and the chroma from one decision and the packed kernel stores 6 adjacent bytes per row.  The
// workgroup reads n_prims[f] (a scalar load) and leaves at once if nothing is live.  Otherwise the live
// rows are taken DRAW_LIST = 256 at a time, one row per thread: validity, then the row's bounding box
// against the tile (int32); the survivors are compacted in row order into an LDS list (ballot and a
// population count within a wave, then the waves' offsets), and every thread walks the list for its
// four pixels, carrying the winner (row index and colour) from pass to pass: a later row paints over an
// earlier one, and P has no cap.  In the walk the pixel is tested against the row's bounding box before
// any product, so every product but the segment's last two squares fits int32 (|v|, |d| < 2^15).
// draw_covers, draw_cull and draw_walk exist once; the two kernels differ in the store.
// Only covered pixels are stored, with byte stores: a frame row may start at any byte address.
// LDS (static): the list, 48 B x 256 = 12 KB, the colour table 1 KB.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/hpe.h"
#include "hpe_boxes.h"
#include "hpe_common.h"

#pragma clang fp contract(off)

#define DRAW_T 256
#define DRAW_LIST DRAW_T   // one row per thread per culling pass, so a pass never overfills the list
#define DRAW_BW 64         // 2 x 2 blocks per tile row: one per lane
#define DRAW_BH (DRAW_T / DRAW_BW)
#define DRAW_TW (2 * DRAW_BW)
#define DRAW_TH (2 * DRAW_BH)

struct DrawPrim {
  int kind, x0, y0, x1, y1, size, colour, row;
  int bx0, by0, bx1, by1;   // the inclusive bounding box of the covered pixels
};

struct DrawArgs {
  uint8_t* p0;   // packed frames, or the luma planes
  uint8_t* p1;   // the chroma planes (NV12)
  int64_t rs0, fs0, rs1, fs1;
  int h, w, tiles_x, tiles_y;
  const int32_t* prims;
  const int32_t* n_prims;
  int P;
  const uint8_t* colours;
  int n_colours;
};

__device__ __forceinline__ bool draw_coord_ok(int c) { return c >= -HPE_DRAW_MAX_DIM && c <= HPE_DRAW_MAX_DIM; }

// the pixel at (x, y), which lies inside p's bounding box
__device__ __forceinline__ bool draw_covers(const DrawPrim& p, int x, int y) {
  if (p.kind == 1) {
    const int h1 = (p.size - 1) / 2, m = p.size / 2;
    // the hole, from the outer box's corners: xa + h1 + 1 = bx0 + m + h1 + 1
    const int hx0 = p.bx0 + m + h1 + 1, hx1 = p.bx1 - m - h1 - 1;
    const int hy0 = p.by0 + m + h1 + 1, hy1 = p.by1 - m - h1 - 1;
    return !(x >= hx0 && x <= hx1 && y >= hy0 && y <= hy1);
  }
  if (p.kind == 2) {
    const int dx = x - p.x0, dy = y - p.y0;
    return dx * dx + dy * dy <= p.size * p.size;
  }
  const int dx = p.x1 - p.x0, dy = p.y1 - p.y0;
  const int vx = x - p.x0, vy = y - p.y0;
  const int L2 = dx * dx + dy * dy;
  const int t = vx * dx + vy * dy;
  const int th2 = p.size * p.size;
  if (t <= 0) return 4 * (int64_t)(vx * vx + vy * vy) <= th2;
  if (t >= L2) {
    const int ux = x - p.x1, uy = y - p.y1;
    return 4 * (int64_t)(ux * ux + uy * uy) <= th2;
  }
  const int64_t cross = (int64_t)(vx * dy - vy * dx);
  return 4 * cross * cross <= (int64_t)th2 * (int64_t)L2;
}

// row `row` of the frame's table: valid and touching the tile [tx0, tx1] x [ty0, ty1]?  Fills p.
__device__ __forceinline__ bool draw_cull(const int32_t* r, int row, int n_colours, int tx0, int ty0, int tx1,
                                          int ty1, DrawPrim& p) {
  const int4 a = *(const int4*)r;   // rows are 32 B apart in an int32 table
  const int4 b = *(const int4*)(r + 4);
  p.kind = a.x;
  p.x0 = a.y;
  p.y0 = a.z;
  p.x1 = a.w;
  p.y1 = b.x;
  p.size = b.y;
  p.colour = b.z;
  p.row = row;
  const bool ok = p.kind >= 1 && p.kind <= 3 && draw_coord_ok(p.x0) && draw_coord_ok(p.y0) && draw_coord_ok(p.x1) &&
                  draw_coord_ok(p.y1) && p.size >= (p.kind == 2 ? 0 : 1) && p.size <= HPE_DRAW_MAX_SIZE &&
                  p.colour >= 0 && p.colour < n_colours;
  if (!ok) return false;
  const int m = p.kind == 2 ? p.size : p.size / 2;
  const bool dot = p.kind == 2;
  p.bx0 = (dot ? p.x0 : min(p.x0, p.x1)) - m;
  p.bx1 = (dot ? p.x0 : max(p.x0, p.x1)) + m;
  p.by0 = (dot ? p.y0 : min(p.y0, p.y1)) - m;
  p.by1 = (dot ? p.y0 : max(p.y0, p.y1)) + m;
  return p.bx0 <= tx1 && p.bx1 >= tx0 && p.by0 <= ty1 && p.by1 >= ty0;
}

// The winners of the thread's 2 x 2 block at (px, py): wrow[k] / wcol[k] for pixel (px + (k & 1),
// py + (k >> 1)), wrow < 0 where no row covers it.  Returns false (uniformly) when the frame has no
// live rows.  scol: the colour table, bytes 0..2 packed into a word.
__device__ __forceinline__ bool draw_walk(const DrawArgs& a, int64_t f, int tx0, int ty0, int px, int py,
                                          int wrow[4], int wcol[4], uint32_t* scol) {
  __shared__ DrawPrim list[DRAW_LIST];
  __shared__ int wcnt[DRAW_T / 64];
  const int n = min(max(a.n_prims[f], 0), a.P);
  if (n == 0) return false;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < a.n_colours; c += DRAW_T) {
    const uint8_t* q = a.colours + 4 * c;
    scol[c] = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
  }
  const int tx1 = min(tx0 + DRAW_TW, a.w) - 1, ty1 = min(ty0 + DRAW_TH, a.h) - 1;
  const int32_t* tab = a.prims + f * a.P * HPE_DRAW_PRIM_WORDS;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    wrow[k] = -1;
    wcol[k] = 0;
  }
  for (int base = 0; base < n; base += DRAW_LIST) {
    DrawPrim p;
    const int row = base + tid;
    const bool keep = row < n && draw_cull(tab + (int64_t)row * HPE_DRAW_PRIM_WORDS, row, a.n_colours, tx0, ty0, tx1,
                                           ty1, p);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wcnt[wave] = __popcll(m);
    __syncthreads();   // also: the walk of the pass before is over, the list may be overwritten
    int off = 0, total = 0;
#pragma unroll
    for (int v = 0; v < DRAW_T / 64; ++v) {
      const int c = wcnt[v];
      if (v < wave) off += c;
      total += c;
    }
    if (keep) list[off + __popcll(m & ((1ull << lane) - 1ull))] = p;
    __syncthreads();
    for (int i = 0; i < total; ++i) {
      const DrawPrim& e = list[i];
      if (e.bx0 > px + 1 || e.bx1 < px || e.by0 > py + 1 || e.by1 < py) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = px + (k & 1), y = py + (k >> 1);
        if (x >= e.bx0 && x <= e.bx1 && y >= e.by0 && y <= e.by1 && draw_covers(e, x, y)) {
          wrow[k] = e.row;
          wcol[k] = e.colour;
        }
      }
    }   // no barrier here: wcnt was last read before the one above, the list is rewritten after the next
  }
  return true;
}

template <bool NV12>
__global__ void __launch_bounds__(DRAW_T) draw_kernel(DrawArgs a) {
  __shared__ uint32_t scol[256];
  const int tiles = a.tiles_x * a.tiles_y;
  const int64_t f = blockIdx.x / tiles;
  const int tile = blockIdx.x % tiles;
  const int tx0 = (tile % a.tiles_x) * DRAW_TW, ty0 = (tile / a.tiles_x) * DRAW_TH;
  const int px = tx0 + 2 * (threadIdx.x & 63), py = ty0 + 2 * (threadIdx.x >> 6);
  int wrow[4], wcol[4];
  if (!draw_walk(a, f, tx0, ty0, px, py, wrow, wcol, scol)) return;
  int best = -1, bcol = 0;   // the block's highest winning row (NV12 chroma)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = px + (k & 1), y = py + (k >> 1);
    if (wrow[k] < 0 || x >= a.w || y >= a.h) continue;   // wcol is a checked colour index from here on
    const uint32_t c = scol[wcol[k]];
    if (NV12) {
      a.p0[f * a.fs0 + y * a.rs0 + x] = (uint8_t)c;
      if (wrow[k] > best) {
        best = wrow[k];
        bcol = wcol[k];
      }
    } else {
      uint8_t* q = a.p0 + f * a.fs0 + y * a.rs0 + 3 * (int64_t)x;
      q[0] = (uint8_t)c;
      q[1] = (uint8_t)(c >> 8);
      q[2] = (uint8_t)(c >> 16);
    }
  }
  if (NV12 && best >= 0) {   // px < w and py < h here, and both are even
    const uint32_t c = scol[bcol];
    uint8_t* q = a.p1 + f * a.fs1 + (py >> 1) * a.rs1 + px;
    q[0] = (uint8_t)(c >> 8);
    q[1] = (uint8_t)(c >> 16);
  }
}

// ------------------------------------------------------------------------------------------------
// detections -> primitives
// ------------------------------------------------------------------------------------------------
struct PosePrimArgs {
  const int32_t* count;
  const double* boxes;
  const double* keypoints;
  const float* poses;
  int total, M;   // total = n_images * M
  int src_x0, src_y0;
  double src_w, src_h;
  int box_th, kp_radius, axis_th[3];
  int32_t* prims;
  int32_t* n_prims;
};

__device__ __forceinline__ int draw_clamp_dim(int v) { return min(max(v, -HPE_DRAW_MAX_DIM), HPE_DRAW_MAX_DIM); }

// o + (int) clamp(trunc(s * v), -2^30, 2^30), clamped to +-HPE_DRAW_MAX_DIM; v finite
__device__ __forceinline__ int draw_pix(double v, double s, int o) {
  const double t = fmin(fmax(trunc(s * v), -1073741824.0), 1073741824.0);
  return draw_clamp_dim(o + (int)t);
}

// trunc(v) clamped to +-HPE_DRAW_MAX_DIM; |v| < 2^31
__device__ __forceinline__ int draw_end(double v) { return draw_clamp_dim((int)v); }

__device__ __forceinline__ void draw_put(int32_t* r, int kind, int x0, int y0, int x1, int y1, int size, int colour) {
  const bool on = kind != 0;   // an omitted or non-finite row is a row of zeros
  *(int4*)r = on ? make_int4(kind, x0, y0, x1) : make_int4(0, 0, 0, 0);
  *(int4*)(r + 4) = on ? make_int4(y1, size, colour, 0) : make_int4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(256) pose_prims_kernel(PosePrimArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.total) return;
  const int img = i / a.M, j = i - img * a.M;
  const int c = min(max(a.count[img], 0), a.M);
  if (j == 0) a.n_prims[img] = HPE_DRAW_FACE_PRIMS * c;
  if (j >= c) return;
  int32_t* rows = a.prims + (int64_t)i * (HPE_DRAW_FACE_PRIMS * HPE_DRAW_PRIM_WORDS);
  const double* b = a.boxes + (int64_t)i * 4;
  const double* kp = a.keypoints + (int64_t)i * 12;
  const float* po = a.poses + (int64_t)i * 3;
  const double b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
  const bool box_ok = isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3);
  int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
  if (box_ok) {
    x1 = draw_pix(b0, a.src_w, a.src_x0);
    y1 = draw_pix(b1, a.src_h, a.src_y0);
    x2 = draw_pix(b2, a.src_w, a.src_x0);
    y2 = draw_pix(b3, a.src_h, a.src_y0);
  }
  draw_put(rows, box_ok && a.box_th > 0 ? 1 : 0, x1, y1, x2, y2, a.box_th, 0);
  for (int k = 0; k < 6; ++k) {
    const double kx = kp[2 * k], ky = kp[2 * k + 1];
    const bool ok = box_ok && a.kp_radius >= 0 && isfinite(kx) && isfinite(ky);
    int ix = 0, iy = 0;
    if (ok) {
      ix = draw_pix(kx, a.src_w, a.src_x0);
      iy = draw_pix(ky, a.src_h, a.src_y0);
    }
    draw_put(rows + (1 + k) * HPE_DRAW_PRIM_WORDS, ok ? 2 : 0, ix, iy, ix, iy, a.kp_radius, 1);
  }
  const double yaw = (double)po[0], pitch = (double)po[1], roll = (double)po[2];
  const bool ang_ok = box_ok && isfinite(yaw) && isfinite(pitch) && isfinite(roll);
  int cx = 0, cy = 0, ex[3] = {0, 0, 0}, ey[3] = {0, 0, 0};
  if (ang_ok) {
    const double pi = 3.141592653589793;
    const double tdx = (double)(x1 + x2) / 2.0, tdy = (double)(y1 + y2) / 2.0;
    cx = (int)tdx;
    cy = (int)tdy;
    const double size = trunc((double)min(x2 - x1, y2 - y1) / 2.0);
    const double r = (-roll) / 180.0 * pi, y = (-yaw) / 180.0 * pi, p = (-pitch) / 180.0 * pi;
    const double cr = cos(r), sr = sin(r), cy_ = cos(y), sy = sin(y), cp = cos(p), sp = sin(p);
    const double spsy = sp * sy;
    const double m00 = cy_ * cr;
    const double m10 = spsy * cr + cp * sr;
    const double m01 = -(cy_ * sr);
    const double m11 = -(spsy * sr) + cp * cr;
    const double m02 = sy;
    const double m12 = -(sp * cy_);
    ex[0] = draw_end(m00 * size + tdx);
    ey[0] = draw_end(-(m10 * size) + tdy);
    ex[1] = draw_end(-(m01 * size) + tdx);
    ey[1] = draw_end(m11 * size + tdy);
    ex[2] = draw_end(m02 * size + tdx);
    ey[2] = draw_end(-(m12 * size) + tdy);
  }
  for (int k = 0; k < 3; ++k)
    draw_put(rows + (7 + k) * HPE_DRAW_PRIM_WORDS, ang_ok && a.axis_th[k] > 0 ? 3 : 0, cx, cy, ex[k], ey[k],
             a.axis_th[k], 2 + k);
  draw_put(rows + 10 * HPE_DRAW_PRIM_WORDS, 0, 0, 0, 0, 0, 0, 0);   // the face's 11th row: reserved, draws nothing
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
// (n - 1) * frame_stride + (rows - 1) * row_stride + row_bytes must fit int64
static bool draw_extent_ok(int64_t n, int64_t frame_stride, int64_t rows, int64_t row_stride, int64_t row_bytes) {
  int64_t a, b, s;
  if (__builtin_mul_overflow(n - 1, frame_stride, &a)) return false;
  if (__builtin_mul_overflow(rows - 1, row_stride, &b)) return false;
  if (__builtin_add_overflow(a, b, &s)) return false;
  return !__builtin_add_overflow(s, row_bytes, &s);
}

// the checks hpe_draw and hpe_draw_nv12 share; *tiles receives the grid
static int draw_check(const char* fn, int64_t n_frames, int32_t h, int32_t w, int nv12, int32_t P, int32_t n_colours,
                      int* tiles_x, int* tiles_y) {
  if (n_frames < 0 || P < 0)
    return hpe_fail(HPE_EINVAL, "%s: negative frame count %lld or P %d", fn, (long long)n_frames, P);
  if (h < 1 || h > HPE_DRAW_MAX_DIM || w < 1 || w > HPE_DRAW_MAX_DIM)
    return hpe_fail(HPE_EINVAL, "%s: frame size %d x %d outside 1 .. HPE_DRAW_MAX_DIM = %d", fn, w, h,
                    HPE_DRAW_MAX_DIM);
  if (nv12 && ((h | w) & 1)) return hpe_fail(HPE_EINVAL, "%s: NV12 frame size %d x %d must be even", fn, w, h);
  if (n_colours < 1 || n_colours > 256)
    return hpe_fail(HPE_EINVAL, "%s: n_colours %d outside 1 .. 256", fn, n_colours);
  *tiles_x = (w + DRAW_TW - 1) / DRAW_TW;
  *tiles_y = (h + DRAW_TH - 1) / DRAW_TH;
  int64_t words;
  if (n_frames > 0x7fffffff || n_frames * *tiles_x * *tiles_y > 0x7fffffff ||
      __builtin_mul_overflow(n_frames * HPE_DRAW_PRIM_WORDS, (int64_t)P, &words))
    return hpe_fail(HPE_EINVAL, "%s: batch too large", fn);
  return HPE_OK;
}

extern "C" int hpe_draw(uint8_t* frames, int64_t n_frames, int32_t h, int32_t w, int64_t row_stride,
                        int64_t frame_stride, const int32_t* prims, const int32_t* n_prims, int32_t P,
                        const uint8_t* colours, int32_t n_colours, void* stream) {
  int tx, ty;
  if (int rc = draw_check("hpe_draw", n_frames, h, w, 0, P, n_colours, &tx, &ty)) return rc;
  if (row_stride < 3 * (int64_t)w)
    return hpe_fail(HPE_EINVAL, "hpe_draw: row stride %lld below 3 * w = %d", (long long)row_stride, 3 * w);
  if (frame_stride < 0) return hpe_fail(HPE_EINVAL, "hpe_draw: negative frame stride");
  if (n_frames > 0 && !draw_extent_ok(n_frames, frame_stride, h, row_stride, 3 * (int64_t)w))
    return hpe_fail(HPE_EINVAL, "hpe_draw: strides overflow");
  if (n_frames == 0 || P == 0) return HPE_OK;
  if (!frames || !prims || !n_prims || !colours) return hpe_fail(HPE_EINVAL, "hpe_draw: null argument");
  const DrawArgs a = {frames, nullptr, row_stride, frame_stride, 0, 0, h, w, tx, ty, prims, n_prims, P, colours,
                      n_colours};
  hipLaunchKernelGGL(draw_kernel<false>, dim3((unsigned)(n_frames * tx * ty)), dim3(DRAW_T), 0, (hipStream_t)stream,
                     a);
  return hpe_launched("hpe_draw");
}

extern "C" int hpe_draw_nv12(uint8_t* y, uint8_t* uv, int64_t n_frames, int32_t h, int32_t w, int64_t y_row_stride,
                             int64_t y_frame_stride, int64_t uv_row_stride, int64_t uv_frame_stride,
                             const int32_t* prims, const int32_t* n_prims, int32_t P, const uint8_t* colours,
                             int32_t n_colours, void* stream) {
  int tx, ty;
  if (int rc = draw_check("hpe_draw_nv12", n_frames, h, w, 1, P, n_colours, &tx, &ty)) return rc;
  if (y_row_stride < w || uv_row_stride < w)
    return hpe_fail(HPE_EINVAL, "hpe_draw_nv12: row strides %lld, %lld below w = %d", (long long)y_row_stride,
                    (long long)uv_row_stride, w);
  if (y_frame_stride < 0 || uv_frame_stride < 0) return hpe_fail(HPE_EINVAL, "hpe_draw_nv12: negative frame stride");
  if (n_frames > 0 && (!draw_extent_ok(n_frames, y_frame_stride, h, y_row_stride, w) ||
                       !draw_extent_ok(n_frames, uv_frame_stride, h / 2, uv_row_stride, w)))
    return hpe_fail(HPE_EINVAL, "hpe_draw_nv12: strides overflow");
  if (n_frames == 0 || P == 0) return HPE_OK;
  if (!y || !uv || !prims || !n_prims || !colours) return hpe_fail(HPE_EINVAL, "hpe_draw_nv12: null argument");
  const DrawArgs a = {y, uv, y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride, h, w, tx, ty, prims,
                      n_prims, P, colours, n_colours};
  hipLaunchKernelGGL(draw_kernel<true>, dim3((unsigned)(n_frames * tx * ty)), dim3(DRAW_T), 0, (hipStream_t)stream,
                     a);
  return hpe_launched("hpe_draw_nv12");
}

extern "C" int hpe_pose_prims(const int32_t* count, const double* boxes, const double* keypoints, const float* poses,
                              int64_t n_images, int32_t max_faces, int32_t src_x0, int32_t src_y0, int32_t src_w,
                              int32_t src_h, int32_t box_th, int32_t kp_radius, int32_t axis_th_x, int32_t axis_th_y,
                              int32_t axis_th_z, int32_t* prims, int32_t* n_prims, void* stream) {
  if (n_images < 0) return hpe_fail(HPE_EINVAL, "hpe_pose_prims: negative image count");
  if (max_faces < 1) return hpe_fail(HPE_EINVAL, "hpe_pose_prims: max_faces %d must be positive", max_faces);
  if (!roi_rect_ok(src_x0, src_y0, src_w, src_h))
    return hpe_fail(HPE_EINVAL, "hpe_pose_prims: source rectangle (%d, %d, %d, %d) outside 1 .. 2^24 / +-2^24", src_x0,
                    src_y0, src_w, src_h);
  if (box_th < 0 || box_th > HPE_DRAW_MAX_SIZE || axis_th_x < 0 || axis_th_x > HPE_DRAW_MAX_SIZE || axis_th_y < 0 ||
      axis_th_y > HPE_DRAW_MAX_SIZE || axis_th_z < 0 || axis_th_z > HPE_DRAW_MAX_SIZE)
    return hpe_fail(HPE_EINVAL, "hpe_pose_prims: thickness (%d; %d, %d, %d) outside 0 .. HPE_DRAW_MAX_SIZE = %d",
                    box_th, axis_th_x, axis_th_y, axis_th_z, HPE_DRAW_MAX_SIZE);
  if (kp_radius < -1 || kp_radius > HPE_DRAW_MAX_SIZE)
    return hpe_fail(HPE_EINVAL, "hpe_pose_prims: kp_radius %d outside -1 .. HPE_DRAW_MAX_SIZE = %d", kp_radius,
                    HPE_DRAW_MAX_SIZE);
  if (n_images > 0x7fffffff / HPE_DRAW_FACE_PRIMS / max_faces)
    return hpe_fail(HPE_EINVAL, "hpe_pose_prims: n_images * max_faces * %d beyond int32", HPE_DRAW_FACE_PRIMS);
  if (n_images == 0) return HPE_OK;
  if (!count || !boxes || !keypoints || !poses || !prims || !n_prims)
    return hpe_fail(HPE_EINVAL, "hpe_pose_prims: null argument");
  const int total = (int)(n_images * max_faces);
  const PosePrimArgs a = {count, boxes, keypoints, poses, total, max_faces, src_x0, src_y0, (double)src_w,
                          (double)src_h, box_th, kp_radius, {axis_th_x, axis_th_y, axis_th_z}, prims, n_prims};
  hipLaunchKernelGGL(pose_prims_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  return hpe_launched("hpe_pose_prims");
}
