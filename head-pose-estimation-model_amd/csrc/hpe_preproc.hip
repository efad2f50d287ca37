// hpe_preproc.hip — raw camera frames to the network input in one launch (SURVEY.md §8 f2's first
// step; prepareInputForInference, blazeFaceDetectorH5.py:247-269): BGR -> RGB, / 255, bicubic resize
// of the crop rectangle to out_h x out_w, (x - 0.5) / 0.5.
//
// The resize is TF 2.x ResizeBicubic with half_pixel_centers (what tf.image.resize(method='bicubic')
// runs without antialias), restated bit for bit by tests/bicubic_ref.py:
//   loc_f = (o + 0.5) * scale - 0.5, loc = floor(loc_f), off = rint((loc_f - loc) * 1024)
//   weights of taps loc-1 .. loc+2: Keys cubic (A = -0.5) at off / 1024 and (1024 - off) / 1024 (the
//   values of TF's 1025 x 2 coefficient table, evaluated in place), taps clamped to the crop, a
//   clamped tap's weight 0, the rest divided by their sum; y pass over the four tap columns, then x.
// Every fp32 operation is rounded on its own: the file is compiled with contraction off (the weights,
// the filter passes, the NV12 conversion and hpe_face_rois' float64 need it), so no multiply-add pair
// becomes an FMA (the only fused ops left are inside the division expansions).
// One thread per output pixel (three channels), lanes along x; a gather bounded by load latency.
// One kernel template, preprocess_kernel<Src, ROIS>, with two compile-time axes and four instantiations:
//   ROIS: where an output's rectangle comes from.  false: one crop for the batch, its scale computed
//     on the host.  true: one row of a device table of regions of interest per output, which may reach
//     outside the frame; this adds the row's validity test with its pad-constant exit, the per-row
//     scale and the in-frame tests of the window and of each tap.
//   Src: where the bytes come from.  BgrSrc: packed 3-byte pixels in either channel order.  Nv12Src:
//     decoded NV12 video frames, each tap converted to B, G, R bytes in the gather.  A source gives
//     frame i, the interior 4 x 4 window, and the taps one by one under an in-frame mask: Nv12Src for
//     the window as a whole (its tap rows share chroma loads), BgrSrc row by row, from one small
//     gather per form in the kernel's body (see by_row there for why).
// The body names no pixel format and exists once; the four C entry points (hpe_preprocess,
// hpe_preprocess_rois, hpe_preprocess_nv12, hpe_preprocess_rois_nv12) check their arguments, fill a
// source and a geometry struct and share one launch helper.  Last: the table of a second detector pass
// (hpe_face_rois).
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpe.h"
#include "hpe_boxes.h"
#include "hpe_common.h"

#pragma clang fp contract(off)

#define PRE_T 256

typedef uint32_t u32u __attribute__((aligned(1)));   // a dword at any byte address

// the outputs and their rectangles.  A specialization reads the fields of its own ROIS value only; each
// form's fields lie together, so that they arrive in a few wide scalar loads at the kernel's start.
struct Geom {
  float* out;
  const int32_t* rois;     // ROIS true: output r is row r of this (m, 5) table: frame, x0, y0, w, h
  int out_w, out_h;
  int total;               // outputs * out_h * out_w
  int n_frames, in_w, in_h;
  int pad[3];              // pad bytes in the source's channel order
  int x0, y0, w, h;        // ROIS false: one crop for the batch
  float sx, sy;            // (float)w / (float)out_w, (float)h / (float)out_h
};

// TF's coefficient table entries [i * 2] and [i * 2 + 1] at t = i / 1024 (exact in fp32)
__device__ __forceinline__ float keys_near(float t) {
  const float A = -0.5f;
  return ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
}
__device__ __forceinline__ float keys_far(float t) {
  const float A = -0.5f;
  const float u = t + 1.0f;
  return ((A * u - 5.0f * A) * u + 8.0f * A) * u - 4.0f * A;
}

// weights and clamped indices of output index o's four taps along one axis of `limit` source pixels
__device__ __forceinline__ void taps(int o, float scale, int limit, int* idx, float* w) {
  const float loc_f = ((float)o + 0.5f) * scale - 0.5f;
  const float fl = floorf(loc_f);
  const float d = loc_f - fl;
  const int off = (int)rintf(d * 1024.0f);
  const int loc = (int)fl;
  const float t0 = (float)off * (1.0f / 1024.0f), t1 = (float)(1024 - off) * (1.0f / 1024.0f);
  w[0] = keys_far(t0);
  w[1] = keys_near(t0);
  w[2] = keys_near(t1);
  w[3] = keys_far(t1);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = loc - 1 + k;
    const int c = min(max(i, 0), limit - 1);
    if (c != i) w[k] = 0.0f;
    idx[k] = c;
  }
  const float s = ((w[0] + w[1]) + w[2]) + w[3];
  if (fabsf(s) >= 1000.0f * FLT_MIN) {
    const float inv = 1.0f / s;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = w[k] * inv;
  }
}

// ---- what the kernel is made of, apart from the gather -------------------------------------------
// byte -> (float)(byte / 255.0), the reference's float64 division
__device__ __forceinline__ void fill_lut(float* lut) {
  lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
  __syncthreads();
}

// this thread's output pixel pix = (img * out_h + oy) * out_w + ox; false past the last one
struct Px {
  int pix, ox, oy;
  int64_t img;
};
__device__ __forceinline__ bool decode_px(int total, int out_w, int out_h, Px* p) {
  const int64_t gid = (int64_t)blockIdx.x * PRE_T + threadIdx.x;
  if (gid >= total) return false;
  const int pix = (int)gid, row = pix / out_w;
  *p = {pix, pix % out_w, row % out_h, row / out_h};
  return true;
}

// the four taps of one row where they are 12 contiguous bytes: three dword loads at any byte address
__device__ __forceinline__ void load12(const uint8_t* p, uint8_t* b) {
  const u32u* q = (const u32u*)p;
  const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    b[e] = (uint8_t)(q0 >> (8 * e));
    b[4 + e] = (uint8_t)(q1 >> (8 * e));
    b[8 + e] = (uint8_t)(q2 >> (8 * e));
  }
}

// one tap: a pixel's three bytes
__device__ __forceinline__ void load3(const uint8_t* p, uint8_t* b) {
  b[0] = p[0];
  b[1] = p[1];
  b[2] = p[2];
}

// o: the three values in the frame's channel order
__device__ __forceinline__ void store_px(float* dst, const float* o, int bgr) {
  dst[0] = bgr ? o[2] : o[0];
  dst[1] = o[1];
  dst[2] = bgr ? o[0] : o[2];
}

// b[j][3 * k + ch]: the byte of tap row j, tap column k.  y pass: c[k][ch] = ((v0 wy0 + v1 wy1) + v2 wy2)
// + v3 wy3 for tap column k; then the x pass over the four columns, (r - 0.5) / 0.5 and the store
__device__ __forceinline__ void filter_store(const float* lut, const uint8_t (*b)[12], const float* wy,
                                             const float* wx, int bgr, float* dst) {
  float c[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    c[e] = lut[b[0][e]] * wy[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) c[e] = c[e] + lut[b[j][e]] * wy[j];
  }
  float o[3];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const float r = ((c[ch] * wx[0] + c[3 + ch] * wx[1]) + c[6 + ch] * wx[2]) + c[9 + ch] * wx[3];
    o[ch] = (r - 0.5f) / 0.5f;
  }
  store_px(dst, o, bgr);
}

// ---- packed BGR (or RGB) frames ------------------------------------------------------------------
struct BgrSrc {
  const uint8_t* frames;
  int64_t frame_stride, row_stride;   // bytes
  int bgr;

  // The tap rows are independent, so this source gathers row by row, from loops that stand in the
  // kernel's body.  With the same loops inside window() / tap_by_tap() members as Nv12Src has them,
  // the compiler keeps the 48 window bytes packed four to a register and packs and unpacks them around
  // every tap: 1,380 instead of 985 instructions in the ROI form, and 10 to 16 % more time on MI355X.
  static constexpr bool by_row = true;
  // hpe_preprocess folds the crop's origin into `frames`, which saves the crop form a register; an
  // NV12 tap's chroma pair depends on its frame coordinates' parity, so Nv12Src cannot do the same
  static constexpr bool origin_in_frame = true;

  __device__ __forceinline__ int order() const { return bgr; }
  __device__ __forceinline__ const uint8_t* frame(int64_t i) const { return frames + i * frame_stride; }
  __device__ __forceinline__ const uint8_t* row(const uint8_t* f, int y) const { return f + (int64_t)y * row_stride; }
  // columns x0 .. x0 + 3 of a row, all inside the frame: 12 contiguous bytes
  __device__ __forceinline__ void row_window(const uint8_t* r, int x0, uint8_t* b) const { load12(r + x0 * 3, b); }
  __device__ __forceinline__ void tap(const uint8_t* r, int x, uint8_t* b) const { load3(r + x * 3, b); }
};

// ---- NV12 frames ------------------------------------------------------------------------------------
// Nv12Src (hpe_preprocess_nv12 / hpe_preprocess_rois_nv12): a gather that reads a luma plane and a
// half-resolution plane of interleaved (U, V) pairs and fills b[][] with the B, G, R bytes it converts
// per tap (include/hpe.h states the rule; tests/nv12_ref.py restates it), so the output equals
// BgrSrc's on the converted frame, bit for bit.  The chroma of pixel (y, x) is the
// pair (y >> 1, x >> 1): a 4 x 4 window touches at most 3 chroma rows x 3 pairs.  The interior path
// loads one dword of luma per tap row and each distinct pair once, all before the first conversion,
// and computes a pair's three chroma terms once; no load touches a byte past in_w in a row.
typedef uint16_t u16u __attribute__((aligned(1)));   // a (U, V) pair at any byte address

#define NV12_SHIFT 20
#define NV12_HALF (1 << (NV12_SHIFT - 1))

struct Nv12Coef {
  int cy, cvr, cvg, cug, cub;
};
__device__ __forceinline__ Nv12Coef nv12_coef(int matrix) {
  if (matrix == 1) return {1220945, 1879825, -558796, -223607, 2215014};   // BT.709
  return {1220542, 1673527, -852492, -409993, 2116026};                    // BT.601
}

struct Nv12Frame {   // one frame's two planes
  const uint8_t *y, *uv;
  int64_t y_row, uv_row;   // bytes
};

// what a (U, V) pair adds to the luma term of R, G and B, the rounding half included
struct Chroma {
  int r, g, b;
};
__device__ __forceinline__ Chroma chroma_terms(const Nv12Coef& k, int u, int v) {
  u -= 128;
  v -= 128;
  return {k.cvr * v + NV12_HALF, k.cvg * v + k.cug * u + NV12_HALF, k.cub * u + NV12_HALF};
}
__device__ __forceinline__ Chroma pick(bool second, const Chroma& a, const Chroma& b) {
  return {second ? b.r : a.r, second ? b.g : a.g, second ? b.b : a.b};
}
__device__ __forceinline__ uint8_t sat8(int v) { return (uint8_t)min(max(v, 0), 255); }

// one pixel -> its three bytes in B, G, R order
__device__ __forceinline__ void nv12_px(const Nv12Coef& k, int y, const Chroma& c, uint8_t* bgr) {
  const int yy = max(y - 16, 0) * k.cy;
  bgr[0] = sat8((yy + c.b) >> NV12_SHIFT);
  bgr[1] = sat8((yy + c.g) >> NV12_SHIFT);
  bgr[2] = sat8((yy + c.r) >> NV12_SHIFT);
}

// the window of tap rows fy[0..3] (ascending, steps of 0 or 1) and columns fx0 .. fx0 + 3, all inside
// the frame.  Chroma rows: fy[0] >> 1 <= fy[1] >> 1, fy[2] >> 1 <= (fy[0] >> 1) + 1 and fy[3] >> 1, so
// the three rows loaded are the first, the first + 1 (capped at the last) and the last.  Chroma pairs:
// columns fx0 >> 1 and (fx0 >> 1) + 1 as one dword and (fx0 + 3) >> 1, the third pair for odd fx0
// and the second again for even; the dword ends at byte 2 * (fx0 >> 1) + 3 <= in_w - 1.
__device__ __forceinline__ void nv12_window(const Nv12Frame& f, const Nv12Coef& k, const int* fy, int fx0,
                                            uint8_t (*b)[12]) {
  const int cy0 = fy[0] >> 1, cy3 = fy[3] >> 1;
  const int cr[3] = {cy0, min(cy0 + 1, cy3), cy3};
  const int cx0 = fx0 >> 1, cx3 = (fx0 + 3) >> 1;
  uint32_t yq[4], q01[3];
  uint16_t q3[3];
#pragma unroll
  for (int j = 0; j < 4; ++j) yq[j] = *(const u32u*)(f.y + (int64_t)fy[j] * f.y_row + fx0);
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const uint8_t* r = f.uv + (int64_t)cr[s] * f.uv_row;
    q01[s] = *(const u32u*)(r + 2 * cx0);
    q3[s] = *(const u16u*)(r + 2 * cx3);
  }
  // c[s][kx]: chroma row slot s, tap column kx
  const bool odd = fx0 & 1;
  Chroma c[3][4];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    c[s][0] = chroma_terms(k, q01[s] & 255, (q01[s] >> 8) & 255);
    c[s][2] = chroma_terms(k, (q01[s] >> 16) & 255, q01[s] >> 24);
    c[s][3] = chroma_terms(k, q3[s] & 255, q3[s] >> 8);
    c[s][1] = pick(odd, c[s][0], c[s][2]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bool up = (fy[j] >> 1) != cy0;   // rows 1 and 2: the first chroma row or the one after it
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      const Chroma t = j == 0 ? c[0][kx] : j == 3 ? c[2][kx] : pick(up, c[0][kx], c[1][kx]);
      nv12_px(k, (yq[j] >> (8 * kx)) & 255, t, b[j] + 3 * kx);
    }
  }
}

// the taps one by one (an x tap clamped, or part of the window outside the frame): in[j][kx] says
// which taps lie in the frame; the others take the pad bytes as they are.  All loads first.
__device__ __forceinline__ void nv12_taps(const Nv12Frame& f, const Nv12Coef& k, const int* fy, const int* fx,
                                          const bool (*in)[4], const uint8_t* pad, uint8_t (*b)[12]) {
  uint8_t yv[4][4], uu[4][4], vv[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      yv[j][kx] = uu[j][kx] = vv[j][kx] = 0;
      if (in[j][kx]) {
        const uint8_t* c = f.uv + (int64_t)(fy[j] >> 1) * f.uv_row + 2 * (fx[kx] >> 1);
        yv[j][kx] = f.y[(int64_t)fy[j] * f.y_row + fx[kx]];
        uu[j][kx] = c[0];
        vv[j][kx] = c[1];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int kx = 0; kx < 4; ++kx) {
      if (in[j][kx])
        nv12_px(k, yv[j][kx], chroma_terms(k, uu[j][kx], vv[j][kx]), b[j] + 3 * kx);
      else
        load3(pad, b[j] + 3 * kx);
    }
  }
}

struct Nv12Src {
  const uint8_t *y, *uv;
  int64_t y_frame, y_row, uv_frame, uv_row;   // bytes
  int matrix;

  static constexpr bool by_row = false;            // the tap rows share their chroma loads
  static constexpr bool origin_in_frame = false;

  __device__ __forceinline__ int order() const { return 1; }   // the conversion makes B, G, R
  __device__ __forceinline__ Nv12Frame frame(int64_t i) const {
    return {y + i * y_frame, uv + i * uv_frame, y_row, uv_row};
  }
  __device__ __forceinline__ void window(const Nv12Frame& f, const int* fy, int fx0, uint8_t (*b)[12]) const {
    nv12_window(f, nv12_coef(matrix), fy, fx0, b);
  }
  __device__ __forceinline__ void tap_by_tap(const Nv12Frame& f, const int* fy, const int* fx, const bool (*in)[4],
                                             const uint8_t* pad, uint8_t (*b)[12]) const {
    nv12_taps(f, nv12_coef(matrix), fy, fx, in, pad, b);
  }
};

// ---- the kernel ------------------------------------------------------------------------------------
// ROIS false: output i is the crop (x0, y0, w, h) of frame i.  ROIS true: output r is the same
// preparation of a whole h x w canvas whose pixel (y, x) is the frame's pixel (y0 + y, x0 + x) where that
// lies inside the frame and the pad bytes elsewhere, for row r = (frame, x0, y0, w, h) of the table.  The
// taps clamp to the rectangle, not to the frame, so an ROI inside the frame equals the crop form with
// that crop and an ROI reaching outside equals the crop form on a host-padded copy, bit for bit.  A
// row's rectangle must pass roi_rect_ok (hpe_boxes.h): every coordinate sum below then fits int32.
template <class Src, bool ROIS>
__global__ void __launch_bounds__(PRE_T) preprocess_kernel(Src src, Geom g) {
  __shared__ float lut[256];
  fill_lut(lut);
  Px p;   // p.img: the frame, or the ROI row
  if (!decode_px(g.total, g.out_w, g.out_h, &p)) return;
  float* dst = g.out + (int64_t)p.pix * 3;

  int64_t fr = p.img;
  int x0 = g.x0, y0 = g.y0, cw = g.w, ch = g.h;
  float sx = g.sx, sy = g.sy;
  uint8_t pad[3] = {0, 0, 0};
  int in_w = 0, in_h = 0;   // the frame's size, read here with the rest of the ROI form's fields
  if constexpr (ROIS) {
    in_w = g.in_w, in_h = g.in_h;
    const int32_t* roi = g.rois + p.img * 5;
    fr = roi[0], x0 = roi[1], y0 = roi[2], cw = roi[3], ch = roi[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) pad[c] = (uint8_t)g.pad[c];
    if (!(fr >= 0 && fr < g.n_frames && roi_rect_ok(x0, y0, cw, ch))) {   // invalid: reads no frame memory
      float o[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (lut[pad[c]] - 0.5f) / 0.5f;
      store_px(dst, o, src.order());
      return;
    }
    sx = (float)cw / (float)g.out_w;
    sy = (float)ch / (float)g.out_h;
  }

  int yi[4], xi[4];
  float wy[4], wx[4];
  taps(p.oy, sy, ch, yi, wy);
  taps(p.ox, sx, cw, xi, wx);
  // frame coordinates of the taps (ascending along each axis, as the clamped indices are); a crop whose
  // origin the host folded into the frame pointer counts from that origin
  if constexpr (!ROIS && Src::origin_in_frame) x0 = y0 = 0;
  int fy[4], fx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    fy[k] = y0 + yi[k];
    fx[k] = x0 + xi[k];
  }
  // no x tap clamped and, for an ROI, the whole 4 x 4 window inside the frame
  bool interior = xi[3] - xi[0] == 3;
  if constexpr (ROIS) interior = interior && fx[0] >= 0 && fx[3] < in_w && fy[0] >= 0 && fy[3] < in_h;

  const auto f = src.frame(fr);
  uint8_t b[4][12];
  if constexpr (Src::by_row && !ROIS) {
    // a crop lies inside its frame; the branch stands in the row loop (66 VGPRs; around it, 74 and a
    // wave per SIMD less)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const auto r = src.row(f, fy[j]);
      if (interior) {
        src.row_window(r, fx[0], b[j]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) src.tap(r, fx[k], b[j] + 3 * k);
      }
    }
  } else if constexpr (Src::by_row) {
    // an ROI: the branch stands around the row loop, so that the four rows' loads go out together (in
    // it, 8 % slower on MI355X); a tap outside the frame takes the pad bytes
    if (interior) {
#pragma unroll
      for (int j = 0; j < 4; ++j) src.row_window(src.row(f, fy[j]), fx[0], b[j]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool row_in = fy[j] >= 0 && fy[j] < in_h;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (row_in && fx[k] >= 0 && fx[k] < in_w)
            src.tap(src.row(f, fy[j]), fx[k], b[j] + 3 * k);
          else
            load3(pad, b[j] + 3 * k);
        }
      }
    }
  } else if (interior) {
    src.window(f, fy, fx[0], b);
  } else {
    bool in[4][4];   // which taps lie in the frame; a crop lies inside it: all true at compile time
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool row_in = !ROIS || (fy[j] >= 0 && fy[j] < in_h);
#pragma unroll
      for (int k = 0; k < 4; ++k) in[j][k] = row_in && (!ROIS || (fx[k] >= 0 && fx[k] < in_w));
    }
    src.tap_by_tap(f, fy, fx, in, pad, b);
  }
  filter_store(lut, b, wy, wx, src.order(), dst);
}

// ---- the C entry points ------------------------------------------------------------------------------
// what the four check alike, in the order their callers see.  crop: the crop forms' (x0, y0, w, h),
// null for the ROI forms
static int check_rect(const char* fn, int32_t in_h, int32_t in_w, const int32_t* crop, int32_t out_h,
                      int32_t out_w) {
  if (in_h <= 0 || in_w <= 0 || out_h <= 0 || out_w <= 0)
    return hpe_fail(HPE_EINVAL, "%s: sizes must be positive (frame %d x %d, out %d x %d)", fn, in_h, in_w, out_h,
                    out_w);
  if (!crop) return HPE_OK;
  if (crop[2] <= 0 || crop[3] <= 0)
    return hpe_fail(HPE_EINVAL, "%s: crop sizes must be positive (%d x %d)", fn, crop[3], crop[2]);
  if (crop[0] < 0 || crop[1] < 0 || (int64_t)crop[0] + crop[2] > in_w || (int64_t)crop[1] + crop[3] > in_h)
    return hpe_fail(HPE_EINVAL, "%s: crop (%d, %d, %d, %d) outside the %d x %d frame", fn, crop[0], crop[1], crop[2],
                    crop[3], in_w, in_h);
  return HPE_OK;
}

// the ROI forms: the frame count must fit the kernel's int, the pad bytes a byte
static int check_table(const char* fn, int64_t n_frames, int32_t pad0, int32_t pad1, int32_t pad2) {
  if (n_frames > 0x7fffffff) return hpe_fail(HPE_EINVAL, "%s: batch too large", fn);
  if (pad0 < 0 || pad0 > 255 || pad1 < 0 || pad1 > 255 || pad2 < 0 || pad2 > 255)
    return hpe_fail(HPE_EINVAL, "%s: pad bytes (%d, %d, %d) outside 0..255", fn, pad0, pad1, pad2);
  return HPE_OK;
}

// count (`what`: its name in the message) outputs of out_h x out_w pixels must fit the kernel's int index
static int check_count(const char* fn, const char* what, int64_t count, int32_t out_h, int32_t out_w) {
  if (count > 0 && count > (int64_t)0x7fffffff / ((int64_t)out_h * out_w))
    return hpe_fail(HPE_EINVAL, "%s: %s * out_h * out_w exceeds INT32_MAX", fn, what);
  return HPE_OK;
}

// a packed source: one row stride in bytes, the frames back to back
static int check_bgr(const char* fn, int64_t n, int32_t in_h, int32_t in_w, int64_t row_stride_bytes) {
  if (in_w > 0x7fffffff / 3) return hpe_fail(HPE_EINVAL, "%s: frame width %d too large", fn, in_w);
  if (row_stride_bytes < 3 * (int64_t)in_w)
    return hpe_fail(HPE_EINVAL, "%s: row stride %lld below 3 * in_w = %lld", fn, (long long)row_stride_bytes,
                    3 * (long long)in_w);
  if (row_stride_bytes > INT64_MAX / in_h || (n > 0 && row_stride_bytes * in_h > INT64_MAX / n))
    return hpe_fail(HPE_EINVAL, "%s: batch too large", fn);
  return HPE_OK;
}

// an NV12 source: two planes, each with a row and a frame stride in bytes
static int check_nv12(const char* fn, int64_t n, int32_t in_h, int32_t in_w, int64_t y_row, int64_t y_frame,
                      int64_t uv_row, int64_t uv_frame, int32_t matrix) {
  if ((in_h | in_w) & 1) return hpe_fail(HPE_EINVAL, "%s: an NV12 frame's size %d x %d must be even", fn, in_h, in_w);
  if (matrix != 0 && matrix != 1)
    return hpe_fail(HPE_EINVAL, "%s: matrix %d is neither 0 (BT.601) nor 1 (BT.709)", fn, matrix);
  if (y_row < in_w || uv_row < in_w)
    return hpe_fail(HPE_EINVAL, "%s: row strides (%lld, %lld) below in_w = %d", fn, (long long)y_row,
                    (long long)uv_row, in_w);
  if (y_frame < 0 || uv_frame < 0)
    return hpe_fail(HPE_EINVAL, "%s: negative frame stride (%lld, %lld)", fn, (long long)y_frame, (long long)uv_frame);
  // the last byte's offset, n * frame stride + in_h * row stride at most, must fit int64
  const int64_t rows = y_row > uv_row ? y_row : uv_row, frames = y_frame > uv_frame ? y_frame : uv_frame;
  if (rows > INT64_MAX / in_h || (n > 0 && frames > (INT64_MAX - rows * in_h) / n))
    return hpe_fail(HPE_EINVAL, "%s: batch too large", fn);
  return HPE_OK;
}

static Geom crop_geom(float* out, int64_t n, int32_t out_h, int32_t out_w, const int32_t* crop) {
  return {.out = out, .out_w = out_w, .out_h = out_h, .total = (int)(n * out_h * out_w),
          .x0 = crop[0], .y0 = crop[1], .w = crop[2], .h = crop[3],
          .sx = (float)crop[2] / (float)out_w, .sy = (float)crop[3] / (float)out_h};
}

static Geom rois_geom(float* out, int64_t m, int32_t out_h, int32_t out_w, const int32_t* rois, int64_t n_frames,
                      int32_t in_h, int32_t in_w, int32_t pad0, int32_t pad1, int32_t pad2) {
  return {.out = out, .rois = rois, .out_w = out_w, .out_h = out_h, .total = (int)(m * out_h * out_w),
          .n_frames = (int)n_frames, .in_w = in_w, .in_h = in_h, .pad = {pad0, pad1, pad2}};
}

template <class Src, bool ROIS>
static int launch(const char* fn, const Src& src, const Geom& g, void* stream) {
  const unsigned grid = (unsigned)(((int64_t)g.total + PRE_T - 1) / PRE_T);
  hipLaunchKernelGGL((preprocess_kernel<Src, ROIS>), dim3(grid), dim3(PRE_T), 0, (hipStream_t)stream, src, g);
  return hpe_launched(fn);
}

extern "C" int hpe_preprocess(const uint8_t* frames, int64_t n, int32_t in_h, int32_t in_w, int64_t row_stride_bytes,
                              int32_t crop_x0, int32_t crop_y0, int32_t crop_w, int32_t crop_h, int32_t bgr,
                              float* out, int32_t out_h, int32_t out_w, void* stream) {
  const char* fn = "hpe_preprocess";
  if (n < 0) return hpe_fail(HPE_EINVAL, "%s: negative frame count", fn);
  const int32_t crop[4] = {crop_x0, crop_y0, crop_w, crop_h};
  if (int rc = check_rect(fn, in_h, in_w, crop, out_h, out_w)) return rc;
  if (int rc = check_bgr(fn, n, in_h, in_w, row_stride_bytes)) return rc;
  if (int rc = check_count(fn, "n", n, out_h, out_w)) return rc;
  if (n == 0) return HPE_OK;
  if (!frames || !out) return hpe_fail(HPE_EINVAL, "%s: null argument", fn);
  const BgrSrc src = {.frames = frames + (int64_t)crop_y0 * row_stride_bytes + (int64_t)crop_x0 * 3,   // origin_in_frame
                      .frame_stride = (int64_t)in_h * row_stride_bytes,
                      .row_stride = row_stride_bytes, .bgr = bgr};
  return launch<BgrSrc, false>(fn, src, crop_geom(out, n, out_h, out_w, crop), stream);
}

extern "C" int hpe_preprocess_rois(const uint8_t* frames, int64_t n_frames, int32_t in_h, int32_t in_w,
                                   int64_t row_stride_bytes, const int32_t* rois, int64_t m, int32_t pad_b0,
                                   int32_t pad_b1, int32_t pad_b2, int32_t bgr, float* out, int32_t out_h,
                                   int32_t out_w, void* stream) {
  const char* fn = "hpe_preprocess_rois";
  if (n_frames < 0 || m < 0) return hpe_fail(HPE_EINVAL, "%s: negative frame or ROI count", fn);
  if (int rc = check_rect(fn, in_h, in_w, nullptr, out_h, out_w)) return rc;
  if (int rc = check_bgr(fn, n_frames, in_h, in_w, row_stride_bytes)) return rc;
  if (int rc = check_table(fn, n_frames, pad_b0, pad_b1, pad_b2)) return rc;
  if (int rc = check_count(fn, "m", m, out_h, out_w)) return rc;
  if (m == 0) return HPE_OK;
  // without frames every row is invalid and nothing is read through `frames`
  if ((!frames && n_frames > 0) || !rois || !out) return hpe_fail(HPE_EINVAL, "%s: null argument", fn);
  const BgrSrc src = {.frames = frames, .frame_stride = (int64_t)in_h * row_stride_bytes,
                      .row_stride = row_stride_bytes, .bgr = bgr};
  return launch<BgrSrc, true>(
      fn, src, rois_geom(out, m, out_h, out_w, rois, n_frames, in_h, in_w, pad_b0, pad_b1, pad_b2), stream);
}

extern "C" int hpe_preprocess_nv12(const uint8_t* y, const uint8_t* uv, int64_t n, int32_t in_h, int32_t in_w,
                                   int64_t y_row_stride, int64_t y_frame_stride, int64_t uv_row_stride,
                                   int64_t uv_frame_stride, int32_t matrix, int32_t crop_x0, int32_t crop_y0,
                                   int32_t crop_w, int32_t crop_h, float* out, int32_t out_h, int32_t out_w,
                                   void* stream) {
  const char* fn = "hpe_preprocess_nv12";
  if (n < 0) return hpe_fail(HPE_EINVAL, "%s: negative frame count", fn);
  const int32_t crop[4] = {crop_x0, crop_y0, crop_w, crop_h};
  if (int rc = check_rect(fn, in_h, in_w, crop, out_h, out_w)) return rc;
  if (int rc = check_nv12(fn, n, in_h, in_w, y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride, matrix))
    return rc;
  if (int rc = check_count(fn, "n", n, out_h, out_w)) return rc;
  if (n == 0) return HPE_OK;
  if (!y || !uv || !out) return hpe_fail(HPE_EINVAL, "%s: null argument", fn);
  const Nv12Src src = {.y = y, .uv = uv, .y_frame = y_frame_stride, .y_row = y_row_stride,
                       .uv_frame = uv_frame_stride, .uv_row = uv_row_stride, .matrix = matrix};
  return launch<Nv12Src, false>(fn, src, crop_geom(out, n, out_h, out_w, crop), stream);
}

extern "C" int hpe_preprocess_rois_nv12(const uint8_t* y, const uint8_t* uv, int64_t n_frames, int32_t in_h,
                                        int32_t in_w, int64_t y_row_stride, int64_t y_frame_stride,
                                        int64_t uv_row_stride, int64_t uv_frame_stride, const int32_t* rois,
                                        int64_t m, int32_t pad_b, int32_t pad_g, int32_t pad_r, int32_t matrix,
                                        float* out, int32_t out_h, int32_t out_w, void* stream) {
  const char* fn = "hpe_preprocess_rois_nv12";
  if (n_frames < 0 || m < 0) return hpe_fail(HPE_EINVAL, "%s: negative frame or ROI count", fn);
  if (int rc = check_rect(fn, in_h, in_w, nullptr, out_h, out_w)) return rc;
  if (int rc = check_nv12(fn, n_frames, in_h, in_w, y_row_stride, y_frame_stride, uv_row_stride, uv_frame_stride,
                          matrix))
    return rc;
  if (int rc = check_table(fn, n_frames, pad_b, pad_g, pad_r)) return rc;
  if (int rc = check_count(fn, "m", m, out_h, out_w)) return rc;
  if (m == 0) return HPE_OK;
  // without frames every row is invalid and nothing is read through `y` or `uv`
  if (((!y || !uv) && n_frames > 0) || !rois || !out) return hpe_fail(HPE_EINVAL, "%s: null argument", fn);
  const Nv12Src src = {.y = y, .uv = uv, .y_frame = y_frame_stride, .y_row = y_row_stride,
                       .uv_frame = uv_frame_stride, .uv_row = uv_row_stride, .matrix = matrix};
  return launch<Nv12Src, true>(
      fn, src, rois_geom(out, m, out_h, out_w, rois, n_frames, in_h, in_w, pad_b, pad_g, pad_r), stream);
}

// hpe_face_rois: hpe_detect's boxes -> the ROI table of a second pass.  One workgroup per frame: the
// row offset of frame i is the sum of count[0 .. i) (a block reduction, so the compaction is
// deterministic), and the slots past the total are filled with the invalid row.  float64, every
// operation rounded on its own (contraction is off in this file).
#define FROI_T 256

__device__ __forceinline__ int froi_count(const int32_t* count, int64_t i, int max_faces) {
  return min(max(count[i], 0), max_faces);
}

__global__ void __launch_bounds__(FROI_T) face_rois_kernel(const int32_t* count, const double* boxes, int n_images,
                                                            int max_faces, double sx0, double sy0, double sw,
                                                            double sh, double scale, int32_t* rois,
                                                            int32_t* n_rois) {
  __shared__ int red[2][FROI_T];
  const int img = blockIdx.x;
  const int t = threadIdx.x;
  int before = 0, all = 0;
  for (int i = t; i < n_images; i += FROI_T) {
    const int c = froi_count(count, i, max_faces);
    all += c;
    if (i < img) before += c;
  }
  red[0][t] = before;
  red[1][t] = all;
  __syncthreads();
  for (int s = FROI_T / 2; s > 0; s >>= 1) {
    if (t < s) {
      red[0][t] += red[0][t + s];
      red[1][t] += red[1][t + s];
    }
    __syncthreads();
  }
  const int64_t first = red[0][0], total = red[1][0];
  if (img == 0 && t == 0) *n_rois = (int32_t)total;
  const int c = froi_count(count, img, max_faces);
  for (int j = t; j < max_faces; j += FROI_T) {
    if (j < c) {
      const double* bo = boxes + ((int64_t)img * max_faces + j) * 4;
      const double px1 = sx0 + bo[0] * sw, py1 = sy0 + bo[1] * sh;
      const double px2 = sx0 + bo[2] * sw, py2 = sy0 + bo[3] * sh;
      const double cx = 0.5 * (px1 + px2), cy = 0.5 * (py1 + py2);
      const double side = scale * fmax(px2 - px1, py2 - py1);
      int32_t* o = rois + (first + j) * 5;
      if (isfinite(cx) && isfinite(cy) && isfinite(side)) {
        const double lim = (double)HPE_ROI_LIM;
        const double S = fmin(fmax(ceil(side), 1.0), lim);
        const double rx = fmin(fmax(floor(cx - 0.5 * S), -lim), lim);
        const double ry = fmin(fmax(floor(cy - 0.5 * S), -lim), lim);
        o[0] = img;
        o[1] = (int32_t)rx;
        o[2] = (int32_t)ry;
        o[3] = (int32_t)S;
        o[4] = (int32_t)S;
      } else {
        o[0] = -1;
        o[1] = o[2] = o[3] = o[4] = 0;
      }
    }
    // the tail: slots [total, n_images * max_faces), each written by the block that owns its index
    const int64_t slot = (int64_t)img * max_faces + j;
    if (slot >= total) {
      int32_t* o = rois + slot * 5;
      o[0] = -1;
      o[1] = o[2] = o[3] = o[4] = 0;
    }
  }
}

extern "C" int hpe_face_rois(const int32_t* count, const double* boxes, int64_t n_images, int32_t max_faces,
                             int32_t src_x0, int32_t src_y0, int32_t src_w, int32_t src_h, double scale,
                             int32_t* rois, int32_t* n_rois, void* stream) {
  if (n_images < 0) return hpe_fail(HPE_EINVAL, "hpe_face_rois: negative frame count");
  if (max_faces <= 0) return hpe_fail(HPE_EINVAL, "hpe_face_rois: max_faces must be positive");
  if (src_w <= 0 || src_h <= 0)
    return hpe_fail(HPE_EINVAL, "hpe_face_rois: source rectangle %d x %d must be positive", src_w, src_h);
  if (n_images > (int64_t)0x7fffffff / max_faces) return hpe_fail(HPE_EINVAL, "hpe_face_rois: batch too large");
  if (!n_rois || (n_images > 0 && (!count || !boxes || !rois)))
    return hpe_fail(HPE_EINVAL, "hpe_face_rois: null argument");
  if (n_images == 0) {
    const hipError_t e = hipMemsetAsync(n_rois, 0, sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return hpe_fail(HPE_ERUNTIME, "hpe_face_rois memset: %s", hipGetErrorString(e));
    return HPE_OK;
  }
  hipLaunchKernelGGL(face_rois_kernel, dim3((unsigned)n_images), dim3(FROI_T), 0, (hipStream_t)stream, count, boxes,
                     (int)n_images, (int)max_faces, (double)src_x0, (double)src_y0, (double)src_w, (double)src_h,
                     scale, rois, n_rois);
  return hpe_launched("hpe_face_rois");
}
