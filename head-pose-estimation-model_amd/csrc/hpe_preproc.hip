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
// Every fp32 operation is rounded on its own: the file is compiled with contraction off, so no
// multiply-add pair becomes an FMA (the only fused ops left are inside the division expansions).
// One thread per output pixel (three channels), lanes along x; a gather bounded by load latency.
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpe.h"
#include "hpe_common.h"

#pragma clang fp contract(off)

#define PRE_T 256

typedef uint32_t u32u __attribute__((aligned(1)));   // a dword at any byte address

struct PreArgs {
  const uint8_t* frames;   // + crop origin of frame 0
  float* out;
  int64_t frame_stride, row_stride;   // bytes
  int crop_w, crop_h, out_w, out_h;
  int total;               // n * out_h * out_w
  int bgr;
  float sx, sy;            // (float)crop_w / (float)out_w, (float)crop_h / (float)out_h
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

__global__ void __launch_bounds__(PRE_T) preprocess_kernel(PreArgs a) {
  __shared__ float lut[256];   // byte -> (float)(byte / 255.0), the reference's float64 division
  lut[threadIdx.x] = (float)((double)threadIdx.x / 255.0);
  __syncthreads();
  const int64_t gid = (int64_t)blockIdx.x * PRE_T + threadIdx.x;
  if (gid >= a.total) return;
  const int pix = (int)gid;
  const int ox = pix % a.out_w;
  const int row = pix / a.out_w;
  const int oy = row % a.out_h;
  const int64_t img = row / a.out_h;

  int yi[4], xi[4];
  float wy[4], wx[4];
  taps(oy, a.sy, a.crop_h, yi, wy);
  taps(ox, a.sx, a.crop_w, xi, wx);
  // no x tap clamped: the four taps of a row are 12 contiguous bytes
  const bool interior = xi[3] - xi[0] == 3;

  const uint8_t* base = a.frames + img * a.frame_stride;
  uint8_t b[4][12];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint8_t* r = base + (int64_t)yi[j] * a.row_stride;
    if (interior) {
      const u32u* q = (const u32u*)(r + xi[0] * 3);
      const uint32_t q0 = q[0], q1 = q[1], q2 = q[2];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        b[j][e] = (uint8_t)(q0 >> (8 * e));
        b[j][4 + e] = (uint8_t)(q1 >> (8 * e));
        b[j][8 + e] = (uint8_t)(q2 >> (8 * e));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint8_t* p = r + xi[k] * 3;
        b[j][3 * k] = p[0];
        b[j][3 * k + 1] = p[1];
        b[j][3 * k + 2] = p[2];
      }
    }
  }
  // y pass: c[k][ch] = ((v0 wy0 + v1 wy1) + v2 wy2) + v3 wy3 for tap column k
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
  float* dst = a.out + (int64_t)pix * 3;
  dst[0] = a.bgr ? o[2] : o[0];
  dst[1] = o[1];
  dst[2] = a.bgr ? o[0] : o[2];
}

extern "C" int hpe_preprocess(const uint8_t* frames, int64_t n, int32_t in_h, int32_t in_w, int64_t row_stride_bytes,
                              int32_t crop_x0, int32_t crop_y0, int32_t crop_w, int32_t crop_h, int32_t bgr,
                              float* out, int32_t out_h, int32_t out_w, void* stream) {
  if (n < 0) return hpe_fail(HPE_EINVAL, "hpe_preprocess: negative frame count");
  if (in_h <= 0 || in_w <= 0 || crop_w <= 0 || crop_h <= 0 || out_h <= 0 || out_w <= 0)
    return hpe_fail(HPE_EINVAL, "hpe_preprocess: sizes must be positive (frame %d x %d, crop %d x %d, out %d x %d)",
                    in_h, in_w, crop_h, crop_w, out_h, out_w);
  if (in_w > 0x7fffffff / 3) return hpe_fail(HPE_EINVAL, "hpe_preprocess: frame width %d too large", in_w);
  if (crop_x0 < 0 || crop_y0 < 0 || (int64_t)crop_x0 + crop_w > in_w || (int64_t)crop_y0 + crop_h > in_h)
    return hpe_fail(HPE_EINVAL, "hpe_preprocess: crop (%d, %d, %d, %d) outside the %d x %d frame", crop_x0, crop_y0,
                    crop_w, crop_h, in_w, in_h);
  if (row_stride_bytes < 3 * (int64_t)in_w)
    return hpe_fail(HPE_EINVAL, "hpe_preprocess: row stride %lld below 3 * in_w = %lld", (long long)row_stride_bytes,
                    3 * (long long)in_w);
  if (row_stride_bytes > INT64_MAX / in_h || (n > 0 && row_stride_bytes * in_h > INT64_MAX / n))
    return hpe_fail(HPE_EINVAL, "hpe_preprocess: batch too large");
  if (n > 0 && n > (int64_t)0x7fffffff / ((int64_t)out_h * out_w))
    return hpe_fail(HPE_EINVAL, "hpe_preprocess: n * out_h * out_w exceeds INT32_MAX");
  if (n == 0) return HPE_OK;
  if (!frames || !out) return hpe_fail(HPE_EINVAL, "hpe_preprocess: null argument");
  PreArgs a;
  a.frames = frames + (int64_t)crop_y0 * row_stride_bytes + (int64_t)crop_x0 * 3;
  a.out = out;
  a.frame_stride = (int64_t)in_h * row_stride_bytes;
  a.row_stride = row_stride_bytes;
  a.crop_w = crop_w;
  a.crop_h = crop_h;
  a.out_w = out_w;
  a.out_h = out_h;
  a.total = (int)(n * out_h * out_w);
  a.bgr = bgr;
  a.sx = (float)crop_w / (float)out_w;
  a.sy = (float)crop_h / (float)out_h;
  const unsigned grid = (unsigned)(((int64_t)a.total + PRE_T - 1) / PRE_T);
  hipLaunchKernelGGL(preprocess_kernel, dim3(grid), dim3(PRE_T), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hpe_fail(HPE_ERUNTIME, "hpe_preprocess launch: %s", hipGetErrorString(e));
  return HPE_OK;
}
