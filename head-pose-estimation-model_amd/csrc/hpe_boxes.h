// hpe_boxes.h — what the box kernels (hpe_detect, hpe_merge_rois, hpe_track) share, defined once: the
// ROI validity rule, tf.image.non_max_suppression's IoU, the sort key, the LDS sort and the greedy pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- ROI validity -------------------------------------------------------------------------------
// A rectangle (x0, y0, w, h) in frame pixels is usable iff 1 <= w, h <= 2^24 and |x0|, |y0| <= 2^24:
// every coordinate sum formed from it fits int32 and every value converts to fp32 / fp64 exactly.
// Table rows (hpe_preprocess_rois, hpe_merge_rois) add their own frame-index condition.
#define HPE_ROI_LIM (1 << 24)

__host__ __device__ __forceinline__ bool roi_rect_ok(int32_t x0, int32_t y0, int32_t w, int32_t h) {
  return w >= 1 && w <= HPE_ROI_LIM && h >= 1 && h <= HPE_ROI_LIM && x0 >= -HPE_ROI_LIM && x0 <= HPE_ROI_LIM &&
         y0 >= -HPE_ROI_LIM && y0 <= HPE_ROI_LIM;
}

// ---- IoU ----------------------------------------------------------------------------------------
// TensorFlow's NonMaxSuppressionV3 IoU, as oracle.detector_ref._iou has it: fp32 on fp32 boxes,
// corner order agnostic, a zero (or NaN) area gives 0, and every operation rounds on its own:
// inter / ((area_i + area_j) - inter) with inter = h * w rounded to fp32 before it is subtracted.  A
// fused multiply-add in the denominator moves the IoU by one ulp for about 8 % of overlapping pairs and
// flips the decision for a pair whose IoU is the threshold.  So contraction is switched off inside the
// bodies and not left to the including file: the setting then travels with the operations when they
// are inlined, and the result's bits do not depend on what the caller's translation unit has in force.
// The side compared against many boxes is reduced once (box_prepare) and kept out of the inner loop.
struct BoxRef { float ymin, xmin, ymax, xmax, area; };

__device__ __forceinline__ BoxRef box_prepare(const float b[4]) {
#pragma clang fp contract(off)
  const float ymin = fminf(b[0], b[2]), xmin = fminf(b[1], b[3]);
  const float ymax = fmaxf(b[0], b[2]), xmax = fmaxf(b[1], b[3]);
  return {ymin, xmin, ymax, xmax, (ymax - ymin) * (xmax - xmin)};
}

__device__ __forceinline__ float box_iou(const BoxRef& a, const float b[4]) {
#pragma clang fp contract(off)
  const BoxRef r = box_prepare(b);
  if (!(a.area > 0.f && r.area > 0.f)) return 0.f;
  const float iy0 = fmaxf(a.ymin, r.ymin), ix0 = fmaxf(a.xmin, r.xmin);
  const float iy1 = fminf(a.ymax, r.ymax), ix1 = fminf(a.xmax, r.xmax);
  const float inter = fmaxf(iy1 - iy0, 0.f) * fmaxf(ix1 - ix0, 0.f);
  return inter / (a.area + r.area - inter);
}

__device__ __forceinline__ float box_iou(const float a[4], const float b[4]) { return box_iou(box_prepare(a), b); }

// ---- sort key -----------------------------------------------------------------------------------
// (score, index) -> 64 bits that order as "score descending, then index ascending" when sorted
// descending: the score's bits made monotonic on top, ~index below.  score + 0.0f: -0.0f orders as
// +0.0f, as a comparison of the scores has it; hpe_detect's scores are sigmoids and never -0.0f, so
// the addition changes none of their bits.  A NaN score has no place in the order: callers drop it.
// Every key is above 0, which pads a sort.
__device__ __forceinline__ uint32_t f2ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t box_key(float score, int index) {
  return ((uint64_t)f2ord(score + 0.0f) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)index);
}

__device__ __forceinline__ int key_index(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)key); }

__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// ---- bitonic sort -------------------------------------------------------------------------------
// key[0 .. p2) in LDS, descending, p2 a power of two, by a workgroup of nthreads threads of which this
// is thread t: one compare-exchange pair per thread step, a barrier after every stage.  The keys must
// be visible to the workgroup on entry (a barrier after the last write), and are on return.
__device__ __forceinline__ void bitonic_sort_desc(uint64_t* key, int p2, int t, int nthreads) {
  for (int k = 2; k <= p2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int q = t; q < (p2 >> 1); q += nthreads) {
        const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1));
        const int p = i | j;
        const uint64_t x = key[i], y = key[p];
        const bool desc = (i & k) == 0;
        if (desc ? (x < y) : (x > y)) {
          key[i] = y;
          key[p] = x;
        }
      }
      __syncthreads();
    }
  }
}

// ---- greedy NMS ---------------------------------------------------------------------------------
// tf.image.non_max_suppression over key[0 .. n), sorted descending: the first unsuppressed position is
// kept and suppresses every later one whose IoU with it is above thr, until n is exhausted or max_keep
// are kept.  fb[c] is the fp32 box of candidate c = key_index(key), sup[0 .. n) the suppression flags
// by sorted position, all zero on entry; key, fb and sup are in LDS and visible to the workgroup on
// entry.  Thread 0 calls keep(s, key) for the s-th kept box; the caller puts a barrier between those
// calls and a read of what they wrote.  Returns the number kept, uniform.  nthreads is a multiple of 64:
// every wave finds the next unsuppressed position by a ballot over 64 flags, the workgroup suppresses
// in parallel, one barrier per kept box.
template <typename Keep>
__device__ __forceinline__ int greedy_nms(const uint64_t* key, const float (*fb)[4], int* sup, int n, float thr,
                                          int max_keep, int t, int nthreads, Keep keep) {
  // i and ns are uniform: every thread reads the same flags between barriers
  const int lane = t & 63;
  int ns = 0;
  int i = 0;
  while (i < n && ns < max_keep) {
    // the first unsuppressed position >= i, 64 flags at a time.  Flags of positions above the one
    // found may already be changing (a wave ahead of this one suppressing against it); those below
    // it, and its own, are stable
    const int base = i & ~63;
    const int pos = base + lane;
    const unsigned long long m = __ballot(pos >= i && pos < n && !sup[pos]);
    if (!m) {
      i = base + 64;
      continue;
    }
    i = base + __ffsll(m) - 1;
    if (t == 0) keep(ns, key[i]);
    const BoxRef bi = box_prepare(fb[key_index(key[i])]);
    for (int j = i + 1 + t; j < n; j += nthreads) {
      if (sup[j]) continue;
      if (box_iou(bi, fb[key_index(key[j])]) > thr) sup[j] = 1;
    }
    ++ns;
    ++i;
    __syncthreads();
  }
  return ns;
}
