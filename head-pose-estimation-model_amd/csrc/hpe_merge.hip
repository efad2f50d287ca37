// hpe_merge.hip — tiled detection's last step: the per-ROI detections of a frame (hpe_detect on the
// images hpe_preprocess_rois made of the frame's table rows: the whole look and its tiles) brought
// back into the frame's coordinates and merged by one NMS, one workgroup per frame.
//   candidates  (r, j), r < R table rows of the frame, j < min(max(count[f*R + r], 0), M); a row must
//               pass hpe_preprocess_rois' validity rule and name frame f, else it contributes nothing
//   remap       float64, every operation rounded on its own (contraction is off in this file for
//               this: a fused o + v * s would round once):
//               X = ((rx + x * rw) - dst_x0) / dst_w, Y = ((ry + y * rh) - dst_y0) / dst_h
//               for the two box corners and the six keypoints
//   dropped     a candidate with a non-finite remapped box coordinate or a NaN score
//   order       score descending, then r * M + j ascending (64-bit keys: ordered score, ~index)
//   NMS         hpe_detect's (hpe_boxes.h: the same key, sort, greedy pass and IoU), on the fp32 casts
//               of the remapped boxes, at most max_faces_out kept
// Compaction, the bitonic sort in LDS over the power of two that holds the frame's candidates, then the
// greedy pass.  A latency kernel: the cost of tiled
// detection is the backbone over R images per frame, not this.
// LDS (dynamic): keys 8 B x pow2(R * M), fp32 boxes 16 B and a flag 4 B x R * M: 112 KB at
// HPE_MERGE_MAX_CAND.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpe.h"
#include "hpe_boxes.h"
#include "hpe_common.h"

#pragma clang fp contract(off)

#define MRG_T 256
#define MRG_KP 6

struct MergeArgs {
  const int32_t* rois;
  const int32_t* count;
  const float* scores;
  const double* boxes;
  const double* keypoints;
  const float* poses;
  int R, M, cap, sort_cap;   // cap = R * M, sort_cap = the power of two >= cap
  double dx0, dy0, dw, dh;
  float iou;
  int max_out;
  int32_t* count_out;
  int32_t* src_out;
  float* scores_out;
  double* boxes_out;
  double* keypoints_out;
  float* poses_out;
};

// one coordinate from ROI-normalised to destination-normalised: ((o + v * s) - d0) / d
__device__ __forceinline__ double mrg_map(double v, double o, double s, double d0, double d) {
  return ((o + v * s) - d0) / d;
}

__global__ void __launch_bounds__(MRG_T) merge_rois_kernel(MergeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mrg_lds[];
  uint64_t* key = (uint64_t*)mrg_lds;                  // [sort_cap]
  float(*fb)[4] = (float(*)[4])(key + a.sort_cap);     // [cap] fp32 boxes (NMS input), by candidate index
  int* sup = (int*)(fb + a.cap);                       // [cap] suppression flags, by sorted position
  __shared__ int ncand;
  const int64_t f = blockIdx.x;
  const int t = threadIdx.x;
  const int64_t row0 = f * a.R;
  if (t == 0) ncand = 0;
  __syncthreads();
  // ---- candidates: validity, remap of the box, compaction ----
  for (int c = t; c < a.cap; c += MRG_T) {
    const int r = c / a.M, j = c - r * a.M;
    if (j >= a.count[row0 + r]) continue;   // also a negative count; j < M bounds a count above M
    const int32_t* roi = a.rois + (row0 + r) * 5;
    if (roi[0] != f || !roi_rect_ok(roi[1], roi[2], roi[3], roi[4])) continue;   // not a valid row of this frame
    const int64_t s = (row0 + r) * a.M + j;
    const float sc = a.scores[s];
    const double* bo = a.boxes + s * 4;
    const double rx = (double)roi[1], ry = (double)roi[2], rw = (double)roi[3], rh = (double)roi[4];
    const double x1 = mrg_map(bo[0], rx, rw, a.dx0, a.dw), y1 = mrg_map(bo[1], ry, rh, a.dy0, a.dh);
    const double x2 = mrg_map(bo[2], rx, rw, a.dx0, a.dw), y2 = mrg_map(bo[3], ry, rh, a.dy0, a.dh);
    if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) || sc != sc) continue;
    const int slot = atomicAdd(&ncand, 1);
    key[slot] = box_key(sc, c);
    fb[c][0] = (float)x1;
    fb[c][1] = (float)y1;
    fb[c][2] = (float)x2;
    fb[c][3] = (float)y2;
  }
  __syncthreads();
  const int n = ncand;
  if (n == 0) {   // uniform
    if (t == 0) a.count_out[f] = 0;
    return;
  }
  int p2 = 1;
  while (p2 < n) p2 <<= 1;
  for (int i = n + t; i < p2; i += MRG_T) key[i] = 0;   // below every candidate's key
  for (int i = t; i < n; i += MRG_T) sup[i] = 0;
  __syncthreads();
  // ---- sort (score desc, then index asc) and greedy NMS ----
  bitonic_sort_desc(key, p2, t, MRG_T);
  const int64_t o0 = f * a.max_out;
  const int ns = greedy_nms(key, fb, sup, n, a.iou, a.max_out, t, MRG_T,
                            [&](int s, uint64_t k) { a.src_out[o0 + s] = key_index(k); });
  __syncthreads();   // src_out (thread 0's stores) is read by the workgroup below
  if (t == 0) a.count_out[f] = ns;
  // ---- the kept detections: score and pose copied, box corners and keypoints remapped in fp64 ----
  for (int s = t; s < ns; s += MRG_T) {
    const int c = a.src_out[o0 + s];
    const int64_t in = row0 * a.M + c;   // (row0 + r) * M + j
    a.scores_out[o0 + s] = a.scores[in];
    const float* pp = a.poses + in * 3;
    float* po = a.poses_out + (o0 + s) * 3;
    po[0] = pp[0];
    po[1] = pp[1];
    po[2] = pp[2];
  }
  for (int e = t; e < ns * (2 + MRG_KP); e += MRG_T) {   // one point per thread: 2 corners, 6 keypoints
    const int s = e / (2 + MRG_KP), p = e - s * (2 + MRG_KP);
    const int c = a.src_out[o0 + s];
    const int r = c / a.M;
    const int64_t in = row0 * a.M + c;
    const int32_t* roi = a.rois + (row0 + r) * 5;
    const double* src = p < 2 ? a.boxes + in * 4 + 2 * p : a.keypoints + in * (MRG_KP * 2) + 2 * (p - 2);
    double* dst = p < 2 ? a.boxes_out + (o0 + s) * 4 + 2 * p : a.keypoints_out + (o0 + s) * (MRG_KP * 2) + 2 * (p - 2);
    dst[0] = mrg_map(src[0], (double)roi[1], (double)roi[3], a.dx0, a.dw);
    dst[1] = mrg_map(src[1], (double)roi[2], (double)roi[4], a.dy0, a.dh);
  }
}

extern "C" int hpe_merge_rois(const int32_t* rois, int64_t n_frames, int32_t rows_per_frame, const int32_t* count,
                              const float* scores, const double* boxes, const double* keypoints,
                              const float* poses, int32_t max_faces_in, int32_t dst_x0, int32_t dst_y0,
                              int32_t dst_w, int32_t dst_h, float iou_threshold, int32_t max_faces_out,
                              int32_t* count_out, int32_t* src_out, float* scores_out, double* boxes_out,
                              double* keypoints_out, float* poses_out, void* stream) {
  if (n_frames < 0) return hpe_fail(HPE_EINVAL, "hpe_merge_rois: negative frame count");
  if (rows_per_frame <= 0 || max_faces_in <= 0 || max_faces_out <= 0)
    return hpe_fail(HPE_EINVAL, "hpe_merge_rois: rows_per_frame %d, max_faces_in %d and max_faces_out %d must be positive",
                    rows_per_frame, max_faces_in, max_faces_out);
  if (dst_w <= 0 || dst_h <= 0)
    return hpe_fail(HPE_EINVAL, "hpe_merge_rois: destination rectangle %d x %d must be positive", dst_w, dst_h);
  if (!roi_rect_ok(dst_x0, dst_y0, dst_w, dst_h))
    return hpe_fail(HPE_EINVAL, "hpe_merge_rois: destination rectangle (%d, %d, %d, %d) beyond 2^24", dst_x0, dst_y0,
                    dst_w, dst_h);
  if ((int64_t)rows_per_frame * max_faces_in > HPE_MERGE_MAX_CAND)
    return hpe_fail(HPE_EINVAL, "hpe_merge_rois: rows_per_frame * max_faces_in = %lld above HPE_MERGE_MAX_CAND = %d",
                    (long long)rows_per_frame * max_faces_in, HPE_MERGE_MAX_CAND);
  if (n_frames > 0x7fffffff) return hpe_fail(HPE_EINVAL, "hpe_merge_rois: batch too large");
  if (n_frames == 0) return HPE_OK;
  if (!rois || !count || !scores || !boxes || !keypoints || !poses || !count_out || !src_out || !scores_out ||
      !boxes_out || !keypoints_out || !poses_out)
    return hpe_fail(HPE_EINVAL, "hpe_merge_rois: null argument");
  const int cap = rows_per_frame * max_faces_in;
  int sort_cap = 1;
  while (sort_cap < cap) sort_cap <<= 1;
  const MergeArgs a = {rois, count, scores, boxes, keypoints, poses,
                       rows_per_frame, max_faces_in, cap, sort_cap,
                       (double)dst_x0, (double)dst_y0, (double)dst_w, (double)dst_h,
                       iou_threshold, max_faces_out,
                       count_out, src_out, scores_out, boxes_out, keypoints_out, poses_out};
  const int lds = sort_cap * 8 + cap * 20;
  if (hipFuncSetAttribute((const void*)merge_rois_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) !=
      hipSuccess)
    return hpe_fail(HPE_ERUNTIME, "hpe_merge_rois: LDS attribute");
  hipLaunchKernelGGL(merge_rois_kernel, dim3((unsigned)n_frames), dim3(MRG_T), lds, (hipStream_t)stream, a);
  return hpe_launched("hpe_merge_rois");
}
