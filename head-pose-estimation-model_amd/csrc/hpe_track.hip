// hpe_track.hip — faces tracked across the frames of a video and their box, keypoints and pose
// smoothed, on the device: what the reference's webcam loop does with 19 EMAFilters per face indexed
// by the face's position in the frame's result list (blazeFaceDetectorH5.py:16-35, :383-425), with an
// association step in front so that it also holds for several faces, drop-outs and order swaps.
//   input       S streams of T consecutive frames, stream-major (image g = s * T + t), M slots per image
//               as hpe_detect / hpe_merge_rois wrote them; c = min(max(count[g], 0), M) detections,
//               taken in slot order (the NMS order)
//   state       per stream K track slots: id (< 0: free), miss count, 19 smoothed doubles (box 4,
//               keypoints 12, pose 3) and the last matched raw box (4 doubles); next_id per stream
//   invalid     a detection with a non-finite box coordinate: id -1, outputs bit copies of the inputs
//   match       live tracks not yet matched in this frame; u = hpe_detect's IoU (hpe_boxes.h's box_iou)
//               of the fp32 casts of the detection's box and the track's last raw box; qualifies iff
//               u > match_iou; largest u, then lowest slot
//   update      state = alpha * m + (1.0 - alpha) * state in float64, each operation rounded on its own
//               (contraction is off in this file for this), 1.0 - alpha computed once: EMAFilter.update
//   spawn       nothing matched: lowest free slot, id = next_id, next_id = (next_id + 1) & 0x7fffffff,
//               state = m; no free slot: id -1, outputs bit copies of the inputs
//   frame end   every live unmatched track: miss += 1, freed (id = -1) iff miss > max_missed; a freed
//               slot keeps its doubles and its miss count until a spawn overwrites them
// One workgroup of one wave per stream.  Lane q owns track slot q: id, miss, the matched flag and the
// fp32 cast of the last raw box stay in its registers for the whole call.  Lane e < 23 owns value e of
// a detection (19 measurements, then the raw box again), so an update is one LDS read and one LDS
// write per lane with no cross-lane traffic.  The best track: every qualifying lane forms a 64-bit key,
// the IoU's bits on top (never negative, so they order as the float does) and 63 - q below; the
// maximum is taken over the ballot of the qualifying lanes with scalar lane reads, since that set is
// nearly always one lane or none.  The frame loop is a dependent chain; the next detection's values
// (the next slot of the frame, and slot 0 and the count of frame t + 1) are loaded while the current
// one is processed, as they do not depend on the state.  A latency kernel like hpe_merge_rois: many
// streams hide what one stream cannot.
// Nothing read from the state is used as an index.
// LDS (static): the stream's doubles, 8 B x 23 x HPE_TRACK_MAX_TRACKS = 11.5 KB, read once and written
// back once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hpe.h"
#include "hpe_boxes.h"
#include "hpe_common.h"

#pragma clang fp contract(off)

#define TRK_T 64
#define TRK_D HPE_TRACK_STATE_D
#define TRK_V 19   // smoothed values per track: box 4, keypoints 12, pose 3

struct TrackArgs {
  int T, M, K;
  const int32_t* count;
  const double* boxes;
  const double* keypoints;
  const float* poses;
  double alpha, om;   // om = 1.0 - alpha
  float iou;
  int max_missed;
  int32_t* state_i;
  double* state_d;
  int32_t* track_out;
  double* boxes_out;
  double* keypoints_out;
  float* poses_out;
};

struct TrkVal {
  double m;   // lanes 0..15 and 19..22: the value as read
  float p;    // lanes 16..18: the pose float as read
};

// value `lane` of detection (g, j): box, keypoints, pose, then the box again (lanes 19..22).  Two loads
// with no branch around them, so that they can stay in flight while the detection before is processed;
// the lanes that own no double (or no float) read the detection's first one and ignore it
__device__ __forceinline__ TrkVal trk_load(const TrackArgs& a, int64_t g, int j, int lane) {
  const int64_t d = g * a.M + j;
  const double* pb = a.boxes + d * 4;
  const double* pd = lane >= 4 && lane < 16 ? a.keypoints + d * 12 + (lane - 4)
                                            : pb + (lane < 4 ? lane : lane >= TRK_V && lane < TRK_D ? lane - TRK_V : 0);
  const float* pf = a.poses + d * 3 + (lane >= 16 && lane < TRK_V ? lane - 16 : 0);
  TrkVal v;
  v.m = *pd;
  v.p = *pf;
  return v;
}

// lane l's double, in every lane
__device__ __forceinline__ double trk_lane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ void __launch_bounds__(TRK_T) track_kernel(TrackArgs a) {
  __shared__ double sd[HPE_TRACK_MAX_TRACKS * TRK_D];
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  const int K = a.K, M = a.M;
  int32_t* si = a.state_i + s * (1 + 2 * K);
  double* sdg = a.state_d + s * K * TRK_D;
  for (int i = lane; i < K * TRK_D; i += TRK_T) sd[i] = sdg[i];
  int32_t next_id = si[0];
  const bool own = lane < K;
  int32_t id = own ? si[1 + lane] : -1;
  int32_t miss = own ? si[1 + K + lane] : 0;
  __syncthreads();
  float r0 = 0.f, r1 = 0.f, r2 = 0.f, r3 = 0.f;   // the slot's last raw box in fp32
  if (own) {
    r0 = (float)sd[lane * TRK_D + TRK_V];
    r1 = (float)sd[lane * TRK_D + TRK_V + 1];
    r2 = (float)sd[lane * TRK_D + TRK_V + 2];
    r3 = (float)sd[lane * TRK_D + TRK_V + 3];
  }
  const int64_t g0 = s * a.T;
  int32_t cnt = a.count[g0];
  TrkVal first = trk_load(a, g0, 0, lane);   // slot 0 exists (M >= 1), whatever the count
  for (int t = 0; t < a.T; ++t) {
    const int64_t g = g0 + t;
    const int c = min(max(cnt, 0), M);
    TrkVal cur = first;
    if (t + 1 < a.T) {   // frame t + 1's count and first detection, while this frame is processed
      cnt = a.count[g + 1];
      first = trk_load(a, g + 1, 0, lane);
    }
    bool matched = false;
    for (int j = 0; j < c; ++j) {
      TrkVal nxt = cur;
      if (j + 1 < c) nxt = trk_load(a, g, j + 1, lane);
      const double m = lane >= 16 && lane < TRK_V ? (double)cur.p : cur.m;   // the pose floats convert exactly
      const double b0 = trk_lane(m, 0), b1 = trk_lane(m, 1), b2 = trk_lane(m, 2), b3 = trk_lane(m, 3);
      int w = -1;         // the slot this detection updates or starts (uniform)
      bool hit = false;   // matched an existing track (uniform)
      if (isfinite(b0) && isfinite(b1) && isfinite(b2) && isfinite(b3)) {
        const float f0 = (float)b0, f1 = (float)b1, f2 = (float)b2, f3 = (float)b3;
        const float fd[4] = {f0, f1, f2, f3}, fr[4] = {r0, r1, r2, r3};
        const float u = box_iou(fd, fr);
        const bool q = id >= 0 && !matched && u > a.iou;
        const uint32_t ub = __float_as_uint(u);
        unsigned long long cand = __ballot(q);
        uint64_t best = 0;
        while (cand) {   // uniform: the maximum of (IoU bits, 63 - slot) over the qualifying lanes
          const int l = __ffsll(cand) - 1;
          cand &= cand - 1;
          const uint64_t key = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)ub, l) << 32) | (uint32_t)(63 - l);
          if (!hit || key > best) {
            best = key;
            hit = true;
          }
        }
        if (hit) {
          w = 63 - (int)(uint32_t)best;
        } else {
          const unsigned long long fr = __ballot(own && id < 0);
          if (fr) w = __ffsll(fr) - 1;
        }
        if (w >= 0 && lane == w) {
          if (!hit) id = next_id;
          matched = true;
          miss = 0;
          r0 = f0;
          r1 = f1;
          r2 = f2;
          r3 = f3;
        }
      }
      double o = m;   // what goes out: the input's bits unless the detection is tracked
      int32_t oid = -1;
      if (w >= 0) {
        oid = hit ? __builtin_amdgcn_readlane(id, w) : next_id;
        if (!hit) next_id = (int32_t)(((uint32_t)next_id + 1u) & 0x7fffffffu);
        if (lane < TRK_D) {
          double* p = sd + w * TRK_D + lane;
          if (hit && lane < TRK_V) o = a.alpha * m + a.om * *p;
          *p = o;
        }
      }
      const int64_t d = g * M + j;
      if (lane < 4) {
        a.boxes_out[d * 4 + lane] = o;
      } else if (lane < 16) {
        a.keypoints_out[d * 12 + (lane - 4)] = o;
      } else if (lane < TRK_V) {
        a.poses_out[d * 3 + (lane - 16)] = w >= 0 ? (float)o : cur.p;
      } else if (lane == TRK_V) {
        a.track_out[d] = oid;
      }
      cur = nxt;
    }
    if (id >= 0 && !matched) {
      miss = (int32_t)((uint32_t)miss + 1u);
      if (miss > a.max_missed) id = -1;
    }
  }
  __syncthreads();
  for (int i = lane; i < K * TRK_D; i += TRK_T) sdg[i] = sd[i];
  if (lane == 0) si[0] = next_id;
  if (own) {
    si[1 + lane] = id;
    si[1 + K + lane] = miss;
  }
}

__global__ void __launch_bounds__(256) track_reset_kernel(int64_t S, int K, int32_t* state_i, double* state_d) {
  const int W = 1 + 2 * K;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < S * K * TRK_D; i += (int64_t)gridDim.x * 256) {
    if (i < S * W) {   // fewer ints than doubles: 1 + 2 K < 23 K
      const int k = (int)(i % W);
      state_i[i] = (k >= 1 && k <= K) ? -1 : 0;
    }
    state_d[i] = 0.0;
  }
}

static int trk_check_tracks(const char* fn, int32_t max_tracks) {
  if (max_tracks < 1 || max_tracks > HPE_TRACK_MAX_TRACKS)
    return hpe_fail(HPE_EINVAL, "%s: max_tracks %d outside 1 .. HPE_TRACK_MAX_TRACKS = %d", fn, max_tracks,
                    HPE_TRACK_MAX_TRACKS);
  return HPE_OK;
}

extern "C" int hpe_track_reset(int64_t n_streams, int32_t max_tracks, int32_t* state_i, double* state_d,
                               void* stream) {
  if (n_streams < 0) return hpe_fail(HPE_EINVAL, "hpe_track_reset: negative stream count");
  if (trk_check_tracks("hpe_track_reset", max_tracks)) return HPE_EINVAL;
  if (n_streams > 0x7fffffff) return hpe_fail(HPE_EINVAL, "hpe_track_reset: too many streams");
  if (n_streams == 0) return HPE_OK;
  if (!state_i || !state_d) return hpe_fail(HPE_EINVAL, "hpe_track_reset: null argument");
  const int64_t blocks = (n_streams * max_tracks * TRK_D + 255) / 256;
  hipLaunchKernelGGL(track_reset_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0,
                     (hipStream_t)stream, n_streams, (int)max_tracks, state_i, state_d);
  return hpe_launched("hpe_track_reset");
}

extern "C" int hpe_track(int64_t n_streams, int32_t n_frames, int32_t max_faces, const int32_t* count,
                         const double* boxes, const double* keypoints, const float* poses, double alpha,
                         float match_iou, int32_t max_missed, int32_t max_tracks, int32_t* state_i,
                         double* state_d, int32_t* track_out, double* boxes_out, double* keypoints_out,
                         float* poses_out, void* stream) {
  if (n_streams < 0 || n_frames < 0)
    return hpe_fail(HPE_EINVAL, "hpe_track: negative stream count %lld or frame count %d", (long long)n_streams,
                    n_frames);
  if (max_faces < 1) return hpe_fail(HPE_EINVAL, "hpe_track: max_faces %d must be positive", max_faces);
  if (trk_check_tracks("hpe_track", max_tracks)) return HPE_EINVAL;
  if (max_missed < 0) return hpe_fail(HPE_EINVAL, "hpe_track: negative max_missed %d", max_missed);
  if (!(alpha > 0.0 && alpha <= 1.0)) return hpe_fail(HPE_EINVAL, "hpe_track: alpha %g must be in (0, 1]", alpha);
  if (match_iou != match_iou) return hpe_fail(HPE_EINVAL, "hpe_track: match_iou is NaN");
  if (n_frames > 0 && n_streams > 0x7fffffff / n_frames) return hpe_fail(HPE_EINVAL, "hpe_track: batch too large");
  if (n_streams * n_frames == 0) return HPE_OK;
  if (!count || !boxes || !keypoints || !poses || !state_i || !state_d || !track_out || !boxes_out ||
      !keypoints_out || !poses_out)
    return hpe_fail(HPE_EINVAL, "hpe_track: null argument");
  const TrackArgs a = {n_frames, max_faces, max_tracks, count, boxes, keypoints, poses, alpha, 1.0 - alpha,
                       match_iou, max_missed, state_i, state_d, track_out, boxes_out, keypoints_out, poses_out};
  hipLaunchKernelGGL(track_kernel, dim3((unsigned)n_streams), dim3(TRK_T), 0, (hipStream_t)stream, a);
  return hpe_launched("hpe_track");
}
