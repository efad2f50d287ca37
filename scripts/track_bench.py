"""Time face tracking and smoothing (hpe_track, csrc/hpe_track.hip) against the only route there was
before it: the detections copied to the host and the webcam loop's 19 hpe.detector.EMAFilters per face,
indexed by the face's position in the frame's result list (which associates nothing).

Data: ``--streams`` videos of ``--frames`` frames, ``--max-faces`` slots per frame, 1 to 4 faces per
video on seeded random walks with occasional drop-outs (made on the device, no detector runs).  hpe_track:
a HIP event pair around one call that starts from a reset state, warm-up first, median over ``--runs``
samples with min - max beside it, for all streams and for the first stream alone; the contenders
alternate.  The host route: a host clock around the copy of count, boxes, keypoints and poses to the host
and the filter loop over every frame, ``--host-runs`` samples.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
from hpe import _lib  # noqa: E402
from hpe.detector import EMAFilter  # noqa: E402
from hpe.tracking import PoseTracker  # noqa: E402


def walks(S, T, M, seed, dev='cuda'):
    """count (S*T,), boxes (S*T, M, 4), keypoints (S*T, M, 6, 2), poses (S*T, M, 3) on the device."""
    g = torch.Generator(device=dev).manual_seed(seed)
    F = 4
    n_faces = torch.randint(1, F + 1, (S, 1, 1), device=dev, generator=g)
    c0 = 0.2 + 0.6 * torch.rand((S, 1, F, 2), dtype=torch.float64, device=dev, generator=g)
    c = c0 + 0.01 * torch.randn((S, T, F, 2), dtype=torch.float64, device=dev, generator=g).cumsum(1)
    hw = 0.04 + 0.06 * torch.rand((S, 1, F, 2), dtype=torch.float64, device=dev, generator=g)
    seen = (torch.rand((S, T, F), device=dev, generator=g) > 0.15) & (torch.arange(F, device=dev) < n_faces)
    seen[:, :, 0] |= ~seen.any(2)
    # the faces in view, packed to the front of the frame's slots in face order
    order = torch.argsort((~seen).to(torch.int8), dim=2, stable=True)
    box = torch.cat([c - hw, c + hw], -1).gather(2, order[..., None].expand(S, T, F, 4))
    boxes = torch.zeros((S, T, M, 4), dtype=torch.float64, device=dev)
    boxes[:, :, :min(F, M)] = box[:, :, :M]
    count = seen.sum(2).clamp(max=M).to(torch.int32).reshape(S * T)
    kps = torch.rand((S * T, M, 6, 2), dtype=torch.float64, device=dev, generator=g)
    poses = 30 * torch.randn((S * T, M, 3), device=dev, generator=g)
    return dict(count=count, boxes=boxes.reshape(S * T, M, 4).contiguous(), keypoints=kps, poses=poses,
                scores=torch.zeros((S * T, M), device=dev))


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_route(r, S, T, alpha):
    """The copy to the host and the reference loop: per video 19 filters per result position."""
    t0 = time.perf_counter()
    h = {k: r[k].cpu().numpy() for k in ('count', 'boxes', 'keypoints', 'poses')}
    M = h['boxes'].shape[1]
    for s in range(S):
        filt = [[EMAFilter(alpha) for _ in range(19)] for _ in range(M)]
        for g in range(s * T, (s + 1) * T):
            for j in range(int(h['count'][g])):
                f = filt[j]
                b, k, p = h['boxes'][g, j], h['keypoints'][g, j].reshape(12), h['poses'][g, j]
                for e in range(4):
                    b[e] = f[e].update(b[e])
                for e in range(12):
                    k[e] = f[4 + e].update(k[e])
                for e in range(3):
                    p[e] = f[16 + e].update(p[e])
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=64)
    ap.add_argument('--frames', type=int, default=256)
    ap.add_argument('--max-faces', type=int, default=100)
    ap.add_argument('--max-tracks', type=int, default=16)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-runs', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('track_bench needs a GPU')
    S, T, M, K = args.streams, args.frames, args.max_faces, args.max_tracks
    r = walks(S, T, M, seed=0)
    one = {k: v[:T] for k, v in r.items()}
    trk = {'all': PoseTracker(max_tracks=K, streams=S), 'one': PoseTracker(max_tracks=K, streams=1)}
    data = {'all': r, 'one': one}
    out = {k: trk[k].update(data[k]) for k in trk}   # the output tensors; the timed calls are the bare C call
    lib = _lib.load()
    p = _lib.ptr

    def call(k):
        t, d, o = trk[k], data[k], out[k]
        t.reset()
        return sample(lambda: _lib.check(lib.hpe_track(
            t.streams, T, M, p(d['count']), p(d['boxes']), p(d['keypoints']), p(d['poses']), t.alpha, t.match_iou,
            t.max_missed, K, p(t.state_i), p(t.state_d), p(o['track']), p(o['boxes']), p(o['keypoints']), p(o['poses']),
            _lib.stream()), 'hpe_track'))

    for _ in range(args.warmup):
        for k in trk:
            call(k)
    times = {k: [] for k in trk}
    for _ in range(args.runs):
        for k in trk:
            times[k].append(call(k))
    ids = out['all']['track'].cpu().numpy()
    cnt = r['count'].cpu().numpy()
    faces = int(cnt.sum())
    tracked = int(sum((ids[g, :c] >= 0).sum() for g, c in enumerate(cnt)))
    host = {k: [host_route(data[k], S if k == 'all' else 1, T, 0.15) for _ in range(args.host_runs)] for k in trk}
    rec = {'streams': S, 'frames': T, 'max_faces': M, 'max_tracks': K, 'detections': faces, 'tracked': tracked,
           'ids_issued': [int(v) for v in trk['all'].state()[0][:, 0][:8]], 'runs': args.runs, 'warmup': args.warmup}
    for k, name in (('all', 'hpe_track_%d_streams' % S), ('one', 'hpe_track_1_stream')):
        rec[name + '_ms'] = round(float(np.median(times[k])), 4)
        rec[name + '_ms_min_max'] = [round(min(times[k]), 4), round(max(times[k]), 4)]
    for k, name in (('all', 'host_filters_%d_streams' % S), ('one', 'host_filters_1_stream')):
        rec[name + '_ms'] = round(float(np.median(host[k])), 2)
        rec[name + '_ms_min_max'] = [round(min(host[k]), 2), round(max(host[k]), 2)]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
