"""Time drawing on the device (hpe_pose_prims, hpe_draw, hpe_draw_nv12; csrc/hpe_draw.hip) and the floor
of the only route to an annotated frame there was before it: every frame copied device -> pinned host ->
device with nothing drawn in between (the drawing itself, on the host, would come on top; hpe ships no
host rasteriser and no host NV12 <-> BGR conversion, so none is timed).

Data: ``--frames`` frames of ``--width`` x ``--height``, packed BGR and NV12, seeded random bytes;
``--max-faces`` slots per frame, of which 0, 1, 4 and 16 hold a face: seeded random square boxes of 5 to
30 % of the frame height, keypoints inside them, angles N(0, 30).  Each C call: a HIP event pair around
the bare call, warm-up first, median over ``--runs`` samples with min - max beside it, the contenders
alternating.  ``launch``: hpe_pose_prims for one image of one slot, a one-workgroup kernel, for the cost
of a launch as this script sees it.  The copies: a host clock around the synchronised pair of copies,
``--host-runs`` samples.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
from hpe import _lib  # noqa: E402
from hpe.draw import FACE_PRIMS, PRIM_WORDS, DrawStyle  # noqa: E402


def faces(n, M, k, h, w, seed, dev='cuda'):
    """k faces in each of n frames: count, boxes, keypoints, poses as hpe_detect writes them."""
    g = torch.Generator(device=dev).manual_seed(seed)
    side = (0.05 + 0.25 * torch.rand((n, M, 1), dtype=torch.float64, device=dev, generator=g)) * h
    x = torch.rand((n, M, 1), dtype=torch.float64, device=dev, generator=g) * (w - side)
    y = torch.rand((n, M, 1), dtype=torch.float64, device=dev, generator=g) * (h - side)
    boxes = torch.cat([x / w, y / h, (x + side) / w, (y + side) / h], -1)
    u = torch.rand((n, M, 6, 2), dtype=torch.float64, device=dev, generator=g)
    kps = torch.stack([(x + u[..., 0] * side) / w, (y + u[..., 1] * side) / h], -1)
    poses = 30 * torch.randn((n, M, 3), device=dev, generator=g)
    return dict(count=torch.full((n,), k, dtype=torch.int32, device=dev), boxes=boxes.contiguous(),
                keypoints=kps.contiguous(), poses=poses)


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def round_trip(t, pinned):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pinned.copy_(t)
    torch.cuda.synchronize()
    t.copy_(pinned)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--max-faces', type=int, default=100)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--host-runs', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('draw_bench needs a GPU')
    n, h, w, M = args.frames, args.height, args.width, args.max_faces
    g = torch.Generator(device='cuda').manual_seed(1)
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device='cuda', generator=g)
    nv12 = torch.randint(0, 256, (n, h + h // 2, w), dtype=torch.uint8, device='cuda', generator=g)
    style = DrawStyle()
    col_bgr = torch.from_numpy(style.colours()).cuda()
    col_yuv = torch.from_numpy(style.colours(nv12='bt601')).cuda()
    lib, p, st = _lib.load(), _lib.ptr, _lib.stream
    P = FACE_PRIMS * M
    tables = {}
    for k in (0, 1, 4, 16):
        tables[k] = (faces(n, M, k, h, w, seed=k), torch.zeros((n, P, PRIM_WORDS), dtype=torch.int32, device='cuda'),
                     torch.zeros(n, dtype=torch.int32, device='cuda'))
    tiny = faces(1, 1, 1, h, w, seed=9)
    tiny_p, tiny_n = torch.zeros((1, FACE_PRIMS, PRIM_WORDS), dtype=torch.int32, device='cuda'), torch.zeros(
        1, dtype=torch.int32, device='cuda')

    def prims(k):
        d, t, c = tables[k]
        _lib.check(lib.hpe_pose_prims(p(d['count']), p(d['boxes']), p(d['keypoints']), p(d['poses']), n, M, 0, 0, w, h,
                                      *style.sizes(), p(t), p(c), st()), 'hpe_pose_prims')

    def draw(k):
        _, t, c = tables[k]
        _lib.check(lib.hpe_draw(p(bgr), n, h, w, 3 * w, 3 * w * h, p(t), p(c), P, p(col_bgr), 5, st()), 'hpe_draw')

    def draw_nv12(k):
        _, t, c = tables[k]
        _lib.check(lib.hpe_draw_nv12(p(nv12), ctypes.c_void_p(nv12.data_ptr() + h * w), n, h, w, w, (h + h // 2) * w, w,
                                     (h + h // 2) * w, p(t), p(c), P, p(col_yuv), 5, st()), 'hpe_draw_nv12')

    def launch(_):
        _lib.check(lib.hpe_pose_prims(p(tiny['count']), p(tiny['boxes']), p(tiny['keypoints']), p(tiny['poses']), 1, 1,
                                      0, 0, w, h, *style.sizes(), p(tiny_p), p(tiny_n), st()), 'hpe_pose_prims')

    calls = [('hpe_pose_prims', prims), ('hpe_draw', draw), ('hpe_draw_nv12', draw_nv12), ('launch', launch)]
    times = {(name, k): [] for name, _ in calls for k in tables}
    for i in range(args.warmup + args.runs):
        for k in tables:
            for name, fn in calls:
                t = sample(lambda: fn(k))
                if i >= args.warmup:
                    times[(name, k)].append(t)
    rec = {'frames': n, 'height': h, 'width': w, 'max_faces': M, 'runs': args.runs, 'warmup': args.warmup,
           'rows_per_frame': {str(k): int(tables[k][2][0].item()) for k in tables}}
    for (name, k), v in times.items():
        if name == 'launch' and k:
            continue
        key = name if name == 'launch' else '%s_%d_faces' % (name, k)
        rec[key + '_ms'] = round(float(np.median(v)), 4)
        rec[key + '_ms_min_max'] = [round(min(v), 4), round(max(v), 4)]
    for name, t in (('bgr', bgr), ('nv12', nv12)):
        pinned = torch.empty(t.shape, dtype=torch.uint8, pin_memory=True)
        round_trip(t, pinned)
        v = [round_trip(t, pinned) for _ in range(args.host_runs)]
        rec['copy_%s_device_host_device_ms' % name] = round(float(np.median(v)), 2)
        rec['copy_%s_device_host_device_ms_min_max' % name] = [round(min(v), 2), round(max(v), 2)]
        rec['copy_%s_mbytes' % name] = round(t.numel() / 1e6, 1)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
