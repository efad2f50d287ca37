"""Time hpe.preprocess.prepare_rois (hpe_preprocess_rois: one ROI row per output image, read from a
device table) against hpe.preprocess.prepare_input (hpe_preprocess: one crop for the batch) on the same
bytes and the same arithmetic: 1,024 frames of 480x640, the 480x480 centre square of each to 128x128.
A third contender is the same ROI count with every second ROI shifted so that it straddles the right
and the bottom border of its frame (those pixels take the per-tap frame-or-pad path).

Each sample is a HIP event pair around ``inner`` back-to-back calls, the contenders alternate, warm-up
first, median over ``--runs`` samples (min - max beside it: the run-to-run spread).  The in-frame ROI
output is checked to equal prepare_input's bit for bit before anything is timed.  GB/s is over the
bytes the job needs: the crop's input bytes plus the fp32 output bytes.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
from hpe.preprocess import prepare_input, prepare_rois  # noqa: E402


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--inner', type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('preprocess_rois_bench needs a GPU')
    assert args.runs >= 20
    n, h, w, side, size = args.frames, 480, 640, 480, 128
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device='cuda', generator=g)
    x0, y0 = (w - side) // 2, (h - side) // 2
    inside = np.array([(i, x0, y0, side, side) for i in range(n)], np.int32)
    border = inside.copy()
    border[1::2, 1] = w - side // 2         # the right half of the canvas is outside the frame
    border[1::2, 2] = h - side // 2         # and the bottom half
    t_in, t_bd = torch.from_numpy(inside).cuda(), torch.from_numpy(border).cuda()
    outs = [torch.empty((n, size, size, 3), dtype=torch.float32, device='cuda') for _ in range(3)]
    fns = {
        'prepare_input': lambda: prepare_input(u8, size=size, crop=(x0, y0, side, side), out=outs[0]),
        'rois_in_frame': lambda: prepare_rois(u8, t_in, size=size, out=outs[1]),
        'rois_half_on_border': lambda: prepare_rois(u8, t_bd, size=size, pad_value=(7, 130, 251), out=outs[2]),
    }
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    equal = bool(torch.equal(outs[0], outs[1]))
    assert equal, 'in-frame ROIs differ from prepare_input'
    assert bool(torch.equal(outs[0][0::2], outs[2][0::2])) and not bool(torch.equal(outs[0][1::2], outs[2][1::2]))
    for _ in range(args.warmup):
        for f in fns.values():
            sample(f, args.inner)
    t = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, f in fns.items():
            t[k].append(sample(f, args.inner))
    med = {k: float(np.median(v)) for k, v in t.items()}
    nbytes = n * side * side * 3 + n * size * size * 3 * 4
    rec = {'frames': n, 'in': [h, w], 'roi': side, 'out': size, 'runs': args.runs, 'inner': args.inner,
           'in_frame_equals_prepare_input': equal}
    for k in fns:
        rec[k + '_ms'] = round(med[k], 5)
        rec[k + '_ms_min_max'] = [round(min(t[k]), 5), round(max(t[k]), 5)]
    rec['ratio_in_frame'] = round(med['rois_in_frame'] / med['prepare_input'], 4)
    rec['ratio_half_on_border'] = round(med['rois_half_on_border'] / med['prepare_input'], 4)
    rec['prepare_input_GBps'] = round(nbytes / med['prepare_input'] / 1e6, 1)
    rec['rois_in_frame_GBps'] = round(nbytes / med['rois_in_frame'] / 1e6, 1)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
