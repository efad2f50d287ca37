"""Time hpe.preprocess.prepare_input (one fused kernel: uint8 frames -> network input) against the
torch-on-GPU chain doing the same job in passes (uint8 -> float, channel flip, / 255,
F.interpolate(mode='bicubic', align_corners=False), normalise).  The chain's numerics differ (A =
-0.75, no border renormalisation): it is a yardstick for time only.

Shapes: 1,024 frames of 256x256 -> 128x128 and one 720x720 frame -> 128x128.  Each sample is a HIP
event pair around ``inner`` back-to-back calls (so a sample is not a single launch's jitter), the two
contenders alternate, warm-up first, median over ``--runs`` samples.  GB/s is over the bytes the job
needs: the crop's input bytes plus the fp32 output bytes.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
from hpe.preprocess import prepare_input  # noqa: E402


def torch_chain(u8, size):
    x = u8.float()
    x = x.flip(-1)
    x = x / 255
    x = F.interpolate(x.permute(0, 3, 1, 2), size=(size, size), mode='bicubic', align_corners=False)
    x = (x - 0.5) / 0.5
    return x.permute(0, 2, 3, 1).contiguous()


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
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('preprocess_bench needs a GPU')
    assert args.runs >= 20
    g = torch.Generator(device='cuda').manual_seed(0)
    for name, n, hw, size, inner in (('batch_1024x256', 1024, 256, 128, 2), ('single_720', 1, 720, 128, 50)):
        u8 = torch.randint(0, 256, (n, hw, hw, 3), dtype=torch.uint8, device='cuda', generator=g)
        out = torch.empty((n, size, size, 3), dtype=torch.float32, device='cuda')
        fused = lambda: prepare_input(u8, size=size, bgr=True, out=out)   # noqa: E731
        chain = lambda: torch_chain(u8, size)                            # noqa: E731
        for _ in range(args.warmup):
            sample(fused, inner)
            sample(chain, inner)
        tf, tc = [], []
        for _ in range(args.runs):
            tf.append(sample(fused, inner))
            tc.append(sample(chain, inner))
        diff = float((fused() - chain()).abs().max())
        mf, mc = float(np.median(tf)), float(np.median(tc))
        nbytes = n * hw * hw * 3 + n * size * size * 3 * 4
        print(json.dumps({'shape': name, 'frames': n, 'in': hw, 'out': size, 'runs': args.runs, 'inner': inner,
                          'fused_ms': round(mf, 5), 'fused_ms_min_max': [round(min(tf), 5), round(max(tf), 5)],
                          'chain_ms': round(mc, 5), 'chain_ms_min_max': [round(min(tc), 5), round(max(tc), 5)],
                          'ratio': round(mf / mc, 4), 'fused_GBps': round(nbytes / mf / 1e6, 1),
                          'max_abs_diff_vs_chain': round(diff, 4)}), flush=True)
        del u8, out


if __name__ == '__main__':
    main()
