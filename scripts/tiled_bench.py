"""Time tiled detection (BlazeFaceDetector.detect_tiled) stage by stage: 64 device frames of 720x1280,
tile 256, overlap 64 — 7 x 4 tiles and the whole look, 29 table rows per frame, 1,856 ROI images, and at
max_faces = 100 a capacity of 2,900 candidates per frame for the merge.

Stages, each a HIP event pair around one call on tensors left by the stage before: prepare_rois
(hpe_preprocess_rois), the network forward (BlazeFace and the two pose regressors), postprocess
(hpe_detect) and merge_rois (hpe_merge_rois).  Then the whole detect_tiled call, which ends with the
host copy of the merged results, next to detect_images on the same frames.  The contenders alternate,
warm-up first, median over ``--runs`` samples with min - max beside it.  The frames are uniform noise,
on which the detector finds something in most looks at the 0.15 threshold used here, so the merge has
candidates to sort and suppress; the candidate count per frame is reported.  Noise fills a small part of
the candidate slots, so the merge is also timed on made-up per-ROI results with every slot filled
(``hpe_merge_rois_full``, outside the sum of the stages).  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'head-pose-estimation-model_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from hpe.detector import BlazeFaceDetector  # noqa: E402
from hpe.preprocess import prepare_rois, tile_rois  # noqa: E402
from util import fixture  # noqa: E402

RID = 'reg1-stoqa9pt-reg2-hrchr82r-selected'


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--tile', type=int, default=256)
    ap.add_argument('--overlap', type=int, default=64)
    ap.add_argument('--max-faces', type=int, default=100)
    ap.add_argument('--threshold', type=float, default=0.15)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('tiled_bench needs a GPU')
    n, h, w = args.frames, 720, 1280
    mc, wts = fixture(RID)
    det = BlazeFaceDetector(mc, wts, scoreThreshold=args.threshold, max_faces=args.max_faces)
    g = torch.Generator(device='cuda').manual_seed(0)
    u8 = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device='cuda', generator=g)
    table, per = tile_rois(n, h, w, args.tile, args.overlap)
    t = torch.from_numpy(table).cuda()
    dst = (0, 0, w, h)
    s = {}

    def prepare():
        s['x'] = prepare_rois(u8, t, size=128, device=det.device)

    def forward():
        s['outs'] = det.net.forward(s['x'])

    def detect():
        s['r'] = det.postprocess(s['outs'])

    def merge():
        s['m'] = det.merge_rois(s['r'], t, per, dst)

    # the merge at capacity: made-up per-ROI results with every slot of every row filled (boxes of a
    # tenth of their ROI at uniform places, uniform scores), which noise frames do not produce
    m_in = n * per
    full = dict(count=torch.full((m_in,), args.max_faces, dtype=torch.int32, device='cuda'),
                scores=torch.rand((m_in, args.max_faces), device='cuda', generator=g),
                keypoints=torch.rand((m_in, args.max_faces, 6, 2), dtype=torch.float64, device='cuda', generator=g),
                poses=torch.rand((m_in, args.max_faces, 3), device='cuda', generator=g))
    c = torch.rand((m_in, args.max_faces, 2), dtype=torch.float64, device='cuda', generator=g)
    full['boxes'] = torch.cat([c - 0.05, c + 0.05], -1).contiguous()

    def merge_full():
        s['mf'] = det.merge_rois(full, t, per, dst)

    fns = {
        'prepare_rois': prepare, 'forward': forward, 'hpe_detect': detect, 'hpe_merge_rois': merge,
        'hpe_merge_rois_full': merge_full,
        'detect_tiled': lambda: det.detect_tiled(u8, tile=args.tile, overlap=args.overlap, roi_batch=n * per),
        'detect_images': lambda: det.detect_images(u8),
    }
    for _ in range(args.warmup):
        for f in fns.values():
            sample(f)
    times = {k: [] for k in fns}
    for _ in range(args.runs):
        for k, f in fns.items():
            times[k].append(sample(f))
    med = {k: float(np.median(v)) for k, v in times.items()}
    cand = s['r']['count'].view(n, per).sum(1).cpu().numpy()
    kept = s['m']['count'].cpu().numpy()
    kept_full = s['mf']['count'].cpu().numpy()
    rec = {'frames': n, 'in': [h, w], 'tile': args.tile, 'overlap': args.overlap, 'rows_per_frame': per,
           'roi_images': n * per, 'max_faces': args.max_faces, 'capacity_per_frame': per * args.max_faces,
           'candidates_per_frame_min_median_max': [int(cand.min()), float(np.median(cand)), int(cand.max())],
           'kept_per_frame_min_median_max': [int(kept.min()), float(np.median(kept)), int(kept.max())],
           'full_candidates_per_frame': per * args.max_faces,
           'full_kept_per_frame_min_max': [int(kept_full.min()), int(kept_full.max())],
           'runs': args.runs, 'warmup': args.warmup}
    for k in fns:
        rec[k + '_ms'] = round(med[k], 4)
        rec[k + '_ms_min_max'] = [round(min(times[k]), 4), round(max(times[k]), 4)]
    stages = sum(med[k] for k in ('prepare_rois', 'forward', 'hpe_detect', 'hpe_merge_rois'))
    rec['stages_sum_ms'] = round(stages, 4)
    rec['merge_share_of_stages'] = round(med['hpe_merge_rois'] / stages, 5)
    rec['merge_share_of_detect_tiled'] = round(med['hpe_merge_rois'] / med['detect_tiled'], 5)
    rec['detect_tiled_over_detect_images'] = round(med['detect_tiled'] / med['detect_images'], 2)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
