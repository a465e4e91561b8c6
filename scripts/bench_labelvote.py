"""Times moving a full-size label map (240x240x155, the BraTS extent) through an oblique affine by vote (ops.label_resample3d,
csrc/conform.hip: bts_label_resample3d) beside the two gathers it stands between -- ops.affine_resample3d at orders 0 and 1 with C = 1 on
the same volume and map -- and, with --host, the numpy restatement tests/labelvote_ref.py.  Prints one JSON line.

    python scripts/bench_labelvote.py [--runs 20] [--warmup 3]          # the device passes
    python scripts/bench_labelvote.py --host                            # the numpy restatement alone (no GPU needed)

Device times are HIP events on the launch stream, median of --runs after --warmup.  `min_bytes` is the input once plus the output once;
`of_copy` relates the achieved rate to the 6.29 TB/s a float4 copy reaches on this chip.  The map is that of
scripts/bench_conform.py (12 degrees about a skew axis, 0.97 zoom, about the centres): nearly the whole output lies inside the field of
view, so every voxel pays its taps.  The labels are nested ellipsoids of 2 around 1 around 4 on 0 with 3 % speckle
(labelvote_ref.label_volume), so the taps of many voxels disagree; `differs_from_nearest` is the fraction of voxels inside the field of
view on which the vote and order 0 give different labels.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

import conform_ref  # noqa: E402
import labelvote_ref  # noqa: E402
from bench_conform import COPY_RATE, SHAPE, oblique, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='time the numpy restatement on the host and nothing else')
    args = ap.parse_args()
    yn = labelvote_ref.label_volume(SHAPE, 0)
    m = oblique()
    if args.host:
        t0 = time.perf_counter()
        labelvote_ref.label_vote(yn, m, SHAPE)
        print(json.dumps({'shape': SHAPE, 'host': {'numpy_label_vote_ms': round(1e3 * (time.perf_counter() - t0), 1)}}))
        return
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    y = torch.from_numpy(yn).cuda().unsqueeze(-1).contiguous()
    nbytes = 2 * y.numel() * 4
    res = {'shape': SHAPE, 'min_bytes': nbytes, 'runs': args.runs}

    def entry(ms, best):
        return {'ms': round(ms, 4), 'best_ms': round(best, 4), 'TBps': round(nbytes / (ms * 1e-3) / 1e12, 3),
                'of_copy': round(nbytes / (ms * 1e-3) / COPY_RATE, 3)}

    out = torch.empty_like(y)
    res['torch_copy'] = entry(*timed(lambda: out.copy_(y), args.runs, args.warmup))
    for order in (0, 1):
        res['affine_order%d' % order] = entry(*timed(lambda: ops.affine_resample3d(y, m, SHAPE, order=order, out=out), args.runs, args.warmup))
    nearest = ops.affine_resample3d(y, m, SHAPE, order=0)
    res['label_vote'] = entry(*timed(lambda: ops.label_resample3d(y, m, SHAPE, out=out), args.runs, args.warmup))
    inside = torch.from_numpy(conform_ref.inside(m, SHAPE, SHAPE)).cuda().unsqueeze(-1)
    res['inside_field_of_view'] = round(float(inside.float().mean()), 4)
    res['differs_from_nearest'] = round(float(((out != nearest) & inside).sum()) / float(inside.sum()), 4)
    res['vote_over_order1'] = round(res['label_vote']['ms'] / res['affine_order1']['ms'], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
