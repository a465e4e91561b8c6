"""Times the lesion-wise score (csrc/lesion.hip, bts_amd.infer.lesionwise_scores) on a full-size case.

    python scripts/lesionwise_measure.py [--out profiles/lesionwise_measure.json] [--repeat 5]

Input: a synthetic 240 x 240 x 155 truth / prediction pair of twelve ellipsoidal lesions (labels 2 around 1 around 4), each predicted
shifted and rescaled, two of them not predicted at all, and three predicted blobs where there is no lesion.  Every time is the median over `--repeat` calls after a warm-up, by device events around
the call.  The host comparison runs the SciPy restatement of the tests (tests/lesion_ref.py) on the same maps, with
scipy.ndimage.distance_transform_edt on each lesion's bounding box in place of the tests' brute-force transform, and reports its time and
the largest relative difference of a score.  Kernel times come from a kernel trace of a separate run of this script
(rocprofv3 --kernel-trace --stats -- python scripts/lesionwise_measure.py --trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import bts_amd  # noqa: E402,F401
from bts_amd import infer, ops  # noqa: E402

SHAPE = (240, 240, 155)
SPACING = (1.0, 1.0, 1.0)
ELEMENTWISE_TBPS = 6.3  # the streaming rate DESIGN section 20 holds its kernels against (what the element-wise passes reach)


def ellipsoid(lab, centre, radii, inner=(1.0, 0.6, 0.35), values=(2, 1, 4)):
    lo = [max(0, int(c - r) - 1) for c, r in zip(centre, radii)]
    hi = [min(s, int(c + r) + 2) for c, r, s in zip(centre, radii, lab.shape)]
    g = np.meshgrid(*[np.arange(a, b, dtype=np.float32) for a, b in zip(lo, hi)], indexing='ij')
    r2 = sum(((x - c) / r) ** 2 for x, c, r in zip(g, centre, radii))
    view = lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
    for f, v in zip(inner, values):
        view[r2 < f * f] = v


def synthetic_pair(seed=0):
    rng = np.random.default_rng(seed)
    truth, pred = np.zeros(SHAPE, np.uint8), np.zeros(SHAPE, np.uint8)
    centres = [(40, 50, 40), (40, 50, 62), (60, 160, 50), (110, 70, 100), (120, 120, 75), (120, 150, 75), (170, 60, 40), (180, 180, 110),
               (200, 110, 60), (90, 200, 120), (30, 200, 30), (215, 215, 130)]
    for i, c in enumerate(centres):
        radii = tuple(float(v) for v in rng.uniform(7.0, 14.0, size=3))
        ellipsoid(truth, c, radii)
        if i in (6, 10):                                        # missed
            continue
        shift = rng.uniform(-3.0, 3.0, size=3)
        ellipsoid(pred, tuple(float(a + b) for a, b in zip(c, shift)), tuple(float(r * f) for r, f in zip(radii, rng.uniform(0.8, 1.15, size=3))))
    for c in [(20, 20, 20), (150, 30, 130), (225, 120, 20)]:    # false positives
        ellipsoid(pred, c, (5.0, 6.0, 4.0))
    return truth, pred


def fast_hd95(les, m, spacing, percentile):
    from scipy import ndimage as ndi
    import surface_ref as S
    idx = np.argwhere(les | m)
    sl = tuple(slice(int(a), int(b) + 1) for a, b in zip(idx.min(axis=0), idx.max(axis=0)))
    st, sp = S.surface(les[sl]), S.surface(m[sl])
    dt, dp = ndi.distance_transform_edt(~st, sampling=spacing), ndi.distance_transform_edt(~sp, sampling=spacing)
    return float(np.percentile(np.concatenate([dt[sp], dp[st]]), percentile))


def timed(fn, repeat):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {'median_ms': float(np.median(ms)), 'min_ms': float(min(ms)), 'max_ms': float(max(ms))}


def rel(a, b):
    if np.isnan(a) and np.isnan(b):
        return 0.0
    return abs(a - b) / max(abs(a), abs(b), 1e-300) if a != b else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lesionwise_measure.json'))
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--trace', action='store_true', help='for a kernel trace: the calls alone, no host comparison, nothing written')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    truth_h, pred_h = synthetic_pair()
    truth, pred = torch.from_numpy(truth_h).to(dev), torch.from_numpy(pred_h).to(dev)
    n = truth_h.size
    res = {'device': torch.cuda.get_device_name(0), 'repeat': args.repeat, 'timing': 'device events around the call',
           'shape': list(SHAPE), 'voxels': n, 'truth_voxels': int((truth_h > 0).sum()), 'predicted_voxels': int((pred_h > 0).sum())}

    t = timed(lambda: infer.lesionwise_scores(truth, pred, SPACING), args.repeat)
    got = infer.lesionwise_scores(truth, pred, SPACING)
    t['counts'] = {name: got['lw_counts_' + name] for name in ('wt', 'tc', 'et')}
    t['scores'] = {k: v for k, v in got.items() if k.startswith('lw_dice') or k.startswith('lw_hd95')}
    t['below_the_42_ms_tta_forward'] = bool(t['median_ms'] < 42.0)
    res['lesionwise_scores'] = t

    # the dilation alone: fused passes against ping-pong passes, held against one read plus one write of the map
    out = torch.empty_like(truth)
    res['dilate3d'] = {}
    for conn in (18,) if args.trace else (6, 18, 26):
        for fuse in (1, 3):
            d = timed(lambda: ops.dilate3d(truth, 14, 4, conn, 3, out=out, fuse=fuse), args.repeat)
            passes = 3 if fuse == 1 else 1
            side, width = 16 - 2 * fuse, 64 - 2 * fuse
            tiles = -(-SHAPE[0] // side) * -(-SHAPE[1] // side) * -(-SHAPE[2] // width)
            d.update(passes=passes, bytes_loaded=passes * tiles * 64 * 256, bytes_stored=passes * n, bytes_one_read_one_write=2 * n)
            d['read_write_floor_ms_at_%.1f_TBps' % ELEMENTWISE_TBPS] = 2 * n / (ELEMENTWISE_TBPS * 1e12) * 1e3
            res['dilate3d']['conn%d_fuse%d' % (conn, fuse)] = d
    res['dilate3d']['iterations0'] = timed(lambda: ops.dilate3d(truth, 14, 4, 18, 0, out=out), args.repeat)

    # the pairing pass and the boxes on the whole-tumour maps
    td = ops.components3d(ops.dilate3d(truth, 14, 4, 18, 3), 2, 2, 26)
    pc = ops.components3d(pred, 14, 4, 26)
    cnt = torch.zeros(2, dtype=torch.int64, device=dev)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    ops.component_sizes(td, out=size, count=cnt[0:1])
    ops.component_sizes(pc, out=size, count=cnt[1:2])
    counts = tuple(cnt.cpu().tolist())
    vox = torch.empty(n, dtype=torch.int32, device=dev)
    p = timed(lambda: ops.lesion_pairs(td, truth, pc, 14, counts=counts, lesion_vox=vox), args.repeat)
    rows, _ = ops.lesion_pairs(td, truth, pc, 14, counts=counts, lesion_vox=vox)
    p.update(components=list(counts), pairs=len(rows), capacity=ops.lesion_pairs_capacity(*counts), includes='the host read of the table',
             bytes_read=9 * n, bytes_zeroed=4 * n)
    res['lesion_pairs'] = p
    roots = torch.nonzero(vox).view(-1).to(torch.int32)
    res['component_boxes'] = timed(lambda: ops.component_boxes(td, roots), args.repeat)

    if not args.trace:
        import lesion_ref as L
        t0 = time.time()
        want = L.lesionwise_scores(truth_h, pred_h, SPACING, hd95=fast_hd95)
        host = {'seconds': time.time() - t0, 'what': 'tests/lesion_ref.py with scipy.ndimage.distance_transform_edt on bounding boxes'}
        host['counts_equal'] = all(got['lw_counts_' + k] == want['lw_counts_' + k] for k in ('wt', 'tc', 'et'))
        ints = ('voxels', 'matched_components', 'matched_voxels', 'overlap')
        host['lesion_rows_equal'] = all([[a[i] for i in ints] for a in got['lw_lesions_' + k]] == [[b[i] for i in ints] for b in want['lw_lesions_' + k]]
                                        for k in ('wt', 'tc', 'et'))
        host['largest_relative_difference_of_a_score'] = max(rel(got[k], want[k]) for k in t['scores'])
        host['largest_relative_difference_of_a_lesion_hd95'] = max(
            [rel(a['hd95'], b['hd95']) for k in ('wt', 'tc', 'et') for a, b in zip(got['lw_lesions_' + k], want['lw_lesions_' + k])] or [0.0])
        res['host_reference'] = host
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
