"""Times the connected-component post-processing (csrc/components.hip) on a full-size case.

    python scripts/components_measure.py [--out profiles/components_measure.json] [--repeat 5]

Input: a synthetic 240 x 240 x 155 BraTS-like label map of nested blobs (labels 2 around 1 around 4) with 0.05 % of the voxels set to
a random label, the map of DESIGN section 19; and a 160 x 200 x 160 candidate brain of about 1.5 M voxels with a few fragments beside
it.  Every time is the median over `--repeat` calls after a warm-up, by device events around the call.  Where SciPy is installed the
same results are computed with scipy.ndimage.label on the host and compared.  Kernel times come from a kernel trace of a separate run
of this script (rocprofv3 --kernel-trace --stats -- python scripts/components_measure.py --trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bts_amd  # noqa: E402,F401
from bts_amd import infer, ops  # noqa: E402

HBM_TBPS = 6.3          # the streaming rate the labelling is held against


def nested_blobs(shape=(240, 240, 155), noise=0.0005, seed=0):
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape], indexing='ij')
    r2 = ((g[0] - 0.1) / 0.45) ** 2 + ((g[1] + 0.05) / 0.4) ** 2 + (g[2] / 0.5) ** 2
    lab = np.zeros(shape, np.uint8)
    lab[r2 < 1.0] = 2
    lab[r2 < 0.45] = 1
    lab[r2 < 0.15] = 4
    rng = np.random.default_rng(seed)
    hit = rng.random(shape) < noise
    lab[hit] = np.array([0, 1, 2, 4], np.uint8)[rng.integers(0, 4, size=int(hit.sum()))]
    return lab


def brain_candidate(shape=(160, 200, 160), seed=1):
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in shape], indexing='ij')
    brain = (g[0] / 0.86) ** 2 + (g[1] / 0.8) ** 2 + (g[2] / 0.8) ** 2 < 1.0
    eyes = sum(((g[0] - 0.9) / 0.08) ** 2 + ((g[1] - s * 0.3) / 0.1) ** 2 + ((g[2] + 0.85) / 0.1) ** 2 < 1.0 for s in (-1.0, 1.0)) > 0
    neck = (np.abs(g[0] + 0.93) < 0.05) & (np.abs(g[1]) < 0.2) & (np.abs(g[2]) < 0.2)
    cand = (brain | eyes | neck).astype(np.uint8)
    rng = np.random.default_rng(seed)
    cand[rng.random(shape) < 0.0002] = 1
    return cand


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


def canonical_scipy(region, rank):
    from scipy import ndimage as ndi
    labels, n = ndi.label(region, ndi.generate_binary_structure(3, rank))
    first = ndi.minimum(np.arange(region.size).reshape(region.shape), labels, np.arange(1, n + 1)) + 1
    return np.concatenate([[0], np.atleast_1d(first)])[labels].astype(np.int32), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'components_measure.json'))
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--trace', action='store_true', help='for a kernel trace: 26 neighbours only, no host comparison')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    have_scipy = have_scipy and not args.trace
    res = {'device': torch.cuda.get_device_name(0), 'repeat': args.repeat, 'scipy': have_scipy, 'timing': 'device events around the call'}

    lab_h = nested_blobs()
    n = lab_h.size
    lab = torch.from_numpy(lab_h).to(dev)
    comp = torch.empty(lab_h.shape, dtype=torch.int32, device=dev)
    res['label_map'] = {'shape': list(lab_h.shape), 'voxels': n, 'whole_tumour_voxels': int((lab_h > 0).sum())}
    for conn, rank in ((6, 1), (18, 2), (26, 3)):
        if args.trace and conn != 26:
            continue
        t = timed(lambda: ops.components3d(lab, 14, 4, conn, out=comp), args.repeat)
        moved = 3 * 5 * n                              # 1 B read and 4 B written per voxel in each of the three kernels
        t['bytes_moved_nominal'] = moved
        t['nominal_TBps'] = moved / (t['median_ms'] * 1e-3) / 1e12
        t['fraction_of_%.1f_TBps' % HBM_TBPS] = t['nominal_TBps'] / HBM_TBPS
        size, count = ops.component_sizes(comp)
        t['components'] = int(count.item())
        if have_scipy:
            t0 = time.time()
            ref, nref = canonical_scipy(lab_h > 0, rank)
            t['scipy_label_s'] = time.time() - t0
            t['equal_to_scipy'] = bool(np.array_equal(comp.cpu().numpy(), ref)) and nref == t['components']
        res['components3d_%d' % conn] = t

    ops.components3d(lab, 14, 4, 26, out=comp)
    size = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    key = torch.zeros(1, dtype=torch.int64, device=dev)
    removed = torch.zeros(2, dtype=torch.int64, device=dev)
    work = lab.clone()
    res['component_sizes'] = timed(lambda: ops.component_sizes(comp, out=size, count=count), args.repeat)
    res['component_largest'] = timed(lambda: ops.component_largest(size, out=key), args.repeat)
    res['components_apply_min100'] = timed(lambda: ops.components_apply(work, comp, size, None, 100, False, 0, removed=removed), args.repeat)
    res['region_relabel'] = timed(lambda: ops.region_relabel(work, 8, 1, 10, K=4), args.repeat)

    def post():
        w = lab.clone()
        return w, infer.postprocess_labels(w, min_component_voxels=100, et_min_voxels=50, connectivity=26)

    t = timed(lambda: post(), args.repeat)
    w, counts = post()
    t['counts'] = counts
    t['includes'] = 'a clone of the map and the host read of the counts'
    if have_scipy:
        from scipy import ndimage as ndi
        t0 = time.time()
        ref = lab_h.copy()
        labels, nl = ndi.label(ref > 0, ndi.generate_binary_structure(3, 3))
        sizes = ndi.sum(np.ones_like(labels), labels, np.arange(1, nl + 1))
        small = np.concatenate([[False], sizes < 100])[labels]
        ref[small] = 0
        if 0 < int((ref >= 3).sum()) < 50:
            ref[ref >= 3] = 1
        t['scipy_host_s'] = time.time() - t0
        t['equal_to_scipy'] = bool(np.array_equal(w.cpu().numpy(), ref))
    res['postprocess_labels'] = t

    cand_h = brain_candidate()
    cand = torch.from_numpy(cand_h).to(dev)

    def brain():
        w = cand.clone()
        return w, infer.remove_components(w, 2, K=2, connectivity=26, largest_only=True)

    t = timed(lambda: brain(), args.repeat)
    w, counts = brain()
    t.update(shape=list(cand_h.shape), candidate_voxels=int(cand_h.sum()), counts=counts, kept_voxels=int(w.sum().item()))
    if have_scipy:
        from scipy import ndimage as ndi
        t0 = time.time()
        labels, nl = ndi.label(cand_h > 0, ndi.generate_binary_structure(3, 3))
        sizes = ndi.sum(np.ones_like(labels), labels, np.arange(1, nl + 1))
        ref = (labels == 1 + int(np.argmax(sizes))).astype(np.uint8)
        t['scipy_host_s'] = time.time() - t0
        t['equal_to_scipy'] = bool(np.array_equal(w.cpu().numpy(), ref))
    res['skull_largest_component'] = t

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == '__main__':
    main()
