"""Times the two device passes of infer.Conformer on a full-size scan (240x240x155x4, the BraTS extent) and, with --host, the same
arithmetic in numpy and SciPy.  Prints one JSON line.

    python scripts/bench_conform.py [--runs 20] [--warmup 3]          # the device passes
    python scripts/bench_conform.py --host                            # the host figures alone (no GPU needed)

Device times are HIP events on the launch stream, median of --runs after --warmup.  `min_bytes` is the input once plus the output once;
`of_copy` relates the achieved rate to the 6.29 TB/s a float4 copy reaches on this chip.  The resampling matrix is oblique
(12 degrees about a skew axis, 0.97 zoom, about the centres): nearly the whole output lies inside the field of view, so every voxel
pays its taps.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12
SHAPE, C = (240, 240, 155), 4
TRANSPOSING = ((2, 0, 1), (False, True, False))      # the output W axis runs along the source D axis: the LDS-tiled path
FLIPS_ONLY = ((0, 1, 2), (True, True, False))        # RAS -> LPS: rows stay rows


def oblique():
    k = np.array([1.0, 2.0, -1.5])
    k /= np.linalg.norm(k)
    kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    t = np.deg2rad(12.0)
    lin = 0.97 * (np.eye(3) + np.sin(t) * kx + (1 - np.cos(t)) * (kx @ kx))
    c = (np.array(SHAPE) - 1) / 2.0
    return np.concatenate([lin, (c - lin @ c)[:, None]], axis=1)


def timed(fn, runs, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def host(x):
    out = {}
    t0 = time.perf_counter()
    perm, flip = TRANSPOSING
    np.ascontiguousarray(np.flip(np.transpose(x, perm + (3,)), [a for a in range(3) if flip[a]]))
    out['numpy_transpose_flip_ms'] = 1e3 * (time.perf_counter() - t0)
    try:
        from scipy import ndimage
    except ImportError:
        return out
    m = oblique()
    for order in (0, 1, 3):
        t0 = time.perf_counter()
        for c in range(x.shape[-1]):
            ndimage.affine_transform(x[..., c], m[:, :3], offset=m[:, 3], output_shape=SHAPE, order=order, mode='reflect')
        out['scipy_affine_transform_order%d_ms' % order] = 1e3 * (time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--host', action='store_true', help='time numpy / SciPy on the host and nothing else')
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    xn = rng.uniform(0.0, 1000.0, SHAPE + (C,)).astype(np.float32)
    if args.host:
        print(json.dumps({'shape': SHAPE + (C,), 'host': host(xn)}))
        return
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.from_numpy(xn).cuda()
    nbytes = 2 * x.numel() * 4
    res = {'shape': SHAPE + (C,), 'min_bytes': nbytes, 'runs': args.runs}

    def entry(ms, best):
        return {'ms': round(ms, 4), 'best_ms': round(best, 4), 'TBps': round(nbytes / (ms * 1e-3) / 1e12, 3),
                'of_copy': round(nbytes / (ms * 1e-3) / COPY_RATE, 3)}

    out = torch.empty_like(x)
    res['torch_copy'] = entry(*timed(lambda: out.copy_(x), args.runs, args.warmup))
    for name, (perm, flip) in (('reorient_transposing', TRANSPOSING), ('reorient_flips_only', FLIPS_ONLY)):
        dst = torch.empty(tuple(x.shape[p] for p in perm) + (C,), dtype=torch.float32, device=x.device)
        res[name] = entry(*timed(lambda: ops.reorient3d(x, perm, flip, out=dst), args.runs, args.warmup))
    coef = torch.empty_like(x)
    res['prefilter'] = entry(*timed(lambda: ops.spline_prefilter3d(x, out=coef), args.runs, args.warmup))
    m = oblique()
    for order in (0, 1, 3):
        src = coef if order == 3 else x
        res['affine_order%d' % order] = entry(*timed(lambda: ops.affine_resample3d(src, m, SHAPE, order=order, out=out), args.runs, args.warmup))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
