"""Times the three preprocessing kernels of csrc/prepro.hip at 240x240x155x4 (a BraTS scan, four modalities) and, with --dataset N, the
wall time of bts_amd.preprocess.preprocess() on N synthetic cases of that size.  Prints one JSON line.

    python scripts/bench_prepro.py [--runs 20] [--warmup 3] [--dataset 16] [--workers 8] [--tmp DIR]

Kernel times are HIP events on the launch stream, median of --runs after --warmup.  Every run takes the next of 4 resident volumes
(4 x 143 MB), so no run finds its input in the 256 MB Infinity Cache the run before left behind.  `min_bytes` is what the pass must
move: the input once, for crop_norm also the output once; `of_achievable` relates the rate to the 6.3 TB/s DESIGN.md gives as the
achievable HBM streaming rate.  Windows: `dense` is the whole volume, `crop` the box [40:200, 30:220, 5:150] (its rows start 16-byte
aligned with C = 4; `crop_c3` is a three-channel volume with an odd origin, whose rows do not).

The dataset is written first and is not part of the timing: smooth tissue inside an ellipsoid, zero outside, int16, gzip level 1.
The phases of preprocess() are timed from outside (class Phases): waiting for the decode threads, upload and layout, the kernel
calls, reading the examples back and writing them.
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE = 6.3e12
VOL = (240, 240, 155)


def timed(fn, runs, warmup):
    import torch
    for k in range(warmup):
        fn(k)
    torch.cuda.synchronize()
    ms = []
    for k in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(k)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def rate(nbytes, ms, best):
    return {'ms': round(ms, 4), 'best_ms': round(best, 4), 'min_bytes': nbytes, 'GBps': round(nbytes / ms / 1e6, 1),
            'of_achievable': round(nbytes / ms / 1e-3 / ACHIEVABLE, 3)}


def kernels(args, out):
    import torch
    from bts_amd import ops
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(7)
    for c, cut, tag in ((4, None, 'dense'), (4, (slice(40, 200), slice(30, 220), slice(5, 150)), 'crop'),
                        (3, (slice(41, 200), slice(31, 220), slice(5, 150)), 'crop_c3')):
        vols = []
        for _ in range(4):
            x = torch.randint(0, 900, VOL + (c,), generator=g, dtype=torch.int16).float()
            x *= (torch.rand(VOL + (1,), generator=g) > 0.3)
            vols.append(x.to(dev))
        ys = [torch.randint(0, 5, VOL + (1,), generator=g, dtype=torch.int16).float().to(dev) for _ in range(4)]
        views = [(x, y) if cut is None else (x[cut], y[cut]) for x, y in zip(vols, ys)]
        nvox = views[0][0].numel() // c
        mean = torch.full((c,), 450.0, dtype=torch.float64, device=dev)
        std = torch.full((c,), 600.0, dtype=torch.float64, device=dev)
        acc = torch.zeros(2 * c, dtype=torch.float64, device=dev)
        acc1 = torch.zeros(c, dtype=torch.float64, device=dev)
        if cut is None:
            occ = torch.zeros(sum(VOL), dtype=torch.int32, device=dev)
            ms, best = timed(lambda k: ops.prepro_occupancy(vols[k % 4], occ), args.runs, args.warmup)
            out['occupancy_' + tag] = rate(nvox * c * 4, ms, best)
        ms, best = timed(lambda k: ops.prepro_sums(views[k % 4][0], acc), args.runs, args.warmup)
        out['sums_first_' + tag] = rate(nvox * c * 4, ms, best)
        ms, best = timed(lambda k: ops.prepro_sums(views[k % 4][0], acc1, mean=mean), args.runs, args.warmup)
        out['sums_second_' + tag] = rate(nvox * c * 4, ms, best)
        ms, best = timed(lambda k: ops.prepro_crop_norm(views[k % 4][0], views[k % 4][1], mean, std), args.runs, args.warmup)
        out['crop_norm_' + tag] = rate(nvox * (c + 1) * 4 * 2, ms, best)
        del vols, ys, views
        torch.cuda.empty_cache()


def write_dataset(root, n, modalities):
    """n case folders under root; four distinct cases are computed, the rest are copies (decoding costs the same)"""
    import numpy as np
    from bts_amd import nifti
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, s, dtype=np.float32) for s in VOL], indexing='ij')
    inside = (g[0] / 0.70) ** 2 + (g[1] / 0.80) ** 2 + (g[2] / 0.85) ** 2 < 1.0
    raw = os.path.join(root, 'raw.nii')
    for k in range(min(n, 4)):
        d = os.path.join(root, 'scans', 'case_%03d' % k)
        os.makedirs(d)
        tex = 0.6 + 0.4 * np.sin((5.0 + k) * g[0] + 1.0) * np.cos(4.0 * g[1] + k) * np.sin(6.0 * g[2] + 0.5)
        vols = [(np.where(inside, tex * a, 0.0)).astype(np.int16) for a in (900.0, 700.0, 500.0, 800.0)[:len(modalities)]]
        vols.append((np.where(inside & (tex > 0.8), 4, np.where(inside & (tex > 0.7), 2, 0))).astype(np.int16))
        for name, v in zip(list(modalities) + ['seg'], vols):
            nifti.save(raw, v, np.eye(4))
            with open(raw, 'rb') as f, open(os.path.join(d, 'case_%03d_%s.nii.gz' % (k, name)), 'wb') as o:
                o.write(gzip.compress(f.read(), 1))
    os.remove(raw)
    for k in range(4, n):
        src, dst = os.path.join(root, 'scans', 'case_%03d' % (k % 4)), os.path.join(root, 'scans', 'case_%03d' % k)
        os.makedirs(dst)
        for f in os.listdir(src):
            shutil.copy(os.path.join(src, f), os.path.join(dst, f.replace('case_%03d' % (k % 4), 'case_%03d' % k)))
    return os.path.join(root, 'scans')


class Phases:
    """Wall time spent inside chosen functions of bts_amd.preprocess, measured from outside: each is replaced by a wrapper for the
    length of the run, the module itself carries no timers.  With sync=True the device is drained before and after the call, so
    the time is that of the call's own device work; this serialises the run a little (reported as wall_s all the same).  Decoding
    runs on the pool's threads: its seconds add up over threads, the main thread's share is what is left of create_dataset."""

    def __init__(self, module):
        import threading
        self.module, self.saved, self.s, self.lock = module, {}, {}, threading.Lock()

    def wrap(self, name, sync=False):
        import torch
        fn = getattr(self.module, name)
        self.saved[name], self.s[name] = fn, 0.0

        def timed_call(*a, **k):
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            if sync:
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            with self.lock:
                self.s[name] += dt
            return r
        setattr(self.module, name, timed_call)

    def restore(self):
        for name, fn in self.saved.items():
            setattr(self.module, name, fn)


def dataset(args, out):
    import torch
    from bts_amd import ops, preprocess
    modalities = ['t1', 't1ce', 't2', 'flair']
    root = tempfile.mkdtemp(dir=args.tmp)
    ph, dv = Phases(preprocess), Phases(ops)
    try:
        t0 = time.perf_counter()
        loc = write_dataset(root, args.dataset, modalities)
        made = time.perf_counter() - t0
        nbytes = sum(os.path.getsize(os.path.join(dp, f)) for dp, _, fs in os.walk(loc) for f in fs)
        ph.wrap('_decode_case')
        ph.wrap('_upload_case', sync=True)
        ph.wrap('create_dataset')
        ph.wrap('compute_norm', sync=True)
        ph.wrap('_write')
        for k in ('prepro_occupancy', 'prepro_sums', 'prepro_crop_norm'):
            dv.wrap(k, sync=True)
        t0 = time.perf_counter()
        r = preprocess.preprocess([loc], modalities, 'seg', os.path.join(root, 'data'), create_val=True, workers=args.workers)
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
        kern = sum(dv.s.values())
        s = ph.s
        out['dataset'] = {'cases': args.dataset, 'volume': list(VOL) + [4], 'workers': args.workers, 'input_bytes': nbytes,
                          'generated_in_s': round(made, 1), 'wall_s': round(wall, 2), 'size': r['size'],
                          'n_train': r['n_train'], 'n_val': r['n_val'],
                          'create_dataset_s': round(s['create_dataset'], 2),
                          'decode_thread_s': round(s['_decode_case'], 2),
                          'waited_for_decode_s': round(s['create_dataset'] - s['_upload_case'] - dv.s['prepro_occupancy'], 2),
                          'upload_and_layout_s': round(s['_upload_case'], 2),
                          'compute_norm_s': round(s['compute_norm'], 3),
                          'write_s': round(s['_write'], 2),
                          'write_host_s': round(s['_write'] - dv.s['prepro_crop_norm'], 2),
                          'device_s': {k: round(v, 4) for k, v in dv.s.items()}, 'device_total_s': round(kern, 3)}
    finally:
        ph.restore()
        dv.restore()
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dataset', type=int, default=0)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--tmp', type=str, default=None)
    ap.add_argument('--no-kernels', action='store_true')
    args = ap.parse_args()
    import torch
    import bts_amd  # noqa: F401
    torch.cuda.set_device(0)
    out = {'volume': list(VOL) + [4], 'runs': args.runs, 'achievable_Bps': ACHIEVABLE}
    if not args.no_kernels:
        kernels(args, out)
    if args.dataset:
        dataset(args, out)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
