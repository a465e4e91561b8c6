"""Times N4 bias-field correction (csrc/n4.hip, bts_amd.n4) on one 240x240x155 volume: a whole `n4.correct` with the default spec on the
device and through the numpy evaluator of tests/n4_ref.py, and `ops.n4_apply` alone against a plain device copy of the same bytes.
Prints one JSON line.

    python scripts/bench_n4.py [--runs 50] [--warmup 5] [--corrections 5] [--no-host]

The volume is the analytic head of tests/n4_ref.py (three tissues, a smooth multiplicative field, 2 % noise) at 240x240x155; the default
spec works on a 60x60x39 lattice (shrink 4), four levels of at most 50 sweeps.  `correct_ms` is a host clock around one whole call that
ends in a device synchronise, the median of --corrections after one warm-up; it is launch- and synchronisation-bound (six launches and
two read-backs per sweep), so `ms_per_sweep` is the figure to watch.  `host_numpy_ms` is the same `n4.correct` with the numpy evaluator,
once; the two runs must take the same sweeps per level.  `apply_ms` is HIP events around one ops.n4_apply, the median of --runs after
--warmup, every run on the next of 4 resident volumes; `copy_ms` the same around out.copy_(x), which moves the same 8 bytes per voxel;
`GBps` = 8 bytes x voxels / time."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPE = (240, 240, 155)


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
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--corrections', type=int, default=5)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import n4, ops
    import n4_ref as R
    if not torch.cuda.is_available():
        raise SystemExit('bench_n4.py measures on the GPU; none is available')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    x, tissue, logb = R.phantom(SHAPE)
    xg = torch.from_numpy(x).to(dev)
    spec = n4.N4Spec()
    res = n4.correct(xg, None, spec)                         # warm-up: code objects, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(args.corrections):
        t0 = time.perf_counter()
        res = n4.correct(xg, None, spec)
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    sweeps = sum(res.sweeps)
    out = {'shape': list(SHAPE), 'spec': n4.spec_record(spec), 'lattice_points': res.points, 'sweeps': list(res.sweeps),
           'correct_ms': round(statistics.median(ts), 2), 'correct_best_ms': round(min(ts), 2), 'correct_worst_ms': round(max(ts), 2),
           'ms_per_sweep': round(statistics.median(ts) / max(sweeps, 1), 3),
           'tissue_cv_before': [round(v, 4) for v in R.tissue_cv(x, tissue)],
           'tissue_cv_after': [round(v, 4) for v in R.tissue_cv(res.out.cpu().numpy(), tissue)]}
    if not args.no_host:
        t0 = time.perf_counter()
        ref = n4.correct(x, None, spec, evaluate=R.NumpyEvaluator())
        out['host_numpy_ms'] = round(1e3 * (time.perf_counter() - t0), 1)
        out['host_sweeps'] = list(ref.sweeps)
        out['host_over_device'] = round(out['host_numpy_ms'] / out['correct_ms'], 1)
        out['max_abs_phi_diff_to_host'] = float(np.abs(ref.phi - res.phi).max()) if ref.phi.shape == res.phi.shape else None
    vols = [xg] + [torch.from_numpy(R.phantom(SHAPE, seed=k)[0]).to(dev) for k in (1, 2, 3)]
    phi = torch.from_numpy(res.phi).to(dev)
    dst = torch.empty_like(xg)
    nbytes = 8 * xg.numel()
    for name, fn in (('apply', lambda k: ops.n4_apply(vols[k % 4], phi, res.mesh)), ('copy', lambda k: dst.copy_(vols[k % 4]))):
        ms, best, worst = timed(fn, args.runs, args.warmup)
        out[name + '_ms'] = round(ms, 4)
        out[name + '_best_ms'] = round(best, 4)
        out[name + '_worst_ms'] = round(worst, 4)
        out[name + '_GBps'] = round(nbytes / ms / 1e6, 1)
    out['apply_over_copy'] = round(out['apply_ms'] / out['copy_ms'], 2)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
