"""Times the class-location table of one example (csrc/sampling.hip: bts_class_locations through ops.class_locations) on a 240x240x155
label volume against the two things it stands between, on one GPU.  Prints one JSON line.

    python scripts/bench_sampling.py [--runs 20] [--inner 50] [--warmup 3] [--samples 10000]

Labels: three nested spheres (labels 1, 2, 3 from the outside in, radii 36, 24 and 12 voxels) off the centre of a background volume, the
shape of data.synthetic_batch's labels; V = 240*240*155 voxels, out_ch = 3.
  table     ops.class_locations(y, 3, K): three launches, the volume read twice (8 V bytes), at most 3 K ints stored
  copy      a device-to-device copy of the same 4 V bytes (torch's copy_: 4 V read + 4 V written, 8 V bytes moved)
  build     what the dataset pays once per file: the table and its two copies to the host, by the host's clock around a synchronise
  host      np.flatnonzero(y == c + 1)[::s_c] per class on the host array: what the kernel replaces
Device times are HIP events around `--inner` back-to-back calls on the launch stream, per call, median of `--runs` windows after
`--warmup`; table and copy take turns window by window.  `enqueue_us` is the host's time to enqueue one call: a `us` no larger than
that is bound by the launches, not by the kernel.  `TBps` counts the bytes above.  `volume_rate_vs_copy` = copy us / table us: the
volumes per second of the table over those of the copy.  The table reads the volume twice where the copy reads and writes it once, so by
bytes the two move the same 8 V and a ratio near 1 means both run at the streaming rate; near one half would mean that a read pass costs
what a whole copy does.
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

DIMS, OUT_CH = (240, 240, 155), 3
RADII, CENTRE = (36.0, 24.0, 12.0), (130.0, 100.0, 85.0)


def labels():
    zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in DIMS], indexing='ij')
    r2 = (zz - CENTRE[0]) ** 2 + (yy - CENTRE[1]) ** 2 + (xx - CENTRE[2]) ** 2
    lab = np.zeros(DIMS, np.float32)
    for k, r in enumerate(RADII):
        lab[r2 <= r * r] = k + 1
    return lab


def host_table(y, k):
    out = []
    flat = y.ravel()
    for c in range(OUT_CH):
        idx = np.flatnonzero(flat == c + 1)
        out.append(idx[::max(1, -(-idx.size // k))])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--samples', type=int, default=10000)
    args = ap.parse_args()
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/bench_sampling.py needs a GPU: a host timing says nothing about this kernel')
    dev = torch.device('cuda', 0)
    yh = labels()
    v = yh.size
    y = torch.from_numpy(yh).to(dev)
    dst = torch.empty_like(y)
    k = args.samples
    # the result first: the timed kernel computes what the host does
    counts, loc = ops.class_locations(y, OUT_CH, k)
    want = host_table(yh, k)
    loc_h = loc.cpu().numpy()
    for c in range(OUT_CH):
        assert np.array_equal(loc_h[c, :want[c].size], want[c]) and bool((loc_h[c, want[c].size:] == -1).all())
    calls = {'table': lambda: ops.class_locations(y, OUT_CH, k), 'copy': lambda: dst.copy_(y)}
    nbytes = {'table': 8 * v, 'copy': 8 * v}
    for fn in calls.values():
        for _ in range(args.warmup * args.inner):
            fn()
    torch.cuda.synchronize()
    us, enq = {n: [] for n in calls}, {n: [] for n in calls}
    for _ in range(args.runs):
        for n, fn in calls.items():          # the variants take turns
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            enq[n].append(1e6 * (time.perf_counter() - t0) / args.inner)
            b.synchronize()
            us[n].append(1e3 * a.elapsed_time(b) / args.inner)
    res = {'dims': DIMS, 'voxels': v, 'out_ch': OUT_CH, 'samples': k, 'counts': counts.cpu().tolist(), 'runs': args.runs, 'inner': args.inner}
    for n in calls:
        med = statistics.median(us[n])
        res[n] = {'us': round(med, 2), 'best_us': round(min(us[n]), 2), 'enqueue_us': round(statistics.median(enq[n]), 2),
                  'bytes': nbytes[n], 'TBps': round(nbytes[n] / (med * 1e-6) / 1e12, 3)}
    res['volume_rate_vs_copy'] = round(res['copy']['us'] / res['table']['us'], 3)
    build = []
    for _ in range(args.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c, t = ops.class_locations(y, OUT_CH, k)
        c.cpu().tolist(), t.cpu().numpy()
        build.append(1e3 * (time.perf_counter() - t0))
    res['build_ms'] = round(statistics.median(build), 3)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        host_table(yh, k)
        host.append(1e3 * (time.perf_counter() - t0))
    res['host_flatnonzero_ms'] = round(statistics.median(host), 2)
    res['host_over_build'] = round(res['host_flatnonzero_ms'] / res['build_ms'], 1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
