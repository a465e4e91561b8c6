"""Times the three kernels of csrc/ensemble.hip at 160x192x160 voxels x 3 channels, each against a device-to-device copy that moves the
same number of bytes, on one GPU.  Prints one JSON line.

    python scripts/bench_ensemble.py [--runs 20] [--inner 50] [--warmup 3]

With V = 160*192*160 voxels and n = 3 V floats:
  update        ops.ensemble_update(p, mean, m2, 2): p, mean and m2 read, mean and m2 written, 20 n bytes
  update_mean   ops.ensemble_update(p, mean, None, 2), what entropy mode runs: 12 n bytes
  entropy       ops.uncertainty_finish(mean, bmask, 'entropy'): the mean and the mask read, the levels written, 4 n + 4 V + n bytes
  std           ops.uncertainty_finish(mean, bmask, 'std', spread=m2, scale=1/5): the same bytes
  table         ops.uncertainty_confusion(truth, pred, unc, masks, mask): four uint8 maps read, 3 V + 3 V bytes (the table itself is 9.7 kB)
  copy_<name>   torch's copy_ of a uint8 buffer of half that many bytes: as many read as written, the same total
Device times are HIP events around `--inner` back-to-back calls on the launch stream, per call, median of `--runs` windows after
`--warmup`; a kernel and its copy take turns window by window.  `enqueue_us` is the host's time to enqueue one call: a `us` no larger
than that is bound by the launches, not by the kernel.  `vs_copy` = copy us / kernel us: 1 means the kernel moves its bytes as fast as
the copy moves the same number.  The inputs are what a scan gives: probabilities near 0 over most of the volume and a blob of uncertain
voxels, labels 0 outside nested spheres."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

DIMS, C, MEMBERS = (160, 192, 160), 3, 5
REGION_MASKS = [14, 10, 8]


def inputs(seed=0):
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(n, dtype=np.float32) for n in DIMS], indexing='ij')
    r = np.sqrt((zz - 90.0) ** 2 + (yy - 100.0) ** 2 + (xx - 70.0) ** 2)
    truth = np.zeros(DIMS, np.uint8)
    for lab, rad in ((2, 40.0), (1, 28.0), (4, 14.0)):
        truth[r <= rad] = lab
    pred = np.zeros(DIMS, np.uint8)
    for lab, rad in ((2, 43.0), (1, 25.0), (4, 15.0)):
        pred[r <= rad] = lab
    brain = (np.sqrt((zz - 80.0) ** 2 + (yy - 96.0) ** 2 + (xx - 80.0) ** 2) <= 75.0)
    soft = 1.0 / (1.0 + np.exp((r[..., None] - np.array([42.0, 27.0, 14.5], np.float32)) / 3.0))
    p = np.clip(soft + 0.02 * rng.standard_normal(soft.shape), 0.0, 1.0).astype(np.float32)
    q = np.clip(soft + 0.05 * rng.standard_normal(soft.shape), 0.0, 1.0).astype(np.float32)
    return truth, pred, brain.astype(np.uint8), p, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    import ensemble_ref as E
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/bench_ensemble.py needs a GPU: a host timing says nothing about these kernels')
    dev = torch.device('cuda', 0)
    truth_h, pred_h, brain_h, p_h, q_h = inputs()
    v, n = truth_h.size, p_h.size
    truth, pred, brain = (torch.from_numpy(a).to(dev) for a in (truth_h, pred_h, brain_h))
    bmask = brain.to(torch.float32).reshape(DIMS + (1,)).contiguous()
    p, q = torch.from_numpy(p_h).to(dev), torch.from_numpy(q_h).to(dev)
    # the results first: the timed kernels compute what the restatement does
    mean, m2 = torch.empty_like(p), torch.empty_like(p)
    ops.ensemble_update(p, mean, m2, 1)
    ops.ensemble_update(q, mean, m2, 2)
    ref_mean, ref_m2 = E.welford([p_h, q_h], np.float32)
    assert np.array_equal(mean.cpu().numpy().view(np.uint32), ref_mean.view(np.uint32))
    assert np.array_equal(m2.cpu().numpy().view(np.uint32), ref_m2.view(np.uint32))
    unc = ops.uncertainty_finish(mean, bmask, 'entropy')
    scaled = E.entropy_scaled(ref_mean)
    off = unc.cpu().numpy() != E.levels(scaled, brain_h.reshape(DIMS + (1,)))
    assert not off[~E.near_half(scaled)].any()
    table = ops.uncertainty_confusion(truth, pred, unc, REGION_MASKS, mask=brain)
    assert np.array_equal(table.cpu().numpy(), E.table(truth_h, pred_h, unc.cpu().numpy(), REGION_MASKS, brain_h))
    levels = torch.empty_like(unc)
    nbytes = {'update': 20 * n, 'update_mean': 12 * n, 'entropy': 5 * n + 4 * v, 'std': 5 * n + 4 * v, 'table': 6 * v}
    calls = {'update': lambda: ops.ensemble_update(q, mean, m2, 2),
             'update_mean': lambda: ops.ensemble_update(q, mean, None, 2),
             'entropy': lambda: ops.uncertainty_finish(mean, bmask, 'entropy', out=levels),
             'std': lambda: ops.uncertainty_finish(mean, bmask, 'std', spread=m2, scale=1.0 / MEMBERS, out=levels),
             'table': lambda: ops.uncertainty_confusion(truth, pred, unc, REGION_MASKS, mask=brain, table=table)}
    pairs = {}
    for name, fn in calls.items():
        src = torch.empty(nbytes[name] // 2, dtype=torch.uint8, device=dev).zero_()
        dst = torch.empty_like(src)
        pairs[name] = (fn, lambda src=src, dst=dst: dst.copy_(src))
    res = {'dims': DIMS, 'channels': C, 'voxels': v, 'runs': args.runs, 'inner': args.inner, 'in_band_fraction': round(float(E.near_half(scaled).mean()), 5)}
    for name, both in pairs.items():
        for fn in both:
            for _ in range(args.warmup * args.inner):
                fn()
        torch.cuda.synchronize()
        us, enq = ([], []), ([], [])
        for _ in range(args.runs):
            for i, fn in enumerate(both):          # the kernel and its copy take turns
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                enq[i].append(1e6 * (time.perf_counter() - t0) / args.inner)
                b.synchronize()
                us[i].append(1e3 * a.elapsed_time(b) / args.inner)
        for i, key in enumerate((name, 'copy_' + name)):
            med = statistics.median(us[i])
            res[key] = {'us': round(med, 2), 'best_us': round(min(us[i]), 2), 'enqueue_us': round(statistics.median(enq[i]), 2),
                        'bytes': 2 * (nbytes[name] // 2), 'TBps': round(nbytes[name] / (med * 1e-6) / 1e12, 3)}
        res[name]['vs_copy'] = round(res['copy_' + name]['us'] / res[name]['us'], 3)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
