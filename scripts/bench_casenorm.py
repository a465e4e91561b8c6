"""Times ops.case_norm (csrc/casenorm.hip) on a 155x190x147x4 scan with the derived mask and on a 160x192x160x2 padded volume with an
explicit mask, with clipping off and at the percentiles (0.5, 99.5), and the same arithmetic in numpy on the host.  Prints one JSON line.

    python scripts/bench_casenorm.py [--runs 50] [--warmup 5] [--host-runs 2]

Device times are HIP events on the launch stream around one whole call (every kernel of it), the median of --runs after --warmup.  Every
run takes the next of 4 resident volumes, so no call finds its input in the 256 MB Infinity Cache the call before left behind; the
passes of one call do re-read the volume the first of them fetched, as they do in use.  `bytes` is what the passes of a call must move,
counted from the shapes: each statistics pass reads the volume (and the mask, when there is one) once -- two sum passes, and four
histogram passes more with clipping -- and the apply pass reads them once and writes the output once.  `GBps` = bytes / time;
`passes` is the number of traversals.  The host figure is numpy float64 on one volume: np.percentile, clip, two-pass mean and deviation,
the float32 result -- the arithmetic of tests/casenorm_ref.py with numpy's own percentile.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (('scan_155x190x147x4_derived_mask', (155, 190, 147), 4, False),
         ('padded_160x192x160x2_explicit_mask', (160, 192, 160), 2, True))
CLIPS = (None, (0.5, 99.5))


def pass_bytes(vol, c, masked, clip):
    """-> (bytes the passes of one call move, traversals of the volume)"""
    nvox = vol[0] * vol[1] * vol[2]
    read = nvox * 4 * (c + (1 if masked else 0))
    stat_passes = 2 + (4 if clip is not None else 0)
    return stat_passes * read + read + nvox * c * 4, stat_passes + 1


def host_case_norm(x, mask, clip):
    import numpy as np
    inside = (x > 0).any(axis=-1) if mask is None else mask.reshape(x.shape[:3]) != 0
    out = np.zeros(x.shape, dtype=np.float32)
    for ch in range(x.shape[-1]):
        v = x[..., ch][inside].astype(np.float64)
        if clip is not None:
            lo, hi = np.percentile(v, clip, method='linear')
            v = np.clip(v, lo, hi)
        mean = v.sum() / v.size
        std = np.sqrt(((v - mean) ** 2).sum() / v.size)
        out[..., ch][inside] = ((v - mean) / std).astype(np.float32)
    return out


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
    ap.add_argument('--host-runs', type=int, default=2)
    args = ap.parse_args()
    if args.runs < 50:
        ap.error('--runs: the median is taken over at least 50 calls')
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('bench_casenorm.py measures on the GPU; none is available')
    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(7)
    out = {'runs': args.runs, 'warmup': args.warmup}
    for name, vol, c, masked in CASES:
        vols, masks = [], []
        for _ in range(4):
            brain = torch.rand(vol + (1,), generator=g) > 0.4
            x = (torch.randint(1, 3000, vol + (c,), generator=g, dtype=torch.int16).float() * brain).to(dev)
            vols.append(x)
            masks.append(brain.float().to(dev) if masked else None)
        xn = torch.empty(vol + (c,), dtype=torch.float32, device=dev)
        for clip in CLIPS:
            nbytes, passes = pass_bytes(vol, c, masked, clip)
            ms, best, worst = timed(lambda k: ops.case_norm(vols[k % 4], masks[k % 4], clip, out=xn), args.runs, args.warmup)
            xh = vols[0].cpu().numpy()
            mh = None if masks[0] is None else masks[0].cpu().numpy()
            hs = []
            for _ in range(args.host_runs):
                t0 = time.perf_counter()
                ref = host_case_norm(xh, mh, clip)
                hs.append(time.perf_counter() - t0)
            got = ops.case_norm(vols[0], masks[0], clip)[0].cpu().numpy()
            worst_ulp = float(abs(got.astype('float64') - ref.astype('float64')).max())
            out['%s_clip_%s' % (name, 'off' if clip is None else '%g_%g' % clip)] = {
                'ms': round(ms, 4), 'best_ms': round(best, 4), 'worst_ms': round(worst, 4), 'passes': passes, 'bytes': nbytes,
                'GBps': round(nbytes / ms / 1e6, 1), 'host_numpy_ms': round(1e3 * min(hs), 1),
                'host_over_device': round(1e3 * min(hs) / ms, 1), 'max_abs_diff_to_host': worst_ulp}
        del vols, masks, xn
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
