"""Times the device-side resampling of a full-size scan (155x190x147x4, pixdim (1.2, 0.9, 1.5) -> 186x171x220, padded to 16) and the
way back, next to the 8-flip fp16 TTA forward it feeds, in one process.  Prints one JSON line.

    python scripts/bench_resample.py [--runs 20] [--warmup 3] [--no-host]

Times are HIP events on the launch stream, median of --runs after --warmup.  `min_bytes` is input once + output once; `of_hbm_peak`
relates the achieved rate to 8 TB/s.  The host baseline is scipy.ndimage.zoom per channel on the same volume when SciPy is importable,
else the figure measured on the CPU-only build box (4 x 2.3 s) is quoted and labelled.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--no-tta', action='store_true')
    args = ap.parse_args()
    import numpy as np
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import infer, ops
    from bts_amd.model import Model
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(0)
    vol, C, pixdim, res = (155, 190, 147), 4, (1.2, 0.9, 1.5), 16
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(vol + (C,), generator=g) * 1000.0 * (torch.rand(vol + (1,), generator=g) > 0.3)).to(dev)
    shape = infer.zoom_output_shape(vol, pixdim)
    padded = tuple(s + res - s % res for s in shape)
    coef = torch.empty_like(x)
    out = {'volume': list(vol) + [C], 'pixdim': list(pixdim), 'resampled': list(shape), 'padded': list(padded), 'runs': args.runs}

    def rate(nbytes, ms):
        return {'ms': round(ms, 4), 'min_bytes': nbytes, 'GBps': round(nbytes / ms / 1e6, 1), 'of_hbm_peak': round(nbytes / ms / 1e-3 / HBM_PEAK, 4)}

    ms, best = timed(lambda: ops.spline_prefilter3d(x, out=coef), args.runs, args.warmup)
    out['prefilter'] = dict(rate(2 * x.numel() * 4, ms), best_ms=round(best, 4))
    ms, best = timed(lambda: ops.zoom3d(coef, shape, order=3, pad_to=padded, want_mask=True), args.runs, args.warmup)
    nout = padded[0] * padded[1] * padded[2]
    out['zoom_mask_pad'] = dict(rate(x.numel() * 4 + nout * (C + 1) * 4, ms), best_ms=round(best, 4))
    it = infer.Interpolator(None, order=3)
    ms, best = timed(lambda: it.resample(x, pixdim, pad_res=res), args.runs, args.warmup)
    out['resample_ms'] = round(ms, 4)
    prob = torch.rand(shape + (3,), generator=g).to(dev)
    bm = (torch.rand(shape + (1,), generator=g) > 0.3).float().to(dev)
    ms, best = timed(lambda: it.reverse(prob, mask=bm), args.runs, args.warmup)
    nnat = vol[0] * vol[1] * vol[2]
    out['reverse'] = dict(rate((prob.numel() + bm.numel()) * 4 + nnat * (3 * 4 + 1), ms), best_ms=round(best, 4))
    out['resample_plus_reverse_ms'] = round(out['resample_ms'] + out['reverse']['ms'], 4)

    if not args.no_tta:
        model = Model(base_filters=32, reduction=8, depth=4, groups=8)
        model.build((1, 128, 128, 128, 2))
        tshape = (160, 192, 160)
        xt = torch.randn(tshape + (2,), generator=g).to(dev)
        mt = torch.ones(tshape + (1,), device=dev)
        tta = infer.TestTimeAugmentor(torch.zeros(2), torch.ones(2), model, 'channels_last', compute_dtype='float16')
        ms, best = timed(lambda: tta(xt, mt), max(5, args.runs // 2), 2)
        out['tta_fp16_8flip'] = {'ms': round(ms, 3), 'best_ms': round(best, 3), 'shape': list(tshape) + [2]}
        out['tta_over_resample_plus_reverse'] = round(ms / out['resample_plus_reverse_ms'], 1)
        out['done'] = bool(out['resample_plus_reverse_ms'] < ms)

    host = {'seconds': 4 * 2.3, 'where': 'quoted: per-channel scipy.ndimage.zoom measured on the CPU-only build box'}
    if not args.no_host:
        try:
            from scipy.ndimage import zoom
            xc = x.cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            for c in range(C):
                zoom(xc[..., c], pixdim, order=3, mode='reflect')
            host = {'seconds': round(time.perf_counter() - t0, 2), 'where': 'measured in this run: per-channel scipy.ndimage.zoom, float64'}
        except ImportError:
            pass
    out['host_baseline'] = host
    out['host_over_device_resample'] = round(host['seconds'] * 1e3 / out['resample_ms'], 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
