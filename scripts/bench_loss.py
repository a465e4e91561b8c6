"""Times the compound loss's two streaming passes (csrc/loss_ce.hip: bts_seg_loss_sums, bts_seg_loss_bwd; gamma 0, 2 and 0.5) against the Dice
pair (csrc/loss.hip: bts_loss_sums, bts_loss_bwd) on the same buffers, on one GPU.  Prints one JSON line.

    python scripts/bench_loss.py [--runs 20] [--inner 50] [--warmup 3]

Shapes: N = 1 and N = 8 of 128^3 voxels, C = 3 output channels, Cx = 2 input channels, Lz = 128.  Every variant reads y_pred, y, x and
y_vae once (`sums`: N V (2 C + 2 Cx) floats) and the backward writes dlogit and dyvae once more (N V (C + Cx) floats): the compound
passes move the bytes of the Dice pair and add two logarithms per element (the sums; the backward at gamma 0 adds none), and two powers
at gamma > 0: products for gamma = 1, ..., 8, powf otherwise.  Times are HIP events around `--inner` back-to-back calls on the launch
stream, per call, median of `--runs` windows after `--warmup`; the variants take turns window by window.  `enqueue_us` is the host's
time to enqueue one call: a variant whose `us` is no more than that is bound by the launches, not by the kernel.  `ratio` is compound
over Dice.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS, C, CX, LZ = (128, 128, 128), 3, 2, 128
GAMMAS = (0.0, 2.0, 0.5)      # binary cross-entropy; the default focal exponent (a product); a non-integer one (powf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--inner', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    from bts_amd._lib import lib
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/bench_loss.py needs a GPU: a host timing says nothing about these kernels')
    L = lib()
    dev = torch.device('cuda', 0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {'dims': DIMS, 'C': C, 'Cx': CX, 'runs': args.runs, 'inner': args.inner, 'shapes': {}}
    for n in (1, 8):
        g = torch.Generator(device='cpu').manual_seed(n)
        v = DIMS[0] * DIMS[1] * DIMS[2]
        p = torch.sigmoid(torch.randn((n,) + DIMS + (C,), generator=g) * 2.0).to(dev)
        y = (torch.rand((n,) + DIMS + (C,), generator=g) < 0.3).float().to(dev)
        x = torch.randn((n,) + DIMS + (CX,), generator=g).to(dev)
        yv = torch.randn((n,) + DIMS + (CX,), generator=g).to(dev)
        proj = (torch.randn((n, 2 * LZ), generator=g) * 0.5).to(dev)
        dl, dyv, dpr = torch.empty_like(p), torch.empty_like(x), torch.empty_like(proj)
        one = torch.ones(1, device=dev)
        nb = max(L.query('bts_loss_workspace'), L.query('bts_seg_loss_workspace'))
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        s_dice = ops.loss_sums(p, y, x, yv, proj)
        s_seg = {gm: ops.seg_loss_sums(p, y, x, yv, proj, gm) for gm in GAMMAS}
        shape_args = (n, v, C, C, C, CX, CX, CX, LZ)
        calls = {
            'sums/dice': lambda: L.call('bts_loss_sums', P(p), P(y), P(x), P(yv), P(proj), P(s_dice), P(ws), nb, *shape_args, stream),
            'bwd/dice': lambda: L.call('bts_loss_bwd', P(p), P(y), P(x), P(yv), P(proj), P(s_dice), P(one), P(dl), P(dyv), P(dpr),
                                       *shape_args, 1, stream)}
        for gm in GAMMAS:
            calls['sums/gamma%g' % gm] = (lambda gm=gm: L.call('bts_seg_loss_sums', P(p), P(y), P(x), P(yv), P(proj), P(s_seg[gm]), P(ws), nb,
                                                               *shape_args, gm, 1.0, 1.0, stream))
            calls['bwd/gamma%g' % gm] = (lambda gm=gm: L.call('bts_seg_loss_bwd', P(p), P(y), P(x), P(yv), P(proj), P(s_seg[gm]), P(one), P(dl),
                                                              P(dyv), P(dpr), *shape_args, 1, 1.0, 1.0, gm, 1.0, 1.0, stream))
        nbytes = {'sums': n * v * (2 * C + 2 * CX) * 4, 'bwd': n * v * (3 * C + 3 * CX) * 4}
        for fn in calls.values():
            for _ in range(args.warmup * args.inner):
                fn()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        enq = {k: [] for k in calls}
        for _ in range(args.runs):
            for k, fn in calls.items():          # the variants take turns
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                for _ in range(args.inner):
                    fn()
                b.record()
                enq[k].append(1e6 * (time.perf_counter() - t0) / args.inner)
                b.synchronize()
                us[k].append(1e3 * a.elapsed_time(b) / args.inner)
        out = {}
        for k in calls:
            med = statistics.median(us[k])
            kind = k.split('/')[0]
            out[k] = {'us': round(med, 2), 'best_us': round(min(us[k]), 2), 'enqueue_us': round(statistics.median(enq[k]), 2),
                      'bytes': nbytes[kind], 'TBps': round(nbytes[kind] / (med * 1e-6) / 1e12, 3)}
        for kind in ('sums', 'bwd'):
            for gm in GAMMAS:
                k = '%s/gamma%g' % (kind, gm)
                out[k]['ratio'] = round(out[k]['us'] / out[kind + '/dice']['us'], 3)
        res['shapes']['N%d' % n] = out
    print(json.dumps(res))


if __name__ == '__main__':
    main()
