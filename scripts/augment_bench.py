"""Times the training augmentation launches; not a test, not part of bench.py.

    python scripts/augment_bench.py [--batch 8] [--crop 128] [--size 240,240,155,2] [--sources 16] [--iters 40] [--out FILE.json]

On one GPU, with HIP events after a warm-up, the variants alternating block by block (8 launches between two events):
  copy      bts_augment_batch: crop + flips + intensity + one-hot (what every batch costs without a spatial transform);
  affine    bts_augment_spatial_batch, every example rotated (up to 15 degrees per axis) and zoomed (0.9..1.1);
  elastic   the same with a free-form field of sigma 4 at spacing 32 on top.
Every launch takes fresh draws and other resident sources (`--sources` volumes, more than the Infinity Cache holds), launches follow
each other on one stream without a host synchronise in between, as the batches of a training epoch do.  Bytes: what a launch must move
at the least -- it writes the batch (x and one-hot y) once and reads the source voxels of the crops (x and labels) once -- over the
device time, against the 6.29 TB/s a float4 copy reaches on this device.  Also the host time of ONE example through the scipy
restatement (tests/spatial_ref.py coordinates + scipy.ndimage.map_coordinates), which is what the device pass replaces."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

COPY_PEAK = 6.29e12         # bytes/s of a float4 copy on the MI355X
STEP_MS = 68.4              # the bf16 batch-8 training step the launch runs in series with


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--crop', type=int, default=128)
    ap.add_argument('--size', type=str, default='240,240,155,2')
    ap.add_argument('--sources', type=int, default=16)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out_ch', type=int, default=3)
    ap.add_argument('--skip_host', action='store_true')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args(argv)
    import bts_amd  # noqa: F401
    from bts_amd import data, ops
    import spatial_ref as SR
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/augment_bench.py measures device time: it needs the GPU')
    dev = torch.device('cuda', 0)
    h, w, d, c = (int(s) for s in a.size.split(','))
    crop = (a.crop,) * 3
    g = torch.Generator(device=dev).manual_seed(0)
    xs = [torch.randn((h, w, d, c), device=dev, generator=g) * 30 + 20 for _ in range(a.sources)]
    ys = [torch.randint(0, a.out_ch + 1, (h, w, d, 1), device=dev, generator=g).float() for _ in range(a.sources)]
    var = [ops.channel_moments(x)[1] for x in xs]
    gen = torch.Generator().manual_seed(1)
    cfgs = {'affine': data.SpatialConfig(1.0), 'elastic': data.SpatialConfig(1.0, elastic_sigma=4.0, elastic_spacing=32)}
    rounds = []
    for it in range(a.iters + 3):
        pick = [(it * a.batch + i) % a.sources for i in range(a.batch)]
        dr = [data.draw(gen, c, (h, w, d), crop) for _ in pick]
        sd = {k: [data.draw_spatial(gen, cfg, crop) for _ in pick] for k, cfg in cfgs.items()}
        phis = [s.phi.to(dev) for s in sd['elastic']]
        rounds.append((pick, dr, sd, phis))
    out = (torch.empty((a.batch, c) + crop, device=dev), torch.empty((a.batch, a.out_ch) + crop, device=dev))

    def launch(kind, r):
        pick, dr, sd, phis = r
        base = ([xs[i] for i in pick], [ys[i] for i in pick], [var[i] for i in pick], crop, [q.offsets for q in dr],
                [q.flip_mask for q in dr], [q.shift for q in dr], [q.scale for q in dr], a.out_ch)
        if kind == 'copy':
            return ops.augment_batch(*base, channels_first=True, out=out)
        s = sd[kind]
        return ops.augment_spatial_batch(*base, [q.on for q in s], [q.matrix.reshape(-1).tolist() for q in s],
                                         phis if kind == 'elastic' else [None] * len(s), [q.spacing for q in s], channels_first=True, out=out)
    kinds = ('copy', 'affine', 'elastic')
    for r in rounds[:3]:
        for k in kinds:
            launch(k, r)
    torch.cuda.synchronize()
    # A block = `block` launches of one kind between two events.  A filler of large copies goes first, so that the host has enqueued
    # the whole block before the device reaches it: the events then bracket device time alone, launches back to back.
    fill_a, fill_b = torch.empty(1 << 28, device=dev), torch.zeros(1 << 28, device=dev)
    block = 8
    times = {k: [] for k in kinds}
    timed = rounds[3:]
    for b0 in range(0, len(timed) - block + 1, block):
        for k in kinds:
            for _ in range(24):
                fill_a.copy_(fill_b)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for r in timed[b0:b0 + block]:
                launch(k, r)
            e1.record()
            times[k].append((e0, e1))
    torch.cuda.synchronize()
    nvox = a.batch * a.crop ** 3
    nbytes = nvox * 4 * (c + a.out_ch) + nvox * 4 * (c + 1)
    res = {'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'crop': crop, 'size': (h, w, d, c), 'sources': a.sources,
           'iters': a.iters, 'launches_per_block': block, 'layout': 'channels_first', 'least_bytes_per_launch': nbytes, 'step_ms': STEP_MS}
    for k in kinds:
        ms = sorted(e0.elapsed_time(e1) / block for e0, e1 in times[k])        # per launch, one value per block
        med = float(np.median(ms))
        res[k] = {'median_ms': round(med, 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4),
                  'share_of_copy_peak': round(nbytes / (med * 1e-3) / COPY_PEAK, 4), 'share_of_step': round(med / STEP_MS, 5)}
    if not a.skip_host:
        from scipy import ndimage
        pick, dr, sd, _ = rounds[0]
        x, y = xs[pick[0]].cpu().numpy().astype(np.float64), ys[pick[0]].cpu().numpy()[..., 0].astype(np.float64)
        s = sd['elastic'][0]
        t0 = time.perf_counter()
        co = np.moveaxis(SR.coordinates(crop, dr[0].offsets, s.matrix, s.phi.numpy(), s.spacing), -1, 0)
        for k in range(c):
            ndimage.map_coordinates(x[..., k], co, order=1, mode='grid-constant', cval=0.0)
        ndimage.map_coordinates(y, co, order=0, mode='grid-constant', cval=0.0)
        res['host_scipy_one_example_s'] = round(time.perf_counter() - t0, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return res


if __name__ == '__main__':
    main()
