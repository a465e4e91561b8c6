"""Times the intensity augmentation behind the training augmentation launch; not a test, not part of bench.py.

    python scripts/augment_intensity_bench.py [--batch 8] [--crop 128] [--size 240,240,155,2] [--sources 16] [--iters 40]
                                              [--layout channels_first] [--step_ms 68.4] [--out FILE.json]

On one GPU, with HIP events after a warm-up, the variants alternating block by block (8 batches between two events), by the method of
scripts/augment_bench.py:
  copy      bts_augment_batch alone: what every batch costs without the intensity transforms (the parent's launch);
  all       that launch, then bts_intensity_batch with every stage on for every (example, channel): the worst case;
  default   that launch, then bts_intensity_batch with the draws of data.IntensityConfig()'s default probabilities.
Every batch takes fresh draws and other resident sources, batches follow each other on one stream without a host synchronise in
between.  Bytes: the least a batch's intensity transforms must move -- per (example, channel) volume, in traversals of its 4 vol bytes:
the blur reads and writes it once (noise and brightness ride along), contrast reads it once for its statistics and reads and writes it
once, gamma reads its input's statistics (free with contrast's write in front of it, one read otherwise), then twice reads and writes
(the power, the rescale; the rescale's statistics ride on the power's write) -- over the time the variant adds to `copy`, against the
6.29 TB/s a float4 copy reaches on this device; next to it the traversals the kernels of csrc/intensity.hip really make.  Also the host
time of ONE example through numpy / scipy.ndimage.gaussian_filter with every stage on, which is what the device passes replace."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK = 6.29e12         # bytes/s of a float4 copy on the MI355X
NOISE, BLUR, BRIGHT, CONTRAST, GAMMA = 1, 2, 4, 8, 16


def least_traversals(flags):
    t = 2 if flags & BLUR else 0
    if flags & CONTRAST:
        t += 3
    if flags & GAMMA:
        t += 4 if flags & CONTRAST else 5
    if flags & (NOISE | BRIGHT) and not flags & (BLUR | CONTRAST | GAMMA):
        t = 2
    return t


def made_traversals(flags):
    t = 2 if flags & NOISE else 0
    if flags & BLUR:
        t += 6
    if flags & CONTRAST:
        t += 1
    if flags & (BLUR | BRIGHT | CONTRAST):
        t += 2
    if flags & GAMMA:
        t += 6
    return t


def host_one_example(x, entry, rs):
    """every stage on, one (T0,T1,T2,C) float32 example through numpy / scipy"""
    from scipy import ndimage
    out = np.empty_like(x)
    for c in range(x.shape[-1]):
        _, s, sigma, m, f, g = entry[c]
        v = x[..., c] + np.float32(s) * rs.standard_normal(x.shape[:3]).astype(np.float32)
        v = ndimage.gaussian_filter(v, sigma)
        v = v * np.float32(m)
        mu, lo, hi = v.mean(), v.min(), v.max()
        v = np.clip((v - mu) * np.float32(f) + mu, lo, hi)
        mu, sd, lo = v.mean(), v.std(), v.min()
        R = v.max() - lo
        v = np.power((v - lo) / (R + np.float32(1e-7)), np.float32(g)) * R + lo
        out[..., c] = (v - v.mean()) / (v.std() + np.float32(1e-8)) * sd + mu
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--crop', type=int, default=128)
    ap.add_argument('--size', type=str, default='240,240,155,2')
    ap.add_argument('--sources', type=int, default=16)
    ap.add_argument('--iters', type=int, default=40)
    ap.add_argument('--out_ch', type=int, default=3)
    ap.add_argument('--layout', choices=('channels_first', 'channels_last'), default='channels_first')
    ap.add_argument('--step_ms', type=float, default=68.4, help='the bf16 batch-8 training step the launches run in series with')
    ap.add_argument('--skip_host', action='store_true')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args(argv)
    import bts_amd  # noqa: F401
    from bts_amd import data, ops
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/augment_intensity_bench.py measures device time: it needs the GPU')
    dev = torch.device('cuda', 0)
    h, w, d, c = (int(s) for s in a.size.split(','))
    crop = (a.crop,) * 3
    cf = a.layout == 'channels_first'
    g = torch.Generator(device=dev).manual_seed(0)
    # (normalised volumes: N(0,1), as the intensity ranges of the transforms assume)
    xs = [torch.randn((h, w, d, c), device=dev, generator=g) for _ in range(a.sources)]
    ys = [torch.randint(0, a.out_ch + 1, (h, w, d, 1), device=dev, generator=g).float() for _ in range(a.sources)]
    var = [ops.channel_moments(x)[1] for x in xs]
    gen = torch.Generator().manual_seed(1)
    default = data.IntensityConfig()
    every = data.IntensityConfig(noise_prob=1, blur_prob=1, blur_channel_prob=1, brightness_prob=1, contrast_prob=1, gamma_prob=1)
    rounds = []
    for it in range(a.iters + 3):
        pick = [(it * a.batch + i) % a.sources for i in range(a.batch)]
        dr = [data.draw(gen, c, (h, w, d), crop) for _ in pick]
        idr = {'all': [data.draw_intensity(gen, every, c) for _ in pick], 'default': [data.draw_intensity(gen, default, c) for _ in pick]}
        rounds.append((pick, dr, idr))
    out = (torch.empty(((a.batch, c) + crop) if cf else ((a.batch,) + crop + (c,)), device=dev),
           torch.empty(((a.batch, a.out_ch) + crop) if cf else ((a.batch,) + crop + (a.out_ch,)), device=dev))

    def launch(kind, r):
        pick, dr, idr = r
        xo, _ = ops.augment_batch([xs[i] for i in pick], [ys[i] for i in pick], [var[i] for i in pick], crop, [q.offsets for q in dr],
                                  [q.flip_mask for q in dr], [q.shift for q in dr], [q.scale for q in dr], a.out_ch, channels_first=cf,
                                  out=out)
        if kind != 'copy':
            ops.intensity_batch(xo, [q.params for q in idr[kind]], [q.key for q in idr[kind]], cf)
    kinds = ('copy', 'all', 'default')
    for r in rounds[:3]:
        for k in kinds:
            launch(k, r)
    torch.cuda.synchronize()
    # A block = `block` batches of one kind between two events.  A filler of large copies goes first, so that the host has enqueued
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
    vol_bytes = 4 * a.crop ** 3
    res = {'device': torch.cuda.get_device_name(0), 'batch': a.batch, 'crop': crop, 'size': (h, w, d, c), 'sources': a.sources,
           'iters': a.iters, 'batches_per_block': block, 'layout': a.layout, 'step_ms': a.step_ms}
    for k in kinds:
        ms = sorted(e0.elapsed_time(e1) / block for e0, e1 in times[k])        # per batch, one value per block
        res[k] = {'median_ms': round(float(np.median(ms)), 4), 'min_ms': round(ms[0], 4), 'max_ms': round(ms[-1], 4)}
    for k in kinds[1:]:
        flags = [e[0] for _, _, idr in timed for q in idr[k] for e in q.params]
        per_batch = a.batch * c / float(len(flags))
        least = sum(least_traversals(f) for f in flags) * per_batch * vol_bytes
        made = sum(made_traversals(f) for f in flags) * per_batch * vol_bytes
        added = res[k]['median_ms'] - res['copy']['median_ms']
        res[k].update({'added_ms': round(added, 4), 'share_of_step': round(added / a.step_ms, 5),
                       'volumes_with_a_flag_per_batch': round(sum(1 for f in flags if f & 31) * per_batch, 2),
                       'least_bytes_per_batch': int(least), 'bytes_moved_per_batch': int(made),
                       'share_of_copy_peak': round(least / (added * 1e-3) / COPY_PEAK, 4) if added > 0 else None,
                       'moved_share_of_copy_peak': round(made / (added * 1e-3) / COPY_PEAK, 4) if added > 0 else None})
    if not a.skip_host:
        pick, dr, idr = rounds[0]
        launch('copy', rounds[0])
        x = (out[0][0].permute(1, 2, 3, 0) if cf else out[0][0]).contiguous().cpu().numpy()
        rs = np.random.RandomState(0)
        t0 = time.perf_counter()
        host_one_example(x, idr['all'][0].params, rs)
        res['host_numpy_scipy_one_example_s'] = round(time.perf_counter() - t0, 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return res


if __name__ == '__main__':
    main()
