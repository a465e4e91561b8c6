"""Times the three kernels of csrc/regions.hip; not a test, not part of bench.py.

    python scripts/regions_bench.py [--crop 128] [--batches 1,8] [--iters 40] [--out FILE.json]

On one GPU, with HIP events after a warm-up, the method of scripts/augment_intensity_bench.py: a block is 8 launches of one kernel
between two events, behind a filler of large copies so that the host has enqueued the whole block before the device reaches it (the
events then bracket device time alone, launches back to back); the kernels alternate block by block and a time is the median over
the blocks of (block time / 8).  Every launch of a block works on a buffer set of its own, `sets` of them in rotation, more bytes in all
than the 256 MiB last-level cache holds, so that no launch is served from it.  Per kernel and N (examples of crop^3 voxels):
  targets_last / targets_first   bts_region_targets in place, (N,V,3) / (N,3,V): reads and writes 12 bytes per voxel;
  dice_sums                      bts_region_dice_sums with the label map: reads 24, writes 1 byte per voxel (two launches: the table);
  dice_sums_no_labels            the same without the map: reads 24;
  finish                         bts_region_finish with both outputs: reads 16, writes 13 bytes per voxel;
  finish_labels                  labels only (TestTimeAugmentor.labels): reads 16, writes 1.
Bytes are the least the pass must move; the rate is those bytes over the median time, next to the 6.29 TB/s a float4 copy reaches on
this device."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK = 6.29e12         # bytes/s of a float4 copy on the MI355X
BYTES = {'targets_last': 24, 'targets_first': 24, 'dice_sums': 25, 'dice_sums_no_labels': 24, 'finish': 29, 'finish_labels': 17}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--crop', type=int, default=128)
    ap.add_argument('--batches', type=str, default='1,8')
    ap.add_argument('--iters', type=int, default=40, help='timed launches per kernel and N (a multiple of 8)')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args(argv)
    import bts_amd  # noqa: F401
    from bts_amd import ops
    if not torch.cuda.is_available():
        raise RuntimeError('scripts/regions_bench.py measures device time: it needs the GPU')
    dev = torch.device('cuda', 0)
    crop = (a.crop,) * 3
    vox = a.crop ** 3
    g = torch.Generator(device=dev).manual_seed(0)
    res = {'device': torch.cuda.get_device_name(0), 'crop': crop, 'iters': a.iters, 'launches_per_block': 8, 'copy_peak_bytes_per_s': COPY_PEAK}
    fill_a, fill_b = torch.empty(1 << 28, device=dev), torch.zeros(1 << 28, device=dev)
    for n in (int(v) for v in a.batches.split(',')):
        sets = max(2, -(-(1 << 29) // (n * vox * 24)))                     # >= 512 MiB of (y, prob) per rotation
        bufs = []
        for _ in range(sets):
            lab = torch.randint(0, 4, (n,) + crop, device=dev, generator=g)
            y = torch.stack([(lab == k).float() for k in (1, 2, 3)], dim=-1).contiguous()
            bufs.append({'y_last': y, 'y_first': y.permute(0, 4, 1, 2, 3).contiguous(), 't': ops.region_targets(y.clone()),
                         'p': torch.rand((n,) + crop + (3,), device=dev, generator=g),
                         'm': (torch.rand((n,) + crop + (1,), device=dev, generator=g) > 0.2).float()})
        kinds = {
            'targets_last': lambda b: ops.region_targets(b['y_last'], False),
            'targets_first': lambda b: ops.region_targets(b['y_first'], True),
            'dice_sums': lambda b: ops.region_dice_sums(b['t'], b['p'], True),
            'dice_sums_no_labels': lambda b: ops.region_dice_sums(b['t'], b['p'], False),
            'finish': lambda b: ops.region_finish(b['p'], b['m'], 0.5, True, True),
            'finish_labels': lambda b: ops.region_finish(b['p'], b['m'], 0.5, False, True),
        }
        for k, fn in kinds.items():                                       # warm-up: code objects, the allocator's blocks
            for b in bufs[:2]:
                fn(b)
        torch.cuda.synchronize()
        times = {k: [] for k in kinds}
        turn = 0
        for _ in range(max(1, a.iters // 8)):
            for k, fn in kinds.items():
                for _ in range(24):
                    fill_a.copy_(fill_b)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(8):
                    fn(bufs[turn % sets])
                    turn += 1
                e1.record()
                times[k].append((e0, e1))
        torch.cuda.synchronize()
        row = {'sets': sets}
        for k in kinds:
            us = sorted(e0.elapsed_time(e1) * 1e3 / 8 for e0, e1 in times[k])
            med = float(np.median(us))
            nbytes = BYTES[k] * n * vox
            row[k] = {'median_us': round(med, 2), 'min_us': round(us[0], 2), 'max_us': round(us[-1], 2), 'bytes': nbytes,
                      'bytes_per_s': round(nbytes / (med * 1e-6), 0), 'share_of_copy_peak': round(nbytes / (med * 1e-6) / COPY_PEAK, 4)}
        res['N=%d' % n] = row
        del bufs
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(json.dumps(res, indent=1) + '\n')
    return res


if __name__ == '__main__':
    main()
