"""Measures what `python -m bts_amd.train` rests on; not a test, not part of bench.py.

    python scripts/input_rate.py [--examples 16] [--size 150,190,140,2] [--crop 128] [--batch 8] [--repeats 3] [--out FILE.json]

On one GPU, in one process, the variants alternating, each after a warm-up pass and each timed region ending in a synchronise:
  input rate   examples/s delivered by data.prepare_dataset with (resident_bytes=0, workers=0) -- the per-example path --, with
               workers=8, and by an epoch whose examples are all resident; both data formats;
  kernel time  device-event time per batch of the per-example sequence (moments + crop kernel per example, stack, and for
               channels_first the permute copy) against the one-launch kernel on resident examples;
  epoch shape  wall time of a fit() epoch of 16 training + 4 validation batches (the command's default model, bfloat16, batch 8)
               with eval_dtype None against 'bfloat16'.
Synthetic examples are written to a temporary folder and removed afterwards."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(v):
    return {'runs': [round(x, 4) for x in v], 'median': round(float(np.median(v)), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


def epoch_seconds(ds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    for x, _ in ds:
        n += x.shape[0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--examples', type=int, default=16)
    ap.add_argument('--size', type=str, default='150,190,140,2')
    ap.add_argument('--crop', type=int, default=128)
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--skip_fit', action='store_true')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args(argv)
    import bts_amd  # noqa: F401
    from bts_amd import data, ops, train
    from bts_amd.model import Model
    from bts_amd.util import DiceCoefficient, DiceVAELoss, ScheduledOptim
    size = tuple(int(s) for s in a.size.split(','))
    crop = [a.crop] * 3
    dev = torch.device('cuda', 0)
    res = {'device': torch.cuda.get_device_name(0), 'examples': a.examples, 'size': size, 'crop': crop, 'batch': a.batch,
           'repeats': a.repeats, 'host_cpus_used': len(os.sched_getaffinity(0))}
    loc = tempfile.mkdtemp(prefix='input_rate_')
    try:
        rs = np.random.RandomState(0)
        for i in range(a.examples):
            np.savez(os.path.join(loc, 'ex%02d.npz' % i), x=rs.standard_normal(size).astype(np.float32),
                     y=rs.randint(0, 4, size[:3] + (1,)).astype(np.float32))
        res['example_bytes'] = os.path.getsize(os.path.join(loc, 'ex00.npz'))
        # ---- input rate ----
        res['input_rate_examples_per_s'] = {}
        for fmt in ('channels_last', 'channels_first'):
            variants = {'per_example_inline': (0, 0), 'workers8': (0, 8), 'resident': (1 << 40, 8)}
            sets = {k: data.prepare_dataset(loc, a.batch, size, crop, 3, shuffle=True, data_format=fmt, seed=0, device=dev,
                                            resident_bytes=rb, workers=w)[0] for k, (rb, w) in variants.items()}
            for ds in sets.values():
                epoch_seconds(ds)                      # warm-up (the resident set fills here)
            rates = {k: [] for k in sets}
            for _ in range(a.repeats):
                for k, ds in sets.items():
                    dt, n = epoch_seconds(ds)
                    rates[k].append(n / dt)
            res['input_rate_examples_per_s'][fmt] = {k: spread(v) for k, v in rates.items()}
            resident = sets['resident']
            # ---- kernel time per batch (device events) ----
            ex = [resident._resident[i] for i in range(a.batch)]
            gen = torch.Generator().manual_seed(1)
            draws = [data.draw(gen, size[3], size[:3], crop) for _ in ex]

            def old():
                per = [data.augment_example(e[0], e[1], crop, 3, d) for e, d in zip(ex, draws)]
                xs, ys = torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])
                if fmt == 'channels_first':
                    xs, ys = xs.permute(0, 4, 1, 2, 3).contiguous(), ys.permute(0, 4, 1, 2, 3).contiguous()
                return xs, ys

            def new():
                return ops.augment_batch([e[0] for e in ex], [e[1] for e in ex], [e[2] for e in ex], crop, [d.offsets for d in draws],
                                         [d.flip_mask for d in draws], [d.shift for d in draws], [d.scale for d in draws], 3,
                                         fmt == 'channels_first')
            assert all(torch.equal(p, q) for p, q in zip(old(), new()))
            ms = {'per_example_sequence': [], 'one_launch': []}
            for _ in range(a.repeats + 1):
                for k, fn in (('per_example_sequence', old), ('one_launch', new)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms[k].append(e0.elapsed_time(e1))
            res.setdefault('kernel_ms_per_batch', {})[fmt] = {k: spread(v[1:]) for k, v in ms.items()}        # (first pass: warm-up)
            out_bytes = a.batch * a.crop ** 3 * (size[3] + 3) * 4
            in_bytes = a.batch * a.crop ** 3 * (size[3] + 1) * 4
            res['kernel_ms_per_batch'][fmt]['one_launch_GBps'] = round((in_bytes + out_bytes) / (np.median(ms['one_launch'][1:]) * 1e-3) / 1e9, 1)
            if fmt == 'channels_first':
                batches = [b for b in resident][:2]
            del sets, resident, ex
            torch.cuda.empty_cache()
        # ---- epoch shape ----
        if not a.skip_fit:
            margs = dict(data_format='channels_first', base_filters=32, depth=4, l2_scale=1e-5, dropout=0.2, groups=8, reduction=8,
                         downsampling='conv', upsampling='conv', out_ch=3, in_ch=size[3])
            model = Model(**margs)
            model.build((1,) + tuple(crop) + (size[3],))
            opt = ScheduledOptim(learning_rate=1e-4)
            lf, df = DiceVAELoss(data_format='channels_first'), DiceCoefficient(data_format='channels_first')
            tr, va = [batches[i % 2] for i in range(16)], [batches[i % 2] for i in range(4)]
            secs = {'eval_float32': [], 'eval_bfloat16': []}
            epoch = 0
            for r in range(a.repeats + 1):
                for k, ed in (('eval_float32', None), ('eval_bfloat16', 'bfloat16')):
                    model.epoch.assign(epoch)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    train.fit(model, opt, lf, df, tr, va, n_epochs=epoch + 1, patience=-1, log=lambda s: None, compute_dtype='bfloat16',
                              eval_dtype=ed)
                    torch.cuda.synchronize()
                    secs[k].append(time.perf_counter() - t0)
                    epoch += 1
            res['fit_epoch_seconds_16_train_4_val'] = {k: spread(v[1:]) for k, v in secs.items()}
            res['peak_allocated_GB'] = round(torch.cuda.max_memory_allocated() / 1e9, 1)
    finally:
        shutil.rmtree(loc, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
