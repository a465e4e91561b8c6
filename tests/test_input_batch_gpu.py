"""-m gpu: the batched augmentation kernel (bts_augment_batch) and the dataset behind data.prepare_dataset that uses it.

Kernel: torch.equal to the per-example path (data.augment_example per example, torch.stack, and for the channels-first layout
.permute(0,4,1,2,3).contiguous()), and the yardstick of tests/test_data_gpu.py against the oracle's restatement of train.py:14-49:
labels exact, intensities within 1e-5 * max|x|.  Dataset: for a seed the batches do not depend on resident_bytes / workers."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402


def dev():
    return torch.device('cuda', 0)


# (flip mask, corner): bit k of `corner` puts axis k's offset at the top of its range, else at 0 -- all 8 masks twice, and both ends
# of every axis' range under flipped and unflipped rows; draws from data.draw supply shifts, scales and three interior windows
PINS = [(m, m ^ (0 if r == 0 else 7)) for r in (0, 1) for m in range(8)]
FREE = 3

# volume, C, crop, out_ch, N (None: one more than a launch carries)
CASES = [((9, 10, 11), 2, (8, 8, 8), 3, 3),          # odd row starts, 8-byte alignment only
         ((16, 12, 20), 4, (16, 8, 16), 1, 2),       # four channels
         ((7, 9, 13), 3, (4, 6, 5), 3, 5),           # odd channel count, odd T2 under an axis-2 flip
         ((5, 5, 5), 1, (5, 5, 5), 3, 1),            # crop = volume
         ((6, 6, 10), 2, (4, 4, 8), 2, None)]        # split into two launches


def _draws(data, c, vol, crop, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for mask, corner in PINS:
        d = data.draw(gen, c, vol, crop)
        d.offsets = [(vol[k] - crop[k]) if (corner >> k) & 1 else 0 for k in range(3)]
        d.flips = [bool(mask & 4), bool(mask & 2), bool(mask & 1)]
        out.append(d)
    out += [data.draw(gen, c, vol, crop) for _ in range(FREE)]
    assert {d.flip_mask for d in out[:16]} == set(range(8))
    return out


def _volumes(n, vol, c, out_ch, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [(torch.randn(vol + (c,), generator=g) * 30 + 50) for _ in range(n)]
    ys = [torch.randint(0, out_ch + 1, vol + (1,), generator=g).float() for _ in range(n)]
    return xs, ys


@pytest.mark.parametrize('vol,c,crop,out_ch,n', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_batch_kernel_is_the_per_example_path_and_matches_the_oracle(vol, c, crop, out_ch, n):
    import bts_amd  # noqa: F401
    from bts_amd import data, ops
    n = ops.augment_batch_max() + 1 if n is None else n
    xs, ys = _volumes(n, vol, c, out_ch, seed=1)
    dx, dy = [x.to(dev()) for x in xs], [y.to(dev()) for y in ys]
    var = [ops.channel_moments(x)[1] for x in dx]
    draws = _draws(data, c, vol, crop, seed=2)
    nb = (len(draws) + n - 1) // n
    for b in range(nb):
        ds = [draws[(b * n + i) % len(draws)] for i in range(n)]
        per = [data.augment_example(dx[i], dy[i], crop, out_ch, ds[i]) for i in range(n)]
        want_x, want_y = torch.stack([p[0] for p in per]), torch.stack([p[1] for p in per])
        for cf in (False, True):
            gx, gy = ops.augment_batch(dx, dy, var, crop, [d.offsets for d in ds], [d.flip_mask for d in ds], [d.shift for d in ds],
                                       [d.scale for d in ds], out_ch, channels_first=cf)
            wx, wy = (want_x.permute(0, 4, 1, 2, 3).contiguous(), want_y.permute(0, 4, 1, 2, 3).contiguous()) if cf else (want_x, want_y)
            assert tuple(gx.shape) == tuple(wx.shape) and tuple(gy.shape) == tuple(wy.shape)
            assert torch.equal(gx, wx), 'x, channels_first %s, batch %d: max |d| %.3e' % (cf, b, float((gx - wx).abs().max()))
            assert torch.equal(gy, wy), 'y, channels_first %s, batch %d' % (cf, b)
        # the oracle on the same draws (tests/test_data_gpu.py's bounds)
        gx, gy = want_x.cpu().double(), want_y.cpu().double()
        got_x, got_y = ops.augment_batch(dx, dy, var, crop, [d.offsets for d in ds], [d.flip_mask for d in ds], [d.shift for d in ds],
                                         [d.scale for d in ds], out_ch)
        for i in range(n):
            xr, yr = R.augment_example(xs[i].double(), ys[i].double(), crop, out_ch, ds[i].shift, ds[i].scale, ds[i].offsets, ds[i].flips)
            assert torch.equal(got_y[i].cpu().double(), yr), 'one-hot labels must be exact'
            err = float((got_x[i].cpu().double() - xr).abs().max())
            assert err <= 1e-5 * float(xr.abs().max()), 'augmented intensities: %.3e' % err


@pytest.mark.parametrize('lead', [4, 1, 2], ids=lambda v: 'lead%d' % v)
@pytest.mark.parametrize('cf', [False, True], ids=['channels_last', 'channels_first'])
def test_nothing_outside_the_outputs_is_written(cf, lead):
    """outputs that are slices of larger sentinel-filled buffers, `lead` floats into them (16-, 4- and 8-byte aligned starts: the
    vector and the scalar stores): the slices equal the freshly allocated result, every float around them keeps the sentinel"""
    import bts_amd  # noqa: F401
    from bts_amd import data, ops
    vol, c, crop, out_ch, n = (9, 10, 12), 2, (8, 8, 8), 3, 3
    xs, ys = _volumes(n, vol, c, out_ch, seed=3)
    dx, dy = [x.to(dev()) for x in xs], [y.to(dev()) for y in ys]
    var = [ops.channel_moments(x)[1] for x in dx]
    ds = _draws(data, c, vol, crop, seed=4)[5:5 + n]
    a = ([d.offsets for d in ds], [d.flip_mask for d in ds], [d.shift for d in ds], [d.scale for d in ds], out_ch)
    want_x, want_y = ops.augment_batch(dx, dy, var, crop, *a, channels_first=cf)
    tail, sentinel = 37, -777.0
    bx = torch.full((lead + want_x.numel() + tail,), sentinel, device=dev())
    by = torch.full((lead + want_y.numel() + tail,), sentinel, device=dev())
    ox = bx[lead:lead + want_x.numel()].view(want_x.shape)
    oy = by[lead:lead + want_y.numel()].view(want_y.shape)
    ops.augment_batch(dx, dy, var, crop, *a, channels_first=cf, out=(ox, oy))
    torch.cuda.synchronize()
    assert torch.equal(ox, want_x) and torch.equal(oy, want_y)
    for buf, size in ((bx, want_x.numel()), (by, want_y.numel())):
        assert bool((buf[:lead] == sentinel).all()) and bool((buf[lead + size:] == sentinel).all())


# ---- the dataset ----------------------------------------------------------------------------------------------------------------
SIZE, CROP = (10, 12, 9, 2), (8, 8, 8)
EXAMPLE_BYTES = (10 * 12 * 9 * 2 + 10 * 12 * 9) * 4


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    loc = str(tmp_path_factory.mktemp('examples'))
    rs = np.random.RandomState(0)
    for i in range(5):
        np.savez(os.path.join(loc, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32),
                 y=rs.randint(0, 4, SIZE[:3] + (1,)).astype(np.float32))
    return loc


def _dataset(folder, fmt, shuffle, resident, workers):
    from bts_amd import data
    return data.prepare_dataset(folder, 2, SIZE, list(CROP), 3, shuffle=shuffle, data_format=fmt, seed=7, device=dev(),
                                resident_bytes=resident, workers=workers)[0]


@pytest.mark.parametrize('shuffle', [True, False], ids=['shuffle', 'in_order'])
@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_batches_do_not_depend_on_residency_or_workers(folder, fmt, shuffle):
    import bts_amd  # noqa: F401
    runs = []
    for resident, workers in ((1 << 30, 0), (2 * EXAMPLE_BYTES, 2), (0, 0)):
        ds = _dataset(folder, fmt, shuffle, resident, workers)
        assert len(ds) == 3
        runs.append([b for _ in range(2) for b in ds])
        assert ds._resident_used <= resident and len(ds._resident) == {1 << 30: 5, 2 * EXAMPLE_BYTES: 2, 0: 0}[resident]
    shape = (2, 2) + CROP if fmt == 'channels_first' else (2,) + CROP + (2,)
    assert [tuple(b[0].shape) for b in runs[0][:3]] == [shape, shape, (1,) + shape[1:]]          # the last batch is ragged
    for other in runs[1:]:
        assert len(other) == len(runs[0]) == 6
        for (xa, ya), (xb, yb) in zip(runs[0], other):
            assert torch.equal(xa, xb) and torch.equal(ya, yb)


def test_a_resident_epoch_reads_no_file(folder, monkeypatch):
    import bts_amd  # noqa: F401
    ds = _dataset(folder, 'channels_last', True, 1 << 30, 2)
    ref = _dataset(folder, 'channels_last', True, 0, 0)
    want = [b for _ in range(3) for b in ref]
    got = [b for _ in range(2) for b in ds]

    def refuse(*a, **k):
        raise AssertionError('a resident epoch read a file')
    monkeypatch.setattr(np, 'load', refuse)
    got += list(ds)
    assert len(got) == 9
    for (xa, ya), (xb, yb) in zip(got, want):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)


def test_state_dict_is_the_two_generators_and_restores(folder):
    import bts_amd  # noqa: F401
    a = _dataset(folder, 'channels_last', True, 1 << 30, 2)
    list(a)
    st = a.state_dict()
    assert sorted(st) == ['gen', 'order_gen']
    want = list(a)
    b = _dataset(folder, 'channels_last', True, 0, 0)
    b.load_state_dict(st)
    for (xa, ya), (xb, yb) in zip(list(b), want):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)
