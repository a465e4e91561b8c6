"""-m gpu: foreground-oversampled crops in the dataset behind data.prepare_dataset (ForegroundConfig, draw_foreground, the per-file
class-location table), patterned on tests/test_input_batch_gpu.py: five 10x12x9x2 examples, a 4x4x4 crop, batches of two.  Expected
batches are restated here from the draws (data.draw, tests/sampling_ref.py for the table and the foreground draw) and the augment
launches called directly."""
import os

import numpy as np
import pytest
import torch

import sampling_ref as S

pytestmark = pytest.mark.gpu

SIZE, CROP, OUT_CH, SEED, BATCH = (10, 12, 9, 2), (4, 4, 4), 3, 7, 2
VOL = SIZE[:3]
EXAMPLE_BYTES = (10 * 12 * 9 * 2 + 10 * 12 * 9) * 4
CORNERS = [(0, 0, 0), (9, 11, 8), (0, 11, 0), (9, 0, 8), (9, 11, 0)]          # one foreground voxel each, label 1 + i % 3


def dev():
    return torch.device('cuda', 0)


def _data():
    import bts_amd  # noqa: F401
    from bts_amd import data
    return data


def _write(loc, labels):
    rs = np.random.RandomState(0)
    for i, y in enumerate(labels):
        np.savez(os.path.join(loc, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32), y=y.reshape(VOL + (1,)).astype(np.float32))
    return loc


@pytest.fixture(scope='module')
def corner_folder(tmp_path_factory):
    labels = []
    for i, p in enumerate(CORNERS):
        y = np.zeros(VOL, np.float32)
        y[p] = 1 + i % 3
        labels.append(y)
    return _write(str(tmp_path_factory.mktemp('corners')), labels)


@pytest.fixture(scope='module')
def empty_folder(tmp_path_factory):
    return _write(str(tmp_path_factory.mktemp('empty')), [np.zeros(VOL, np.float32)] * 5)


@pytest.fixture(scope='module')
def random_folder(tmp_path_factory):
    rs = np.random.RandomState(1)
    labels = [(rs.randint(1, 4, VOL) * (rs.random_sample(VOL) < 0.05)).astype(np.float32) for _ in range(4)]
    labels.append(np.zeros(VOL, np.float32))                                    # ... and one example without foreground
    return _write(str(tmp_path_factory.mktemp('random')), labels)


def _dataset(folder, fmt='channels_last', resident=0, workers=0, shuffle=False, **kw):
    return _data().prepare_dataset(folder, BATCH, SIZE, list(CROP), OUT_CH, shuffle=shuffle, data_format=fmt, seed=SEED, device=dev(),
                                   rank=0, world=1, resident_bytes=resident, workers=workers, **kw)[0]


def _examples(folder):
    out = []
    for i in range(5):
        z = np.load(os.path.join(folder, 'ex%d.npz' % i))
        out.append((z['x'], z['y']))
    return out


def _restated(folder, epochs, foreground=None, spatial=None, intensity=None):
    """the in-order epochs as the dataset's docstring orders the draws -> (list of (x, y) channels-last batches, list of the Draws, the
    generator)"""
    data = _data()
    from bts_amd import ops
    ex = _examples(folder)
    dx = [torch.from_numpy(x).to(dev()) for x, _ in ex]
    dy = [torch.from_numpy(y).to(dev()) for _, y in ex]
    var = [ops.channel_moments(x)[1] for x in dx]
    tables = [S.class_locations_ref(y, OUT_CH, foreground.samples) for _, y in ex] if foreground is not None else None
    gen = torch.Generator().manual_seed(SEED + 7919)
    batches, all_draws = [], []
    for _ in range(epochs):
        for first in range(0, 5, BATCH):
            ids = list(range(first, min(first + BATCH, 5)))
            draws, sdraws, idraws = [], [], []
            for i in ids:
                dr = data.draw(gen, SIZE[3], VOL, CROP)
                if foreground is not None:
                    dr.offsets = S.draw_foreground_ref(gen, foreground.prob, foreground.classes, tables[i][0], tables[i][1], VOL, CROP,
                                                       dr.offsets)
                draws.append(dr)
                if spatial is not None:
                    sdraws.append(data.draw_spatial(gen, spatial, CROP))
                if intensity is not None:
                    idraws.append(data.draw_intensity(gen, intensity, SIZE[3]))
            a = ([dx[i] for i in ids], [dy[i] for i in ids], [var[i] for i in ids], CROP, [d.offsets for d in draws],
                 [d.flip_mask for d in draws], [d.shift for d in draws], [d.scale for d in draws], OUT_CH)
            if spatial is None:
                xb, yb = ops.augment_batch(*a)
            else:
                xb, yb = ops.augment_spatial_batch(*a, [s.on for s in sdraws], [s.matrix.reshape(-1).tolist() for s in sdraws],
                                                   [None if s.phi is None else s.phi.to(dev()) for s in sdraws],
                                                   [s.spacing for s in sdraws], [spatial.fill_of(SIZE[3])] * len(ids))
            if intensity is not None:
                ops.intensity_batch(xb, [d.params for d in idraws], [d.key for d in idraws])
            batches.append((xb, yb))
            all_draws.append(draws)
    return batches, all_draws, gen


def _same(got, want):
    assert len(got) == len(want)
    for (xa, ya), (xb, yb) in zip(got, want):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)


def test_every_crop_holds_the_only_foreground_voxel_where_the_draws_put_it(corner_folder):
    data = _data()
    cfg = data.ForegroundConfig(1.0, samples=16)
    for resident in (0, 1 << 30):
        ds = _dataset(corner_folder, resident=resident, foreground=cfg)
        got = [b for _ in range(2) for b in ds]
        want, draws, gen = _restated(corner_folder, 2, foreground=cfg)
        _same(got, want)
        assert torch.equal(ds.gen.get_state(), gen.get_state())
        seen = 0
        for b, ((_, y), drs) in enumerate(zip(got, draws)):
            y = y.cpu().numpy()
            for n, dr in enumerate(drs):
                i = (b % 3) * BATCH + n
                assert y[n].sum() == 1.0, (b, n)
                p = CORNERS[i]
                # a corner voxel clamps every axis: the offset is 0 or vol - crop
                assert dr.offsets == [0 if p[a] == 0 else VOL[a] - CROP[a] for a in range(3)]
                t = [p[a] - dr.offsets[a] for a in range(3)]
                t = tuple(CROP[a] - 1 - t[a] if dr.flips[a] else t[a] for a in range(3))
                assert y[n][t + (i % 3,)] == 1.0, (b, n, t)
                seen += 1
        assert seen == 10


def test_an_example_without_foreground_keeps_the_uniform_crop(empty_folder):
    data = _data()
    cfg = data.ForegroundConfig(1.0, samples=16)
    got = list(_dataset(empty_folder, foreground=cfg))
    # the crops draw() places, with the three foreground values taken and not used
    gen = torch.Generator().manual_seed(SEED + 7919)
    from bts_amd import ops
    ex = _examples(empty_folder)
    want = []
    for first in range(0, 5, BATCH):
        ids = list(range(first, min(first + BATCH, 5)))
        draws = []
        for _ in ids:
            draws.append(data.draw(gen, SIZE[3], VOL, CROP))
            torch.rand(3, generator=gen, dtype=torch.float64)
        dx = [torch.from_numpy(ex[i][0]).to(dev()) for i in ids]
        dy = [torch.from_numpy(ex[i][1]).to(dev()) for i in ids]
        want.append(ops.augment_batch(dx, dy, [ops.channel_moments(x)[1] for x in dx], CROP, [d.offsets for d in draws],
                                      [d.flip_mask for d in draws], [d.shift for d in draws], [d.scale for d in draws], OUT_CH))
    _same(got, want)


@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_off_is_the_dataset_without_the_argument(random_folder, fmt):
    for resident, workers in ((0, 0), (1 << 30, 2)):
        a = _dataset(random_folder, fmt, resident, workers, shuffle=True)
        b = _dataset(random_folder, fmt, resident, workers, shuffle=True, foreground=None)
        _same([x for _ in range(2) for x in b], [x for _ in range(2) for x in a])
        sa, sb = a.state_dict(), b.state_dict()
        assert sorted(sa) == sorted(sb) == ['gen', 'order_gen']
        assert torch.equal(sa['gen'], sb['gen']) and torch.equal(sa['order_gen'], sb['order_gen'])


@pytest.mark.parametrize('shuffle', [True, False], ids=['shuffle', 'in_order'])
def test_batches_do_not_depend_on_residency_workers_or_layout(random_folder, shuffle):
    data = _data()
    cfg = data.ForegroundConfig(0.6, samples=5, classes=[0, 2])
    runs = {}
    for fmt in ('channels_last', 'channels_first'):
        for resident, workers in ((1 << 30, 0), (2 * EXAMPLE_BYTES, 2), (0, 0)):
            ds = _dataset(random_folder, fmt, resident, workers, shuffle=shuffle, foreground=cfg)
            runs[fmt, resident] = [b for _ in range(2) for b in ds]
            assert ds._resident_used <= resident and len(ds._resident) == {1 << 30: 5, 2 * EXAMPLE_BYTES: 2, 0: 0}[resident]
            assert sorted(ds.state_dict()) == ['gen', 'order_gen']
    first = runs['channels_last', 1 << 30]
    assert len(first) == 6
    for (fmt, _), other in runs.items():
        if fmt == 'channels_first':
            other = [(x.permute(0, 2, 3, 4, 1).contiguous(), y.permute(0, 2, 3, 4, 1).contiguous()) for x, y in other]
        _same(other, first)
    if not shuffle:
        _same(first, _restated(random_folder, 2, foreground=cfg)[0])
        # ... and the oversampling does something: these crops are not the uniform ones
        plain = [b for _ in range(2) for b in _dataset(random_folder, foreground=None)]
        assert any(not torch.equal(a[1], b[1]) for a, b in zip(first, plain))


def test_a_resident_example_has_its_table_built_once(random_folder, monkeypatch):
    data = _data()
    calls = []
    real = data.ops.class_locations

    def counted(y, out_ch, k):
        calls.append((tuple(y.shape), out_ch, k))
        return real(y, out_ch, k)
    monkeypatch.setattr(data.ops, 'class_locations', counted)
    cfg = data.ForegroundConfig(0.5, samples=9)
    ds = _dataset(random_folder, resident=1 << 30, workers=0, shuffle=True, foreground=cfg)
    for _ in range(2):
        list(ds)
    assert calls == [(VOL + (1,), OUT_CH, 9)] * 5
    del calls[:]
    for resident in (0, 2 * EXAMPLE_BYTES):                    # streamed examples: rebuilt per read
        ds = _dataset(random_folder, resident=resident, workers=1 if resident else 0, foreground=cfg)
        for _ in range(2):
            list(ds)
    assert len(calls) == 10 + (5 + 3)                          # (the second epoch of the second dataset finds two examples resident)
    del calls[:]
    list(_dataset(random_folder, resident=1 << 30))            # off: the kernel is never asked
    assert calls == []


@pytest.mark.parametrize('targets', ['labels', 'regions'])
def test_it_composes_with_the_spatial_and_intensity_stages(random_folder, targets):
    """everything on: the batches are the restated ones -- the foreground draw changes the offsets and nothing else"""
    data = _data()
    from bts_amd import ops
    cfg = data.ForegroundConfig(0.7, samples=6)
    spatial = data.SpatialConfig(0.8, rotate_deg=10.0, elastic_sigma=0.5, elastic_spacing=2)
    intensity = data.IntensityConfig(noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5, gamma_prob=0.5)
    want, draws, gen = _restated(random_folder, 1, foreground=cfg, spatial=spatial, intensity=intensity)
    if targets == 'regions':
        for _, y in want:
            ops.region_targets(y)
    off, _, _ = _restated(random_folder, 1, spatial=spatial, intensity=intensity)
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(want, off))
    for resident, workers in ((0, 0), (1 << 30, 2)):
        ds = _dataset(random_folder, resident=resident, workers=workers, foreground=cfg, spatial=spatial, intensity=intensity,
                      targets=targets)
        _same(list(ds), want)
        assert torch.equal(ds.gen.get_state(), gen.get_state())
