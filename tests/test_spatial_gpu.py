"""-m gpu: the spatial augmentation kernel (bts_augment_spatial_batch) and data.prepare_dataset(spatial=...).

Identity and quarter turns are bit-equal to ops.augment_batch (analytic checks); general draws are held against the float64 restatement
of tests/spatial_ref.py: labels exact away from rounding ties (at most 2 % of a case, tests/test_spatial_host.py asserts the cap for
these seeds), intensities within 3 delta L + 1e-5 max|x| (delta, L: spatial_ref.coordinate_delta / lipschitz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import spatial_ref as SR

pytestmark = pytest.mark.gpu

EYE = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def dev():
    return torch.device('cuda', 0)


def _ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def _upload(cs):
    ops = _ops()
    dx = [torch.from_numpy(x).to(dev()) for x in cs.xs]
    dy = [torch.from_numpy(y).to(dev()) for y in cs.ys]
    return dx, dy, [ops.channel_moments(x)[1] for x in dx]


def _plain(cs):
    return ([d['offsets'] for d in cs.draws], [d['mask'] for d in cs.draws], [d['shift'] for d in cs.draws],
            [d['scale'] for d in cs.draws], cs.out_ch)


@pytest.mark.parametrize('si', range(len(SR.SHAPES)))
def test_identity_is_bit_equal_to_augment_batch(si):
    """the flag off (the copy inside the launch), and on with M = I and no field (the gather: exact integer coordinates, weights 0 / 1)"""
    ops = _ops()
    cs = SR.case(si, 'affine')
    dx, dy, var = _upload(cs)
    n = len(dx)
    for cf in (False, True):
        wx, wy = ops.augment_batch(dx, dy, var, cs.crop, *_plain(cs), channels_first=cf)
        for flags in ([False] * n, [True] * n, [bool(i & 1) for i in range(n)]):
            gx, gy = ops.augment_spatial_batch(dx, dy, var, cs.crop, *_plain(cs), flags, [EYE] * n, [None] * n, [4] * n,
                                               channels_first=cf)
            assert torch.equal(gx, wx), 'x, channels_first %s, flags %s: max |d| %.3e' % (cf, flags, float((gx - wx).abs().max()))
            assert torch.equal(gy, wy), 'y, channels_first %s, flags %s' % (cf, flags)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_quarter_turn_is_rot90_of_the_window(axis):
    """M with entries exactly 0 / +-1 on a cubic crop inside a larger volume: out[t] = W[c + M (t - c)] = rot90(W, -1, (axis+1, axis+2)),
    so the launch equals augment_batch of the turned window (same variances, flips, shift and scale) bit for bit"""
    ops = _ops()
    vol, T, c, out_ch, n = (11, 10, 12), 8, 2, 3, 4
    xs, ys = SR.volumes(n, vol, c, out_ch, seed=40 + axis)
    dx, dy = [torch.from_numpy(x).to(dev()) for x in xs], [torch.from_numpy(y).to(dev()) for y in ys]
    var = [ops.channel_moments(x)[1] for x in dx]
    rs = np.random.RandomState(50 + axis)
    offs = [[int(rs.randint(0, vol[k] - T + 1)) for k in range(3)] for _ in range(n)]
    masks = [int(m) for m in rs.permutation(8)[:n]]
    shift, scale = rs.uniform(-0.1, 0.1, (n, c)).tolist(), rs.uniform(0.9, 1.1, (n, c)).tolist()
    M = np.round(SR.rotation(axis, np.pi / 2)).reshape(-1).tolist()
    assert sorted(set(M)) == [-1.0, 0.0, 1.0]
    dims = ((axis + 1) % 3, (axis + 2) % 3)
    wx = [torch.rot90(x[o[0]:o[0] + T, o[1]:o[1] + T, o[2]:o[2] + T], -1, dims).contiguous() for x, o in zip(dx, offs)]
    wy = [torch.rot90(y[o[0]:o[0] + T, o[1]:o[1] + T, o[2]:o[2] + T], -1, dims).contiguous() for y, o in zip(dy, offs)]
    for cf in (False, True):
        want = ops.augment_batch(wx, wy, var, (T, T, T), [[0, 0, 0]] * n, masks, shift, scale, out_ch, channels_first=cf)
        got = ops.augment_spatial_batch(dx, dy, var, (T, T, T), offs, masks, shift, scale, out_ch, [True] * n, [M] * n, [None] * n,
                                        [1] * n, channels_first=cf)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), 'channels_first %s' % cf


@pytest.mark.parametrize('mode', SR.MODES)
@pytest.mark.parametrize('si', range(len(SR.SHAPES)))
def test_draws_against_the_restatement(si, mode):
    ops = _ops()
    cs = SR.case(si, mode)
    dx, dy, var = _upload(cs)
    n = len(dx)
    phis = [None if d['phi'] is None else torch.from_numpy(d['phi']).to(dev()) for d in cs.draws]
    refs = [cs.reference(d) for d in range(n)]
    for cf in (False, True):
        gx, gy = ops.augment_spatial_batch(dx, dy, var, cs.crop, *_plain(cs), [True] * n, [d['M'] for d in cs.draws], phis,
                                           [d['spacing'] for d in cs.draws], channels_first=cf)
        if cf:
            gx, gy = gx.permute(0, 2, 3, 4, 1), gy.permute(0, 2, 3, 4, 1)
        gx, gy = gx.cpu().double().numpy(), gy.cpu().double().numpy()
        for d in range(n):
            xr, yr, tie = refs[d]
            assert tie.mean() <= SR.TIE_CAP
            assert np.array_equal(gy[d][~tie], yr[~tie]), 'labels of draw %d, channels_first %s' % (d, cf)
            err, bound = float(np.abs(gx[d] - xr).max()), SR.intensity_bound(cs.xs[d], xr)
            print('shape %d %s draw %d cf %d: max |d| %.3e, bound %.3e' % (si, mode, d, cf, err, bound))
            assert err <= bound, 'intensities of draw %d, channels_first %s: %.3e > %.3e' % (d, cf, err, bound)


@pytest.mark.parametrize('i', range(len(SR.EXTRA)), ids=['field_from_memory', 'row_longer_than_a_wave', 'six_rows_per_unit'])
def test_other_paths_against_the_restatement(i):
    """rotation + zoom + elastic at the shapes where the kernel takes another path (spatial_ref.EXTRA); the same yardstick, with the
    case's own delta"""
    ops = _ops()
    cs = SR.case(i, 'both', True)
    dx, dy, var = _upload(cs)
    n = len(dx)
    phis = [torch.from_numpy(d['phi']).to(dev()) for d in cs.draws]
    delta = cs.delta()
    for cf in (False, True):
        gx, gy = ops.augment_spatial_batch(dx, dy, var, cs.crop, *_plain(cs), [True] * n, [d['M'] for d in cs.draws], phis,
                                           [d['spacing'] for d in cs.draws], channels_first=cf)
        if cf:
            gx, gy = gx.permute(0, 2, 3, 4, 1), gy.permute(0, 2, 3, 4, 1)
        gx, gy = gx.cpu().double().numpy(), gy.cpu().double().numpy()
        for d in range(n):
            xr, yr, tie = cs.reference(d)
            assert tie.mean() <= SR.TIE_CAP
            assert np.array_equal(gy[d][~tie], yr[~tie]), 'labels of draw %d, channels_first %s' % (d, cf)
            err, bound = float(np.abs(gx[d] - xr).max()), SR.intensity_bound(cs.xs[d], xr, delta)
            print('extra %d draw %d cf %d: max |d| %.3e, bound %.3e' % (i, d, cf, err, bound))
            assert err <= bound, 'intensities of draw %d, channels_first %s: %.3e > %.3e' % (d, cf, err, bound)
    # and the identity through the same shapes, bit for bit
    wx, wy = ops.augment_batch(dx, dy, var, cs.crop, *_plain(cs))
    gx, gy = ops.augment_spatial_batch(dx, dy, var, cs.crop, *_plain(cs), [bool(k & 1) for k in range(n)], [EYE] * n, [None] * n, [4] * n)
    assert torch.equal(gx, wx) and torch.equal(gy, wy)


def test_fill_outside_the_volume():
    """a crop equal to its volume at zoom 0.7: the voxels whose eight corners all lie outside carry aug_value(fill) -- the bits
    augment_batch gives a volume that holds `fill` everywhere -- and an all-zero one-hot row"""
    ops = _ops()
    vol, c, out_ch = (12, 10, 14), 2, 3
    xs, ys = SR.volumes(1, vol, c, out_ch, seed=60)
    ys[0][:] = np.maximum(ys[0], 1.0)                    # no background inside: a zero row can only come from outside
    dx, dy = torch.from_numpy(xs[0]).to(dev()), torch.from_numpy(ys[0]).to(dev())
    var = ops.channel_moments(dx)[1]
    fill, shift, scale = [-3.5, 7.25], [0.05, -0.07], [1.05, 0.93]
    M = (np.eye(3) / 0.7)
    s = SR.coordinates(vol, (0, 0, 0), M)
    outside = ((s <= -1.0) | (s >= np.array(vol, np.float64))).any(axis=-1)
    assert 0.2 < outside.mean() < 0.8
    const = torch.tensor(fill, device=dev()).expand(vol + (c,)).contiguous()
    for cf in (False, True):
        for mask in (0, 5):
            wx, _ = ops.augment_batch([const], [dy], [var], vol, [[0, 0, 0]], [mask], [shift], [scale], out_ch, channels_first=cf)
            gx, gy = ops.augment_spatial_batch([dx], [dy], [var], vol, [[0, 0, 0]], [mask], [shift], [scale], out_ch, [True],
                                               [M.reshape(-1).tolist()], [None], [1], fills=[fill], channels_first=cf)
            if cf:
                gx, gy, wx = gx.permute(0, 2, 3, 4, 1), gy.permute(0, 2, 3, 4, 1), wx.permute(0, 2, 3, 4, 1)
            out = torch.from_numpy(np.ascontiguousarray(SR._flip(outside, [bool(mask & 4), bool(mask & 2), bool(mask & 1)]))).to(dev())
            assert torch.equal(gx[0][out], wx[0][out])
            assert bool((gy[0][out] == 0).all()) and bool((gy[0].sum(-1) == 1).any())
            xr, yr, tie = SR.augment(xs[0], ys[0], vol, (0, 0, 0), [bool(mask & 4), bool(mask & 2), bool(mask & 1)], shift, scale, out_ch,
                                     M, fill=fill)
            assert np.array_equal(gy[0].cpu().double().numpy()[~tie], yr[~tie])
            # (this case's own delta, and an L that counts the step from a border voxel to its channel's fill)
            delta = 4.0 * float(np.abs(SR.coordinates(vol, (0, 0, 0), M, dtype=np.float32).astype(np.float64) - s).max())
            L = max(SR.lipschitz(xs[0][..., k:k + 1], fill[k])[1] for k in range(c))
            bound = 3.0 * delta * L + 1e-5 * float(np.abs(xr).max())
            assert float(np.abs(gx[0].cpu().double().numpy() - xr).max()) <= bound


@pytest.mark.parametrize('cf', [False, True], ids=['channels_last', 'channels_first'])
def test_a_batch_of_17_splits_and_writes_only_its_outputs(cf):
    """more than one launch carries; identity and spatial examples mixed; out= views of sentinel-filled buffers at 16-, 4- and 8-byte
    aligned starts: bit-equal to 17 single calls, sentinels untouched, two runs bit-identical"""
    ops = _ops()
    n = 17
    assert n > 2 * ops.augment_spatial_batch_max()
    vol, crop, c, out_ch = (9, 10, 11), (8, 8, 7), 2, 3
    xs, ys = SR.volumes(n, vol, c, out_ch, seed=70)
    dx, dy = [torch.from_numpy(x).to(dev()) for x in xs], [torch.from_numpy(y).to(dev()) for y in ys]
    var = [ops.channel_moments(x)[1] for x in dx]
    rs = np.random.RandomState(71)
    offs = [[int(rs.randint(0, vol[k] - crop[k] + 1)) for k in range(3)] for _ in range(n)]
    masks = [i % 8 for i in range(n)]
    shift, scale = rs.uniform(-0.1, 0.1, (n, c)).tolist(), rs.uniform(0.9, 1.1, (n, c)).tolist()
    flags = [i % 3 != 0 for i in range(n)]
    mats = [SR.matrix(np.deg2rad(rs.uniform(-30, 30, 3)), rs.uniform(0.7, 1.4)).reshape(-1).tolist() for _ in range(n)]
    spacings = [(4, 8)[i % 2] for i in range(n)]
    phis = [torch.from_numpy((rs.randn(*(SR.grid(crop, spacings[i]) + (3,))) * 2).astype(np.float32)).to(dev()) if i % 4 else None
            for i in range(n)]
    fills = rs.uniform(-5, 5, (n, c)).tolist()
    a = lambda i: ([offs[i]], [masks[i]], [shift[i]], [scale[i]], out_ch, [flags[i]], [mats[i]], [phis[i]], [spacings[i]])      # noqa: E731
    singles = [ops.augment_spatial_batch([dx[i]], [dy[i]], [var[i]], crop, *a(i), fills=[fills[i]], channels_first=cf) for i in range(n)]
    want_x, want_y = torch.cat([s[0] for s in singles]), torch.cat([s[1] for s in singles])
    whole = (offs, masks, shift, scale, out_ch, flags, mats, phis, spacings)
    first = ops.augment_spatial_batch(dx, dy, var, crop, *whole, fills=fills, channels_first=cf)
    assert torch.equal(first[0], want_x) and torch.equal(first[1], want_y)
    tail, sentinel = 37, -777.0
    for lead in (4, 1, 2):
        bx = torch.full((lead + want_x.numel() + tail,), sentinel, device=dev())
        by = torch.full((lead + want_y.numel() + tail,), sentinel, device=dev())
        ox = bx[lead:lead + want_x.numel()].view(want_x.shape)
        oy = by[lead:lead + want_y.numel()].view(want_y.shape)
        ops.augment_spatial_batch(dx, dy, var, crop, *whole, fills=fills, channels_first=cf, out=(ox, oy))
        torch.cuda.synchronize()
        assert torch.equal(ox, want_x) and torch.equal(oy, want_y), 'lead %d' % lead
        for buf, size in ((bx, want_x.numel()), (by, want_y.numel())):
            assert bool((buf[:lead] == sentinel).all()) and bool((buf[lead + size:] == sentinel).all())


# ---- the dataset ----------------------------------------------------------------------------------------------------------------
SIZE, CROP = (10, 12, 9, 2), (8, 8, 8)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    loc = str(tmp_path_factory.mktemp('spatial_examples'))
    rs = np.random.RandomState(0)
    for i in range(5):
        np.savez(os.path.join(loc, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32),
                 y=rs.randint(0, 4, SIZE[:3] + (1,)).astype(np.float32))
    return loc


def _dataset(folder, fmt, resident, workers, seed=7, cfg='default', batch=2):
    import bts_amd  # noqa: F401
    from bts_amd import data
    if cfg == 'default':
        cfg = data.SpatialConfig(0.6, rotate_deg=(20, 10, 30), zoom=(0.8, 1.25), elastic_sigma=1.5, elastic_spacing=4, fill=0.0)
    return data.prepare_dataset(folder, batch, SIZE, list(CROP), 3, shuffle=True, data_format=fmt, seed=seed, device=dev(),
                                resident_bytes=resident, workers=workers, spatial=cfg)[0]


def _same(a, b):
    assert len(a) == len(b)
    for (xa, ya), (xb, yb) in zip(a, b):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)


@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_dataset_batches_do_not_depend_on_the_path(folder, fmt):
    """reproducible for a seed, the same for (resident_bytes, workers) in {(0,0), (big,0), (big,2)}: per-example and batched paths"""
    runs = [[b for _ in range(2) for b in _dataset(folder, fmt, r, w)] for r, w in ((0, 0), (0, 0), (1 << 30, 0), (1 << 30, 2))]
    shape = (2, 2) + CROP if fmt == 'channels_first' else (2,) + CROP + (2,)
    assert [tuple(b[0].shape) for b in runs[0][:3]] == [shape, shape, (1,) + shape[1:]]
    for other in runs[1:]:
        _same(runs[0], other)
    # the transform is really there, and another seed gives other batches
    plain = [b for _ in range(2) for b in _dataset(folder, fmt, 0, 0, cfg=None)]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(runs[0], plain))
    other = list(_dataset(folder, fmt, 0, 0, seed=8))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(runs[0], other))


def test_dataset_state_dict_resumes_bit_exactly(folder):
    """five examples in batches of three: after two batches an epoch is complete, which is where train.save_checkpoint takes the state
    (the two generators, nothing else)"""
    a = _dataset(folder, 'channels_last', 1 << 30, 2, batch=3)
    assert len(list(a)) == 2
    st = a.state_dict()
    assert sorted(st) == ['gen', 'order_gen']
    want = list(a) + list(a)
    b = _dataset(folder, 'channels_last', 0, 0, batch=3)
    b.load_state_dict(st)
    _same(list(b) + list(b), want)


# ---- status codes -----------------------------------------------------------------------------------------------------------------
def test_status_codes_without_a_device_fault():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    assert 1 <= L._bts_augment_spatial_batch_max() <= L._bts_augment_batch_max()
    n = 2
    ptrs = (ctypes.c_void_p * n)(64, 64)                    # (never dereferenced on the host, never reached by a refused call)
    nulls = (ctypes.c_void_p * n)(None, None)
    offs = (ctypes.c_int * (3 * n))(0, 0, 0, 1, 2, 3)
    flips = (ctypes.c_int * n)(0, 7)
    sh, sc, fi = (ctypes.c_float * (n * 16))(), (ctypes.c_float * (n * 16))(), (ctypes.c_float * (n * 16))()
    on = (ctypes.c_int * n)(1, 0)
    mats = (ctypes.c_float * (9 * n))(*(EYE * n))
    spc = (ctypes.c_int * n)(4, 1)
    P = lambda a: ctypes.cast(a, ctypes.c_void_p) if a is not None else None      # noqa: E731

    def call(N=n, S=(9, 10, 11), C=2, T=(8, 8, 8), out_ch=3, layout=0, x=ptrs, y=ptrs, var=ptrs, offsets=offs, flip=flips, shift=sh,
             scale=sc, spatial=on, M=mats, phi=nulls, spacing=spc, fill=fi):
        return L._bts_augment_spatial_batch(P(x), P(y), P(var), None, None, N, S[0], S[1], S[2], C, T[0], T[1], T[2], P(offsets), P(flip),
                                            P(shift), P(scale), P(spatial), P(M), P(phi), P(spacing), P(fill), out_ch, layout, None)
    SHAPE = -1
    # everything bts_augment_batch rejects
    assert call(N=0) == SHAPE and call(N=-3) == SHAPE
    assert call(C=0) == SHAPE and call(C=17) == SHAPE
    assert call(out_ch=0) == SHAPE
    assert call(layout=2) == SHAPE and call(layout=-1) == SHAPE
    assert call(T=(8, 8, 12)) == SHAPE and call(T=(0, 8, 8)) == SHAPE
    assert call(flip=(ctypes.c_int * n)(0, 8)) == SHAPE
    assert call(offsets=(ctypes.c_int * (3 * n))(0, 0, 0, 2, 2, 3)) == SHAPE
    assert call(offsets=(ctypes.c_int * (3 * n))(0, -1, 0, 0, 0, 0)) == SHAPE
    # a NULL table, old or new
    for name in ('x', 'y', 'var', 'offsets', 'flip', 'shift', 'scale', 'spatial', 'M', 'phi', 'spacing', 'fill'):
        assert call(**{name: None}) == SHAPE, name
    # spacing < 1 and a non-finite M, on an example whose flag is on or off
    assert call(spacing=(ctypes.c_int * n)(0, 1)) == SHAPE and call(spacing=(ctypes.c_int * n)(4, -2)) == SHAPE
    for bad in (float('nan'), float('inf'), -float('inf')):
        for at in (4, 9 + 8):
            m = EYE * n
            m[at] = bad
            assert call(M=(ctypes.c_float * (9 * n))(*m)) == SHAPE
    # a field with more than 256 nodes along axis 2
    assert call(S=(4, 4, 300), T=(4, 4, 300), offsets=(ctypes.c_int * (3 * n))(), phi=ptrs, spacing=(ctypes.c_int * n)(1, 1)) == SHAPE
    # the wrapper refuses the same by name, and a field of the wrong extent
    ops = _ops()
    x = torch.zeros((9, 10, 11, 2), device=dev())
    y = torch.zeros((9, 10, 11, 1), device=dev())
    var = ops.channel_moments(x)[1]
    base = dict(xs=[x], ys=[y], variances=[var], crop=(8, 8, 8), offsets=[[0, 0, 0]], flip_masks=[0], shifts=[[0, 0]], scales=[[1, 1]],
                out_ch=3, spatial=[True], matrices=[EYE], phis=[None], spacings=[4])
    ops.augment_spatial_batch(**base)
    for change in (dict(spacings=[0]), dict(phis=[torch.zeros((6, 5, 5, 3), device=dev())]), dict(matrices=[EYE[:8]]),
                   dict(fills=[[0.0]]), dict(spatial=[True, False]), dict(phis=[torch.zeros((5, 5, 5, 3))])):
        with pytest.raises((ValueError, RuntimeError)):
            ops.augment_spatial_batch(**dict(base, **change))
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.augment_spatial_batch(**dict(base, matrices=[[float('nan')] + EYE[1:]]))
    torch.cuda.synchronize()


# ---- the command ------------------------------------------------------------------------------------------------------------------
def test_command_trains_with_the_flags_and_validates_without(tmp_path, monkeypatch):
    """python -m bts_amd.train with the spatial flags: the training set carries the config, the validation set none and its batches are
    those of a run without the flags; train.log is finite, train_args.pkl keeps the flags"""
    import bts_amd  # noqa: F401
    from bts_amd import data, train as T
    from bts_amd.layers import _base
    size = (20, 18, 22, 2)
    loc = str(tmp_path)
    rs = np.random.RandomState(5)
    for sub, n in (('train', 3), ('val', 2)):
        os.makedirs(os.path.join(loc, sub))
        for i in range(n):
            lab = (rs.rand(*size[:3]) * 4).astype(np.int64).astype(np.float32)[..., None]
            np.savez(os.path.join(loc, sub, 'ex%d.npz' % i), x=rs.randn(*size).astype(np.float32), y=lab)
    np.save(os.path.join(loc, 'prepro.npy'), {'size': dict(zip('hwdc', size)), 'norm': {'mean': np.zeros(2), 'std': np.ones(2)}},
            allow_pickle=True)
    made, real = [], data.prepare_dataset

    def spy(*a, **k):
        made.append(real(*a, **k)[0])
        return made[-1], len(made[-1].files)
    monkeypatch.setattr(data, 'prepare_dataset', spy)
    val_batches = []
    for flags in (['--spatial_prob', '1', '--rotate_deg', '20', '--zoom_range', '0.8,1.2', '--elastic_sigma', '1.5', '--elastic_spacing', '8'],
                  []):
        del made[:]
        out = os.path.join(loc, 'run%d' % len(flags))
        _base.set_seed(0)
        res = T.run(T.parse_args(['--train_loc', os.path.join(loc, 'train'), '--val_loc', os.path.join(loc, 'val'), '--prepro_loc',
                                  os.path.join(loc, 'prepro.npy'), '--save_folder', out, '--crop_size', '16,16,16', '--base_filters', '16',
                                  '--groups', '4', '--reduction', '4', '--depth', '3', '--batch_size', '2', '--n_epochs', '1',
                                  '--workers', '0'] + flags))
        train_set, val_set = made
        assert val_set.spatial is None and (train_set.spatial is not None) == bool(flags)
        assert all(np.isfinite(float(v)) for v in res['history'][0].values())
        stored = T.load_train_args(out)
        assert stored['spatial_prob'] == (1.0 if flags else 0.0) and stored['elastic_spacing'] == (8 if flags else 32)
        val_set.load_state_dict({'order_gen': torch.Generator().manual_seed(0).get_state(),
                                 'gen': torch.Generator().manual_seed(7919).get_state()})
        val_batches.append(list(val_set))
    _same(val_batches[0], val_batches[1])
