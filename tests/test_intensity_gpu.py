"""-m gpu: the intensity augmentation kernels (bts_intensity_batch) and data.prepare_dataset(intensity=...).

Every stage alone and the whole chain are held against the float64 restatement of tests/intensity_ref.py, fed the same float32 input, in
both layouts, within intensity_ref.Case.bound (noise: 2e-5 s + 2^-23 max|out|; blur: 6 (2r+3) 2^-24 max|v|; contrast, gamma and the
chain: 4 x the float32 restatement's distance from float64, + 4 x 2^-24 of the range where powf acts; tests/test_intensity_host.py
asserts the conditions on these bounds).  Bit-equality where the semantics promise it."""
import ctypes
import os

import numpy as np
import pytest
import torch

import intensity_ref as IR

pytestmark = pytest.mark.gpu

LAYOUTS = pytest.mark.parametrize('cf', [False, True], ids=['channels_last', 'channels_first'])


def dev():
    return torch.device('cuda', 0)


def _ops():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    return ops


def _run(x, params, keys, cf):
    """x: (N,T0,T1,T2,C) host array or device tensor -> the device result, brought back to channels last"""
    t = (torch.from_numpy(x) if isinstance(x, np.ndarray) else x).to(dev())
    if cf:
        t = t.permute(0, 4, 1, 2, 3).contiguous()
    else:
        t = t.clone()
    out = _ops().intensity_batch(t, params, keys, cf)
    assert out is t                                                     # in place
    return out.permute(0, 2, 3, 4, 1).contiguous() if cf else out


@LAYOUTS
@pytest.mark.parametrize('kind', IR.KINDS)
@pytest.mark.parametrize('si', range(len(IR.SHAPES)))
def test_against_the_restatement(si, kind, cf):
    cs = IR.case(si, kind)
    got = _run(cs.x, cs.params, cs.keys, cf).cpu().numpy().astype(np.float64)
    err = np.abs(got - cs.ref()).max(axis=(1, 2, 3))
    bound = cs.bound()
    print('%s %s C%d: largest error / bound = %.3f (error %.3e)' % (kind, cs.crop, cs.c, (err / bound).max(), err.max()))
    assert np.all(err <= bound), (err / bound)
    if kind == 'bright':                                                # bit-equal to the float32 product
        m = torch.tensor([[e[3] for e in row] for row in cs.params], dtype=torch.float32)[:, None, None, None, :]
        assert torch.equal(torch.from_numpy(got.astype(np.float32)), torch.from_numpy(cs.x) * m)
    if kind == 'chain' and cs.c == 4:                                   # the channel without a flag is as it was
        assert np.array_equal(got[2, ..., 3].astype(np.float32), cs.x[2, ..., 3])


@LAYOUTS
def test_all_flags_off_leaves_the_input_bit_unchanged(cf):
    """a sentinel pattern (NaNs with distinct payloads among them) survives a call without a flag, and the flagless volumes of a call
    with flags elsewhere"""
    bits = (np.arange(2 * 6 * 5 * 7 * 3, dtype=np.uint32) * np.uint32(2654435761)).reshape(2, 6, 5, 7, 3)
    x = torch.from_numpy(bits.view(np.float32).copy())
    off = [[(0, float('nan'), -1.0, 0.0, -2.0, float('inf'))] * 3] * 2              # (numbers of stages that are off are not looked at)
    got = _run(x, off, [(1, 2), (3, 4)], cf).cpu()
    assert torch.equal(got.view(torch.int32), x.view(torch.int32))
    one = [[off[0][0], (IR.BRIGHT, 0.0, 1.0, 1.5, 1.0, 1.0), off[0][0]], off[1]]
    got = _run(x, one, [(1, 2), (3, 4)], cf).cpu()
    same = torch.ones(x.shape, dtype=torch.bool)
    same[0, ..., 1] = False
    assert torch.equal(got.view(torch.int32)[same], x.view(torch.int32)[same])
    assert not torch.equal(got.view(torch.int32)[~same], x.view(torch.int32)[~same])


@pytest.mark.parametrize('si', [0, 2, 3])
def test_noise_is_the_same_in_both_layouts(si):
    cs = IR.case(si, 'noise')
    a, b = _run(cs.x, cs.params, cs.keys, False), _run(cs.x, cs.params, cs.keys, True)
    assert torch.equal(a, b) and not torch.equal(a.cpu(), torch.from_numpy(cs.x))
    chain = IR.case(si, 'chain')                                       # ... and so is everything else
    assert torch.equal(_run(chain.x, chain.params, chain.keys, False), _run(chain.x, chain.params, chain.keys, True))


@LAYOUTS
def test_a_constant_volume_goes_through_contrast_and_gamma(cf):
    x = np.empty((1, 7, 6, 9, 4), np.float32)
    values = (3.25, -1.5, 0.0, 1000.0)
    for c, v in enumerate(values):
        x[..., c] = v
    params = [[(IR.CONTRAST, 0, 1, 1, 0.8, 1), (IR.GAMMA, 0, 1, 1, 1, 1.4), (IR.CONTRAST | IR.GAMMA | IR.INVERT, 0, 1, 1, 1.3, 0.7),
               (IR.BRIGHT | IR.CONTRAST | IR.GAMMA, 0, 1, 1.0, 1.2, 1.2)]]
    got = _run(x, params, [(0, 0)], cf).cpu().numpy()
    assert np.all(np.isfinite(got))
    assert np.array_equal(got[..., 0], x[..., 0])                       # contrast: (v - mu) f + mu with v = mu exactly
    for c, v in enumerate(values):                                      # gamma: up to the rounding of its last line
        assert np.abs(got[..., c] - v).max() <= 2.0 ** -22 * abs(v)


@LAYOUTS
def test_a_batch_of_17_is_17_single_calls(cf):
    """mixed flags, more (n, c) volumes than one launch's table carries: bit-equal to one call per example, and to itself run again"""
    crop, c, n = (6, 7, 9), 3, 17
    rs = np.random.RandomState(8)
    x = rs.randn(n, *crop, c).astype(np.float32)
    x[:, :2] = 0.0
    params, keys = [], []
    for i in range(n):
        row = []
        for j in range(c):
            flags = int(rs.randint(0, 64)) if (i + j) % 5 else 0
            row.append((flags, rs.uniform(0.0, 0.2), rs.uniform(0.5, 1.6), rs.uniform(0.8, 1.2), rs.uniform(0.7, 1.4), rs.uniform(0.6, 1.8)))
        params.append(row)
        keys.append((int(rs.randint(0, 2 ** 31)), int(rs.randint(0, 2 ** 31))))
    whole = _run(x, params, keys, cf)
    assert torch.equal(whole, _run(x, params, keys, cf))
    for i in range(n):
        assert torch.equal(whole[i:i + 1], _run(x[i:i + 1], params[i:i + 1], keys[i:i + 1], cf)), i
    flagless = [(i, j) for i in range(n) for j in range(c) if not params[i][j][0] & 31]
    assert flagless and all(torch.equal(whole[i, ..., j].cpu(), torch.from_numpy(x[i, ..., j])) for i, j in flagless)


# ---- the dataset ----------------------------------------------------------------------------------------------------------------
SIZE, CROP = (10, 12, 9, 2), (8, 8, 8)


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    loc = str(tmp_path_factory.mktemp('intensity_examples'))
    rs = np.random.RandomState(0)
    for i in range(5):
        np.savez(os.path.join(loc, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32),
                 y=rs.randint(0, 4, SIZE[:3] + (1,)).astype(np.float32))
    return loc


def _dataset(folder, fmt, resident, workers, seed=7, on=True, spatial=False, batch=2):
    import bts_amd  # noqa: F401
    from bts_amd import data
    cfg = data.IntensityConfig(noise_prob=0.5, blur_prob=0.6, blur_sigma=(0.5, 1.5), blur_channel_prob=0.7, brightness_prob=0.5,
                               contrast_prob=0.5, gamma_prob=0.6, gamma_invert_prob=0.4) if on else None
    sp = data.SpatialConfig(0.6, rotate_deg=(20, 10, 30), zoom=(0.8, 1.25), elastic_sigma=1.5, elastic_spacing=4) if spatial else None
    return data.prepare_dataset(folder, batch, SIZE, list(CROP), 3, shuffle=True, data_format=fmt, seed=seed, device=dev(),
                                resident_bytes=resident, workers=workers, spatial=sp, intensity=cfg)[0]


def _same(a, b):
    assert len(a) == len(b)
    for (xa, ya), (xb, yb) in zip(a, b):
        assert torch.equal(xa, xb) and torch.equal(ya, yb)


@pytest.mark.parametrize('spatial', [False, True], ids=['alone', 'with_spatial'])
@pytest.mark.parametrize('fmt', ['channels_last', 'channels_first'])
def test_dataset_batches_do_not_depend_on_the_path(folder, fmt, spatial):
    """reproducible for a seed, the same for (resident_bytes, workers) in {(0,0), (big,0), (big,2)}: per-example and batched paths"""
    runs = [[b for _ in range(2) for b in _dataset(folder, fmt, r, w, spatial=spatial)]
            for r, w in ((0, 0), (0, 0), (1 << 30, 0), (1 << 30, 2))]
    shape = (2, 2) + CROP if fmt == 'channels_first' else (2,) + CROP + (2,)
    assert [tuple(b[0].shape) for b in runs[0][:3]] == [shape, shape, (1,) + shape[1:]]
    for other in runs[1:]:
        _same(runs[0], other)
    # the transform is really there, and another seed gives other batches; the first example of an epoch has the crop and flips of a
    # run without the config (its draw() comes first on the generator either way) and its labels are not touched
    plain = [b for _ in range(2) for b in _dataset(folder, fmt, 0, 0, on=False, spatial=False)]
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(runs[0], plain))
    if not spatial:
        assert torch.equal(runs[0][0][1][0], plain[0][1][0])
    other = list(_dataset(folder, fmt, 0, 0, seed=8, spatial=spatial))
    assert any(not torch.equal(a[0], b[0]) for a, b in zip(runs[0], other))


def test_dataset_state_dict_resumes_bit_exactly(folder):
    a = _dataset(folder, 'channels_last', 1 << 30, 2, batch=3, spatial=True)
    assert len(list(a)) == 2
    st = a.state_dict()
    assert sorted(st) == ['gen', 'order_gen']
    want = list(a) + list(a)
    b = _dataset(folder, 'channels_last', 0, 0, batch=3, spatial=True)
    b.load_state_dict(st)
    _same(list(b) + list(b), want)


# ---- status codes -----------------------------------------------------------------------------------------------------------------
def test_status_codes_without_a_launch():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    n, c = 2, 2
    P = lambda a: ctypes.cast(a, ctypes.c_void_p) if a is not None else None      # noqa: E731
    x = ctypes.c_void_p(256)                              # (never dereferenced on the host, never reached by a refused call)
    keys = (ctypes.c_uint32 * (2 * n))(1, 2, 3, 4)
    good = [(63, 0.1, 1.0, 1.1, 0.9, 1.2)] * (n * c)

    def call(N=n, T=(8, 8, 8), C=c, layout=0, x=x, entries=good, keys=keys, ws=x, nbytes=None, flags='from entries', params='from entries'):
        fl = (ctypes.c_int * len(entries))(*[e[0] for e in entries]) if flags == 'from entries' else flags
        pr = (ctypes.c_float * (5 * len(entries)))(*[v for e in entries for v in e[1:]]) if params == 'from entries' else params
        if nbytes is None:
            nbytes = 1 << 40
        return L._bts_intensity_batch(x, N, T[0], T[1], T[2], C, layout, P(fl), P(pr), P(keys), ws, nbytes, None)
    SHAPE = -1
    assert L._bts_intensity_batch_workspace(n, 8, 8, 8, c) >= n * c * 512 * 4
    assert L._bts_intensity_batch_workspace(0, 8, 8, 8, c) < 0 and L._bts_intensity_batch_workspace(n, 8, 0, 8, c) < 0
    assert L._bts_intensity_batch_workspace(n, 8, 8, 8, 17) < 0
    assert call(N=0) == SHAPE and call(N=-3) == SHAPE
    assert call(C=0) == SHAPE and call(C=17) == SHAPE
    assert call(T=(0, 8, 8)) == SHAPE and call(T=(8, -1, 8)) == SHAPE and call(T=(8, 8, 0)) == SHAPE
    assert call(layout=2) == SHAPE and call(layout=-1) == SHAPE
    assert call(x=None) == SHAPE and call(flags=None) == SHAPE and call(params=None) == SHAPE and call(keys=None) == SHAPE
    assert call(ws=None) == SHAPE and call(nbytes=L._bts_intensity_batch_workspace(n, 8, 8, 8, c) - 1) == SHAPE
    inf, nan = float('inf'), float('nan')

    def entry(at, value, flags=63):
        e = list(good[0])
        e[0], e[at] = flags, value
        return [good[0]] * (n * c - 1) + [tuple(e)]
    for bad in (-0.01, inf, nan):
        assert call(entries=entry(1, bad)) == SHAPE                       # s
    for bad in (0.0, -1.0, nan, inf, 4.2):
        assert call(entries=entry(2, bad)) == SHAPE                       # sigma <= 0, or r > 16
    for at in (3, 4, 5):
        for bad in (0.0, -0.5, inf, nan):
            assert call(entries=entry(at, bad)) == SHAPE                  # m, f, gamma
    assert call(entries=entry(1, 0.1, flags=64)) == SHAPE and call(entries=entry(1, 0.1, flags=-1)) == SHAPE
    # the wrapper refuses by name what it can see
    ops = _ops()
    t = torch.zeros((1, 4, 4, 4, 2), device=dev())
    row = [[(0, 0, 1, 1, 1, 1)] * 2]
    ops.intensity_batch(t, row, [(0, 0)])
    for args in ((t.cpu(), row, [(0, 0)]), (t.double(), row, [(0, 0)]), (t[0], row, [(0, 0)]), (t, row * 2, [(0, 0)]), (t, row, [(0, 0)] * 2),
                 (t, [[(0, 0, 1, 1, 1, 1)]], [(0, 0)]), (t, [[(0, 0, 1, 1, 1)] * 2], [(0, 0)]), (t, row, [(0,)]),
                 (t[..., :1], [[(0, 0, 1, 1, 1, 1)]], [(0, 0)])):
        with pytest.raises((ValueError, RuntimeError)):
            ops.intensity_batch(*args)
    with pytest.raises(RuntimeError, match='BTS_ERR_SHAPE'):
        ops.intensity_batch(t, [[(IR.GAMMA, 0, 1, 1, 1, -1.0)] * 2], [(0, 0)])
    # a stage that is off does not look at its number
    ops.intensity_batch(t, [[(IR.BRIGHT, -1.0, -1.0, 1.1, nan, 0.0)] * 2], [(0, 0)])
    torch.cuda.synchronize()


# ---- the command ------------------------------------------------------------------------------------------------------------------
def test_command_trains_with_the_flag_and_validates_without(tmp_path, monkeypatch):
    """python -m bts_amd.train --intensity_aug: the training set carries the config, the validation set none and its batches are those
    of a run without the flag; train.log is finite, train_args.pkl keeps the flags"""
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
    for flags in (['--intensity_aug', '--noise_prob', '1', '--blur_prob', '1', '--brightness_prob', '1', '--contrast_prob', '1',
                   '--gamma_prob', '1'], []):
        del made[:]
        out = os.path.join(loc, 'run%d' % len(flags))
        _base.set_seed(0)
        res = T.run(T.parse_args(['--train_loc', os.path.join(loc, 'train'), '--val_loc', os.path.join(loc, 'val'), '--prepro_loc',
                                  os.path.join(loc, 'prepro.npy'), '--save_folder', out, '--crop_size', '16,16,16', '--base_filters', '16',
                                  '--groups', '4', '--reduction', '4', '--depth', '3', '--batch_size', '2', '--n_epochs', '1',
                                  '--workers', '0'] + flags))
        train_set, val_set = made
        assert val_set.intensity is None and (train_set.intensity is not None) == bool(flags)
        assert all(np.isfinite(float(v)) for v in res['history'][0].values())
        stored = T.load_train_args(out)
        assert stored['intensity_aug'] is bool(flags) and stored['gamma_prob'] == (1.0 if flags else 0.3)
        val_set.load_state_dict({'order_gen': torch.Generator().manual_seed(0).get_state(),
                                 'gen': torch.Generator().manual_seed(7919).get_state()})
        val_batches.append(list(val_set))
    _same(val_batches[0], val_batches[1])
