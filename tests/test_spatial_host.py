"""No GPU: the float64 restatement of the spatial augmentation (tests/spatial_ref.py) against scipy.ndimage.map_coordinates, the draws
of data.draw_spatial, the matrix, the command-line flags, and the two tolerance conditions tests/test_spatial_gpu.py relies on."""
import os
import pickle

import numpy as np
import pytest
import torch

import spatial_ref as SR


def _data():
    import bts_amd  # noqa: F401
    from bts_amd import data
    return data


# ---- the restatement against scipy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['affine', 'both'])
@pytest.mark.parametrize('si', range(len(SR.SHAPES)))
def test_restatement_agrees_with_scipy_at_its_coordinates(si, mode):
    from scipy import ndimage
    cs = SR.case(si, mode)
    for d in (0, 3):
        dr = cs.draws[d]
        x, y = cs.xs[d].astype(np.float64), cs.ys[d][..., 0].astype(np.float64)
        s = SR.coordinates(cs.crop, dr['offsets'], dr['M'], dr['phi'], dr['spacing'])
        co = np.moveaxis(s, -1, 0)
        got = SR.sample_linear(x, s, np.zeros(cs.c))
        for c in range(cs.c):
            want = ndimage.map_coordinates(x[..., c], co, order=1, mode='grid-constant', cval=0.0)
            assert np.abs(got[..., c] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
        away = ~SR.ties(s)
        want = ndimage.map_coordinates(y, co, order=0, mode='grid-constant', cval=0.0)
        assert np.array_equal(SR.sample_nearest(y, s)[away], want[away])
        assert away.mean() > 0.9


def test_a_nonzero_fill_is_scipys_cval():
    from scipy import ndimage
    cs = SR.case(2, 'affine')
    x = cs.xs[0].astype(np.float64)
    s = SR.coordinates(cs.crop, (0, 0, 0), np.eye(3) / 0.4)
    got = SR.sample_linear(x, s, [-3.5])[..., 0]
    want = ndimage.map_coordinates(x[..., 0], np.moveaxis(s, -1, 0), order=1, mode='grid-constant', cval=-3.5)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert (got == -3.5).any()


def test_identity_and_quarter_turns_of_the_restatement():
    """M = I reproduces the plain crop; a 90 degree turn about `axis` is np.rot90(window, -1, (axis+1, axis+2)) -- the analytic form
    the GPU test checks the kernel against"""
    cs = SR.case(0, 'affine')
    x, y = cs.xs[0], cs.ys[0]
    o, T = (1, 2, 3), 6
    win = x[o[0]:o[0] + T, o[1]:o[1] + T, o[2]:o[2] + T].astype(np.float64)
    s = SR.coordinates((T, T, T), o, np.eye(3))
    assert np.array_equal(SR.sample_linear(x.astype(np.float64), s, [0, 0]), win)
    for axis in range(3):
        M = np.round(SR.rotation(axis, np.pi / 2))
        assert set(np.unique(M)) <= {-1.0, 0.0, 1.0}
        s = SR.coordinates((T, T, T), o, M)
        assert np.array_equal(s, np.round(s))
        got = SR.sample_linear(x.astype(np.float64), s, [0, 0])
        assert np.array_equal(got, np.rot90(win, -1, ((axis + 1) % 3, (axis + 2) % 3)))


# ---- the draws ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sigma', [0.0, 2.0])
@pytest.mark.parametrize('prob', [0.0, 0.5, 1.0])
def test_draw_spatial_consumes_the_documented_values_in_order(prob, sigma):
    data = _data()
    crop = (12, 10, 15)
    cfg = data.SpatialConfig(prob, rotate_deg=(10, 20, 30), zoom=(0.8, 1.3), elastic_sigma=sigma, elastic_spacing=4)
    G = data.control_grid(crop, 4)
    assert G == (6, 6, 7)
    gen, replay = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    for _ in range(4):
        sd = data.draw_spatial(gen, cfg, crop)
        u = torch.rand(5, generator=replay, dtype=torch.float64).tolist()        # prob, three angles, zoom
        normals = torch.randn(G + (3,), generator=replay, dtype=torch.float32) if sigma > 0 else None      # 3 G0 G1 G2 of them
        assert torch.equal(gen.get_state(), replay.get_state())                  # the same position, whatever the outcome
        assert sd.on == (u[0] < prob)
        want_angles = [np.deg2rad((2 * u[1 + k] - 1) * (10, 20, 30)[k]) for k in range(3)]
        want_zoom = 0.8 + u[4] * 0.5
        assert np.allclose(sd.angles, want_angles, rtol=0, atol=1e-15) and abs(sd.zoom - want_zoom) < 1e-15
        if sd.on:
            assert np.array_equal(sd.matrix, data.spatial_matrix(want_angles, want_zoom))
            assert np.allclose(sd.matrix, SR.matrix(want_angles, want_zoom), rtol=0, atol=1e-15)
            if sigma > 0:
                assert sd.phi.dtype == torch.float32 and tuple(sd.phi.shape) == G + (3,) and torch.equal(sd.phi, normals * sigma)
            else:
                assert sd.phi is None
        else:
            assert np.array_equal(sd.matrix, np.eye(3)) and sd.phi is None
        assert sd.spacing == 4


def test_matrix_is_orthogonal_up_to_the_zoom():
    data = _data()
    rs = np.random.RandomState(3)
    for _ in range(20):
        a, z = np.deg2rad(rs.uniform(-180, 180, 3)), rs.uniform(0.5, 2.0)
        M = data.spatial_matrix(a, z)
        assert M.dtype == np.float64
        assert np.abs(M.dot(M.T) * z * z - np.eye(3)).max() < 1e-14
        assert abs(np.linalg.det(M) * z ** 3 - 1.0) < 1e-13
    # one axis at a time: the rotation leaves its own axis alone; z > 1 magnifies (a step of one output voxel is 1/z source voxels)
    for axis in range(3):
        ang = [0.0, 0.0, 0.0]
        ang[axis] = 0.3
        M = data.spatial_matrix(ang, 2.0)
        e = np.eye(3)[axis]
        assert np.allclose(M.dot(e), e / 2.0, rtol=0, atol=1e-16)


class _Files(object):
    """a dataset over no files at all: only the draws are exercised"""


def test_without_a_config_not_one_extra_value_is_drawn(tmp_path, monkeypatch):
    """spatial=None: the generator after an epoch of either path is where a plain draw() loop leaves it"""
    data = _data()
    size, crop = (10, 12, 9, 2), (8, 8, 8)
    for i in range(3):
        np.savez(os.path.join(str(tmp_path), 'e%d.npz' % i), x=np.zeros(size, np.float32), y=np.zeros(size[:3] + (1,), np.float32))
    calls = []
    monkeypatch.setattr(data, 'augment_example', lambda x, y, crop_size, out_ch, dr: (calls.append('ex'), (x, y))[1])
    monkeypatch.setattr(data.ops, 'augment_batch', lambda xs, *a, **k: (calls.append('batch'), (xs[0], xs[0]))[1])
    monkeypatch.setattr(data.ops, 'channel_moments', lambda x: (None, None))
    monkeypatch.setattr(data.ops, 'augment_spatial_batch', lambda *a, **k: pytest.fail('spatial launch without a config'))
    monkeypatch.setattr(data, 'draw_spatial', lambda *a, **k: pytest.fail('spatial draw without a config'))
    for resident, workers in ((0, 0), (1 << 20, 0)):
        ds, n = data.prepare_dataset(str(tmp_path), 2, size, crop, 3, seed=5, device=torch.device('cpu'), rank=0, world=1,
                                     resident_bytes=resident, workers=workers)
        assert n == 3 and ds.spatial is None
        list(ds)
        plain = torch.Generator().manual_seed(5 + 7919)
        for _ in range(3):
            data.draw(plain, 2, size[:3], crop)
        assert torch.equal(ds.gen.get_state(), plain.get_state())
    assert 'ex' in calls and 'batch' in calls


def test_with_a_config_every_example_draws_both_on_either_path(tmp_path, monkeypatch):
    data = _data()
    size, crop = (10, 12, 9, 2), (8, 8, 8)
    for i in range(3):
        np.savez(os.path.join(str(tmp_path), 'e%d.npz' % i), x=np.zeros(size, np.float32), y=np.zeros(size[:3] + (1,), np.float32))
    cfg = data.SpatialConfig(0.5, elastic_sigma=1.0, elastic_spacing=4)
    seen = []

    def fake(xs, ys, var, crop_size, offsets, masks, shifts, scales, out_ch, spatial, matrices, phis, spacings, fills, cf):
        seen.append((len(xs), list(spatial), [m for m in matrices]))
        z = torch.zeros((len(xs),) + tuple(crop_size) + (2,))
        return z, z
    monkeypatch.setattr(data.ops, 'augment_spatial_batch', fake)
    monkeypatch.setattr(data.ops, 'channel_moments', lambda x: (None, None))
    states = []
    for resident, workers in ((0, 0), (1 << 20, 0)):
        ds, _ = data.prepare_dataset(str(tmp_path), 2, size, crop, 3, seed=5, device=torch.device('cpu'), rank=0, world=1,
                                     resident_bytes=resident, workers=workers, spatial=cfg)
        list(ds)
        both = torch.Generator().manual_seed(5 + 7919)
        for _ in range(3):
            data.draw(both, 2, size[:3], crop)
            data.draw_spatial(both, cfg, crop)
        assert torch.equal(ds.gen.get_state(), both.get_state())
        assert sorted(ds.state_dict()) == ['gen', 'order_gen']
        states.append(seen[:])
        del seen[:]
    assert [n for n, _, _ in states[0]] == [1, 1, 1] and [n for n, _, _ in states[1]] == [2, 1]
    flat = lambda runs: [(f, m) for _, fs, ms in runs for f, m in zip(fs, ms)]      # noqa: E731
    assert flat(states[0]) == flat(states[1])


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 3}, 'norm': {'mean': np.zeros(3), 'std': np.ones(3)}}, allow_pickle=True)
    return path


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + list(more)


def test_flags_parse_with_their_defaults(prepro):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    a = T.parse_args(_argv(prepro))
    assert a.spatial_prob == 0.0 and a.rotate_deg == [15.0, 15.0, 15.0] and a.zoom_range == [0.9, 1.1]
    assert a.elastic_sigma == 0.0 and a.elastic_spacing == 32
    assert T.spatial_config(a) is None                                       # off by default
    b = T.parse_args(_argv(prepro, '--spatial_prob', '0.4', '--rotate_deg', '10,0,25', '--zoom_range', '0.8,1.25', '--elastic_sigma',
                           '3', '--elastic_spacing', '16'))
    cfg = T.spatial_config(b)
    assert (cfg.prob, cfg.rotate_deg, cfg.zoom, cfg.elastic_sigma, cfg.elastic_spacing) == (0.4, (10.0, 0.0, 25.0), (0.8, 1.25), 3.0, 16)
    assert T.spatial_config(T.parse_args(_argv(prepro, '--spatial_prob', '1', '--rotate_deg', '7'))).rotate_deg == (7.0, 7.0, 7.0)
    for bad in (['--rotate_deg', '1,2'], ['--zoom_range', '1'], ['--zoom_range', 'a,b'], ['--spatial_prob', '1.5'],
                ['--spatial_prob', '0.5', '--zoom_range', '1.2,0.8'], ['--spatial_prob', '0.5', '--elastic_spacing', '0']):
        with pytest.raises(ValueError):
            T.parse_args(_argv(prepro, *bad))


def test_flags_round_trip_through_train_args_and_an_old_pickle_is_off(prepro, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    out = os.path.join(str(tmp_path), 'run')
    a = T.parse_args(_argv(prepro, '--save_folder', out, '--spatial_prob', '0.3', '--rotate_deg', '5,6,7', '--elastic_sigma', '2',
                           '--elastic_spacing', '8', '--base_filters', '16', '--groups', '4'))
    stored = T.load_train_args(out)
    assert {k: stored[k] for k in T.SPATIAL_KEYS} == {'spatial_prob': 0.3, 'rotate_deg': [5.0, 6.0, 7.0], 'zoom_range': [0.9, 1.1],
                                                      'elastic_sigma': 2.0, 'elastic_spacing': 8}
    b = T.parse_args(_argv(prepro, '--load_folder', out, '--spatial_prob', '0.9', '--rotate_deg', '1'))      # the folder decides
    assert {k: getattr(b, k) for k in T.SPATIAL_KEYS} == {k: getattr(a, k) for k in T.SPATIAL_KEYS}
    assert T.spatial_config(b).rotate_deg == (5.0, 6.0, 7.0)
    # a pickle from before the flags existed
    old = os.path.join(str(tmp_path), 'old')
    os.makedirs(old)
    with open(os.path.join(old, T.ARGS_NAME), 'wb') as f:
        pickle.dump({'model_args': a.model_args, 'crop_size': [16, 16, 16]}, f)
    c = T.parse_args(_argv(prepro, '--load_folder', old, '--spatial_prob', '0.9'))
    assert c.spatial_prob == 0.0 and T.spatial_config(c) is None and c.crop_size == [16, 16, 16]


def test_only_the_training_set_gets_the_config(prepro, monkeypatch):
    import bts_amd  # noqa: F401
    from bts_amd import data, parallel, train as T
    calls = []

    class Stop(Exception):
        pass

    def fake(loc, *a, **k):
        calls.append((loc, k))
        if len(calls) == 2:
            raise Stop()
        return [], 0
    monkeypatch.setattr(data, 'prepare_dataset', fake)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    monkeypatch.setattr(parallel, 'init_from_env', lambda: None)
    for flags, want in ((['--spatial_prob', '0.5', '--elastic_sigma', '1'], True), ([], False)):
        del calls[:]
        with pytest.raises(Stop):
            T.run(T.parse_args(_argv(prepro, '--resident_gb', '0', *flags)))
        (tr, ktr), (va, kva) = calls
        assert (tr, va) == ('tr', 'va') and 'spatial' not in kva
        assert ('spatial' in ktr) == want
        if want:
            assert isinstance(ktr['spatial'], data.SpatialConfig) and ktr['spatial'].prob == 0.5 and ktr['spatial'].elastic_sigma == 1.0


# ---- the tolerances of the GPU test ---------------------------------------------------------------------------------------------------
def test_flip_masks_cover_all_eight():
    for mode in SR.MODES:
        assert {dr['mask'] for si in range(len(SR.SHAPES)) for dr in SR.case(si, mode).draws} == set(range(8))


def test_intensity_tolerance_condition():
    """delta = 4 x the float32 restatement's worst coordinate error: extents <= 24 here, so a coordinate's float32 spacing is at most
    2^-19 = 1.9e-6 and a handful of roundings stay well under 1e-5; L is not enlarged by the fill border for these volumes, so
    |d value| <= 3 delta L holds for a coordinate error of delta per axis (the trilinear interpolant's slope per axis is at most L)"""
    delta = SR.coordinate_delta()
    print('delta = %.3e voxels' % delta)
    assert 0.0 < delta <= 4e-5
    for si in range(len(SR.SHAPES)):
        cs = SR.case(si, 'affine')
        for x in cs.xs:
            inner, padded = SR.lipschitz(x)
            assert padded <= inner
        for mode in SR.MODES:
            assert all(np.array_equal(a, b) for a, b in zip(cs.xs, SR.case(si, mode).xs))       # the volumes do not depend on the mode
    # the shapes of the kernel's other paths carry their own delta: larger extents, so coarser float32 coordinates (2^-17 at 64..128)
    for i in range(len(SR.EXTRA)):
        cs = SR.case(i, 'both', True)
        d = cs.delta()
        print('extra case %d: delta = %.3e voxels' % (i, d))
        assert 0.0 < d <= 2e-4
        assert all(SR.lipschitz(x)[1] <= SR.lipschitz(x)[0] for x in cs.xs)


def test_label_tie_cap():
    worst = 0.0
    cases = [SR.case(si, mode) for si in range(len(SR.SHAPES)) for mode in SR.MODES] + [SR.case(i, 'both', True) for i in range(len(SR.EXTRA))]
    for cs in cases:
        for dr in cs.draws:
            s = SR.coordinates(cs.crop, dr['offsets'], dr['M'], dr['phi'], dr['spacing'])
            share = float(SR.ties(s).mean())
            worst = max(worst, share)
            assert share <= SR.TIE_CAP, (cs.vol, cs.mode, share)
    print('largest share of tie voxels: %.4f' % worst)
