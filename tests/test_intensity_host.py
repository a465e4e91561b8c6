"""CPU: the float64 restatement of the intensity augmentation (tests/intensity_ref.py) against known answers and scipy, the draws of
data.draw_intensity, the command's flags, and the conditions on the tolerances tests/test_intensity_gpu.py uses."""
import os
import pickle

import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import intensity_ref as IR


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    ones = 0xffffffff
    for counter, key, want in (((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
                               ((ones,) * 4, (ones, ones), '408f276d 41c83b0e a20bc7c6 6d5451fd'),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                                'd16cfe09 94fdcceb 5001e420 24126ea1')):
        got = ' '.join('%08x' % int(w[0]) for w in IR.philox(counter, key))
        assert got == want


def test_normals_have_mean_0_and_variance_1():
    n = 1 << 20
    z = IR.normals((0x1234abcd, 0x9e3779b9), n)
    print('mean %.3e  variance %.5f' % (z.mean(), z.var()))
    assert abs(z.mean()) <= 4.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 0.01
    # element e is word e & 3 of block e >> 2: the first four are one block's two Box-Muller pairs
    w = [int(v[0]) for v in IR.philox((0, 0, 0, 0), (0x1234abcd, 0x9e3779b9))]
    u1, u2 = ((w[2] >> 8) + 1) * 2.0 ** -24, (w[3] >> 8) * 2.0 ** -24
    assert z[3] == pytest.approx(np.sqrt(-2 * np.log(u1)) * np.sin(2 * np.pi * u2), abs=1e-15)
    z32 = IR.normals32((0x1234abcd, 0x9e3779b9), n)
    print('float32 restatement vs float64: %.2e' % np.abs(z32 - z).max())
    assert np.abs(z32 - z).max() <= 8e-6


@pytest.mark.parametrize('shape,sigma', [((3, 5, 4), 1.3), ((9, 10, 11), 0.5), ((9, 10, 11), 1.0), ((4, 7, 33), 2.2), ((2, 1, 3), 4.1)])
def test_blur_is_scipy_gaussian_filter(shape, sigma):
    v = np.random.RandomState(3).randn(*shape)
    r, w = IR.blur_weights(sigma)
    assert r == int(4 * sigma + 0.5) and len(w) == r + 1 and (w[0] + 2 * w[1:].sum()) == pytest.approx(1.0, abs=1e-15)
    err = np.abs(IR.blur(v, sigma) - ndi.gaussian_filter(v, sigma)).max()
    print('r = %d, extents %s: %.2e' % (r, shape, err))
    assert err <= 1e-12


def test_library_weights_are_the_restatement_s():
    """bts_intensity_blur_weights is host code: the float64 normalisation, rounded to float32"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    sigmas = [e[2] for si in range(len(IR.SHAPES)) for row in IR.case(si, 'blur').params for e in row] + [0.5, 1.0, 4.1]
    for sigma in sigmas:
        r, w = ops.intensity_blur_weights(sigma)
        r64, w64 = IR.blur_weights(float(np.float32(sigma)))
        assert r == r64 and np.array_equal(np.array(w, np.float32), w64.astype(np.float32))
    for bad in (0.0, -1.0, float('nan'), float('inf'), 4.2):
        with pytest.raises(ValueError):
            ops.intensity_blur_weights(bad)


def test_chain_on_a_constant_volume_and_without_flags():
    v = np.full((4, 5, 6), 3.25)
    for flags in (IR.CONTRAST, IR.GAMMA, IR.GAMMA | IR.INVERT, IR.CONTRAST | IR.GAMMA):
        assert np.abs(IR.chain(v, (flags, 0.1, 1.0, 1.1, 0.8, 1.3), None) - v).max() <= 1e-12
        assert np.abs(IR.chain32(v, (flags, 0.1, 1.0, 1.1, 0.8, 1.3), None) - v).max() <= 1e-6
    assert np.array_equal(IR.chain(v, (0, 0.1, 1.0, 1.1, 0.8, 1.3), None), v)


# ---- the tolerances of the GPU test ---------------------------------------------------------------------------------------------------
def test_cases_cover_every_flag_both_sides_and_invert():
    assert IR.blur_weights(min(e[2] for row in IR.case(0, 'blur').params for e in row))[0] > max(IR.SHAPES[0][0])
    crop = IR.SHAPES[4][0]
    assert crop[0] * crop[1] * crop[2] > 64 * 256          # the statistics' second round
    for si in range(len(IR.SHAPES)):
        for kind in ('contrast', 'gamma', 'chain'):
            es = [e for row in IR.case(si, kind).params for e in row]
            at = 4 if kind == 'contrast' else 5
            on = IR.CONTRAST if kind == 'contrast' else IR.GAMMA
            if kind != 'gamma':
                assert any(e[0] & IR.CONTRAST and e[4] < 1 for e in es) and any(e[0] & IR.CONTRAST and e[4] > 1 for e in es)
            if kind != 'contrast':
                assert any(e[0] & IR.GAMMA and e[5] < 1 for e in es) and any(e[0] & IR.GAMMA and e[5] > 1 for e in es)
                assert any(e[0] & IR.INVERT for e in es) and any(e[0] & IR.GAMMA and not e[0] & IR.INVERT for e in es)
            assert all(e[at] > 0 for e in es if e[0] & on)
        flags = 0
        for row in IR.case(si, 'chain').params:
            for e in row:
                flags |= e[0]
        assert flags == 63
        assert all(all(float(np.float32(v)) == v for v in e[1:]) for k in IR.KINDS for row in IR.case(si, k).params for e in row)


@pytest.mark.parametrize('si', range(len(IR.SHAPES)))
def test_tolerance_conditions(si):
    """contrast, gamma and the chain: 4 x the float32 restatement's distance from float64 (+ 4 x 2^-24 of the range where powf acts)
    must stay under 1e-4 (contrast) / 1e-3 (gamma, chain) of the range of every result volume, and must not be empty"""
    for kind, cap in (('contrast', 1e-4), ('gamma', 1e-3), ('chain', 1e-3)):
        cs = IR.case(si, kind)
        gap, bound, rng = cs.restatement_gap(), cs.bound(), cs.ranges()
        print('%s %s C%d: float32 restatement within %.3e of float64 = %.3e of the smallest range; bound / range at most %.3e'
              % (kind, cs.crop, cs.c, gap, gap / rng.min(), (bound / rng).max()))
        assert gap > 0.0 and np.all(rng > 0.0)
        assert np.all(bound <= cap * rng)
    for kind in ('noise', 'blur'):
        cs = IR.case(si, kind)
        gap, bound = np.abs(cs.ref32().astype(np.float64) - cs.ref()).max(axis=(1, 2, 3)), cs.bound()
        print('%s %s C%d: float32 restatement uses at most %.2f of the bound' % (kind, cs.crop, cs.c, (gap / bound).max()))
        assert np.all(gap <= bound)          # (the documented order of operations itself fits the issue's formula)
        assert np.all(bound <= 2e-4 * np.abs(cs.ref()).max())


# ---- the draws -------------------------------------------------------------------------------------------------------------------------
def _data():
    import bts_amd  # noqa: F401
    from bts_amd import data
    return data


def test_draw_order_and_count():
    data = _data()
    from bts_amd import ops
    cfg = data.IntensityConfig(noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5, gamma_prob=0.5,
                               gamma_invert_prob=0.5, contrast=(0.6, 1.4), gamma=(0.5, 2.0))
    c = 3
    gen, replay = torch.Generator().manual_seed(11), torch.Generator().manual_seed(11)
    seen = 0
    for _ in range(40):
        d = data.draw_intensity(gen, cfg, c)
        u = torch.rand(6 + 8 * c, generator=replay, dtype=torch.float64).tolist()
        key = torch.randint(0, 2 ** 32, (2,), generator=replay, dtype=torch.int64).tolist()
        assert torch.equal(gen.get_state(), replay.get_state())           # the same count whatever the values are
        assert d.key == (key[0], key[1]) and len(d.params) == c
        on = [u[k] < 0.5 for k in range(5)]
        for j, e in enumerate(d.params):
            v = u[6 + 8 * j:14 + 8 * j]
            want = ((ops.INTENSITY_NOISE if on[0] else 0) | (ops.INTENSITY_BLUR if on[1] and v[1] < 0.5 else 0) |
                    (ops.INTENSITY_BRIGHT if on[2] else 0) | (ops.INTENSITY_CONTRAST if on[3] else 0) |
                    (ops.INTENSITY_GAMMA if on[4] else 0) | (ops.INTENSITY_INVERT if on[4] and u[5] < 0.5 else 0))
            assert e[0] == want
            seen |= e[0]
            assert e[1] == 0.0 + v[0] * 0.1 and e[2] == 0.5 + v[2] * 0.5 and e[3] == 0.75 + v[3] * 0.5
            assert e[4] == (0.6 + v[5] * (1.0 - 0.6) if v[4] < 0.5 else 1.0 + v[5] * (1.4 - 1.0))
            assert e[5] == (0.5 + v[7] * (1.0 - 0.5) if v[6] < 0.5 else 1.0 + v[7] * (2.0 - 1.0))
    assert seen == 63
    # a range entirely above 1 never takes the lower side
    hi = data.IntensityConfig(contrast_prob=1.0, contrast=(1.2, 1.5))
    assert all(1.2 <= e[4] <= 1.5 for _ in range(20) for e in data.draw_intensity(gen, hi, 2).params)
    # the defaults are nnU-Net's
    d = data.IntensityConfig()
    assert (d.noise_prob, d.noise_sigma, d.blur_prob, d.blur_sigma, d.blur_channel_prob) == (0.1, (0.0, 0.1), 0.2, (0.5, 1.0), 0.5)
    assert (d.brightness_prob, d.brightness, d.contrast_prob, d.contrast) == (0.15, (0.75, 1.25), 0.15, (0.75, 1.25))
    assert (d.gamma_prob, d.gamma, d.gamma_invert_prob) == (0.3, (0.7, 1.5), 0.1)


def test_constructor_refusals():
    data = _data()
    for bad in (dict(noise_prob=-0.1), dict(noise_prob=1.5), dict(blur_prob=2), dict(blur_channel_prob=-1), dict(brightness_prob=1.01),
                dict(contrast_prob=float('nan')), dict(gamma_prob=-1e-9), dict(gamma_invert_prob=3), dict(noise_prob='x'),
                dict(noise_sigma=(-0.1, 0.1)), dict(noise_sigma=(0.2, 0.1)), dict(noise_sigma=(0.0, float('inf'))), dict(noise_sigma=0.1),
                dict(blur_sigma=(0.0, 1.0)), dict(blur_sigma=(1.0, 0.5)), dict(blur_sigma=(0.5, 4.2)), dict(blur_sigma=(0.5, 1.0, 2.0)),
                dict(brightness=(0.0, 1.0)), dict(brightness=(1.2, 0.8)), dict(contrast=(-1.0, 1.0)), dict(contrast=(1.5, 1.0)),
                dict(gamma=(0.0, 1.5)), dict(gamma=(2.0, 1.0)), dict(gamma=(0.7, float('nan')))):
        with pytest.raises(ValueError):
            data.IntensityConfig(**bad)
    data.IntensityConfig(noise_sigma=(0.0, 0.0), blur_sigma=(4.1, 4.1), noise_prob=0, gamma_invert_prob=1)


def test_none_leaves_the_generator_where_the_parent_s_loop_does(tmp_path, monkeypatch):
    """intensity=None: draw() alone moves the generator, on both iteration paths; with a config draw_intensity() follows every draw()"""
    data = _data()
    size, crop = (10, 12, 9, 2), (8, 8, 8)
    for i in range(3):
        np.savez(os.path.join(str(tmp_path), 'e%d.npz' % i), x=np.zeros(size, np.float32), y=np.zeros(size[:3] + (1,), np.float32))
    calls = []

    def fake_batch(xs, ys, var, crop_size, offsets, masks, shifts, scales, out_ch, cf=False, out=None):
        z = torch.zeros((len(xs),) + tuple(crop_size) + (2,))
        return z, z

    def fake_intensity(x, params, keys, channels_first=False):
        calls.append((x.shape[0], [list(p) for p in params], list(keys), channels_first))
        return x
    monkeypatch.setattr(data.ops, 'augment_batch', fake_batch)
    monkeypatch.setattr(data.ops, 'augment_crop', lambda x, y, var, crop_size, *a: (torch.zeros(tuple(crop_size) + (2,)),) * 2)
    monkeypatch.setattr(data.ops, 'channel_moments', lambda x: (None, None))
    monkeypatch.setattr(data.ops, 'intensity_batch', fake_intensity)
    cfg = data.IntensityConfig(noise_prob=0.5, blur_prob=0.5, brightness_prob=0.5, contrast_prob=0.5, gamma_prob=0.5)
    seen = []
    for resident, workers in ((0, 0), (1 << 20, 0)):
        ds, _ = data.prepare_dataset(str(tmp_path), 2, size, crop, 3, seed=5, device=torch.device('cpu'), rank=0, world=1,
                                     resident_bytes=resident, workers=workers)
        assert ds.intensity is None
        list(ds)
        alone = torch.Generator().manual_seed(5 + 7919)
        for _ in range(3):
            data.draw(alone, 2, size[:3], crop)
        assert torch.equal(ds.gen.get_state(), alone.get_state()) and not calls
        ds, _ = data.prepare_dataset(str(tmp_path), 2, size, crop, 3, seed=5, device=torch.device('cpu'), rank=0, world=1,
                                     resident_bytes=resident, workers=workers, intensity=cfg)
        list(ds)
        both, want = torch.Generator().manual_seed(5 + 7919), []
        for _ in range(3):
            data.draw(both, 2, size[:3], crop)
            want.append(data.draw_intensity(both, cfg, 2))
        assert torch.equal(ds.gen.get_state(), both.get_state())
        assert sorted(ds.state_dict()) == ['gen', 'order_gen']
        assert [p for _, ps, _, _ in calls for p in ps] == [d.params for d in want]
        assert [k for _, _, ks, _ in calls for k in ks] == [d.key for d in want]
        seen.append([n for n, _, _, _ in calls])
        del calls[:]
    assert seen == [[1, 1, 1], [2, 1]]


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 3}, 'norm': {'mean': np.zeros(3), 'std': np.ones(3)}}, allow_pickle=True)
    return path


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + list(more)


ALL = ['--intensity_aug', '--noise_prob', '0.2', '--noise_sigma', '0.01,0.2', '--blur_prob', '0.3', '--blur_sigma', '0.6,1.5',
       '--blur_channel_prob', '0.7', '--brightness_prob', '0.25', '--brightness_range', '0.8,1.2', '--contrast_prob', '0.35',
       '--contrast_range', '0.7,1.4', '--gamma_prob', '0.4', '--gamma_range', '0.6,1.8', '--gamma_invert_prob', '0.2']


def test_flags_parse_with_their_defaults(prepro):
    import bts_amd  # noqa: F401
    from bts_amd import data, train as T
    a = T.parse_args(_argv(prepro))
    assert a.intensity_aug is False and T.intensity_config(a) is None                      # off by default
    assert set(T.INTENSITY_KEYS) <= set(vars(a))
    d = T.intensity_config(T.parse_args(_argv(prepro, '--intensity_aug')))
    assert vars(d) == vars(data.IntensityConfig())                                           # the flags' defaults are the config's
    cfg = T.intensity_config(T.parse_args(_argv(prepro, *ALL)))
    assert (cfg.noise_prob, cfg.noise_sigma, cfg.blur_prob, cfg.blur_sigma, cfg.blur_channel_prob) == (0.2, (0.01, 0.2), 0.3, (0.6, 1.5), 0.7)
    assert (cfg.brightness_prob, cfg.brightness, cfg.contrast_prob, cfg.contrast) == (0.25, (0.8, 1.2), 0.35, (0.7, 1.4))
    assert (cfg.gamma_prob, cfg.gamma, cfg.gamma_invert_prob) == (0.4, (0.6, 1.8), 0.2)
    for bad in (['--noise_sigma', '0.1'], ['--blur_sigma', 'a,b'], ['--gamma_range', '1,2,3'], ['--intensity_aug', '--noise_prob', '1.5'],
                ['--intensity_aug', '--blur_sigma', '0.5,5'], ['--intensity_aug', '--gamma_range', '1.5,0.7'],
                ['--intensity_aug', '--contrast_range', '0,1'], ['--intensity_aug', '--brightness_range=-1,1']):
        with pytest.raises(ValueError):
            T.parse_args(_argv(prepro, *bad))
    # arg_parser() itself is untouched
    assert not any(k in vars(T.arg_parser().parse_args(_argv(prepro))) for k in T.INTENSITY_KEYS)


def test_flags_round_trip_through_train_args_and_an_old_pickle_is_off(prepro, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    out = os.path.join(str(tmp_path), 'run')
    a = T.parse_args(_argv(prepro, '--save_folder', out, '--base_filters', '16', '--groups', '4', *ALL))
    stored = T.load_train_args(out)
    assert stored['intensity_aug'] is True and stored['gamma_range'] == [0.6, 1.8] and stored['blur_channel_prob'] == 0.7
    b = T.parse_args(_argv(prepro, '--load_folder', out, '--gamma_prob', '0.9'))             # the folder decides
    assert {k: getattr(b, k) for k in T.INTENSITY_KEYS} == {k: getattr(a, k) for k in T.INTENSITY_KEYS}
    assert T.intensity_config(b).gamma == (0.6, 1.8)
    off = os.path.join(str(tmp_path), 'off')
    T.parse_args(_argv(prepro, '--save_folder', off, '--base_filters', '16', '--groups', '4'))
    assert T.intensity_config(T.parse_args(_argv(prepro, '--load_folder', off, '--intensity_aug'))) is None
    # a pickle from before the flags existed
    old = os.path.join(str(tmp_path), 'old')
    os.makedirs(old)
    with open(os.path.join(old, T.ARGS_NAME), 'wb') as f:
        pickle.dump({'model_args': a.model_args, 'crop_size': [16, 16, 16]}, f)
    c = T.parse_args(_argv(prepro, '--load_folder', old, '--intensity_aug'))
    assert c.intensity_aug is False and T.intensity_config(c) is None and c.crop_size == [16, 16, 16]


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
    for flags, want in ((['--intensity_aug', '--gamma_prob', '0.6'], (True, False)), ([], (False, False)),
                        (['--intensity_aug', '--spatial_prob', '0.5'], (True, True))):
        del calls[:]
        with pytest.raises(Stop):
            T.run(T.parse_args(_argv(prepro, '--resident_gb', '0', *flags)))
        (tr, ktr), (va, kva) = calls
        assert (tr, va) == ('tr', 'va') and 'intensity' not in kva and 'spatial' not in kva
        assert ('intensity' in ktr, 'spatial' in ktr) == want
        if want[0]:
            assert isinstance(ktr['intensity'], data.IntensityConfig)
    assert ktr['intensity'].gamma_prob == 0.3
