"""No GPU: the foreground draw (data.draw_foreground) on hand-made tables against tests/sampling_ref.py, ForegroundConfig's validation,
the command-line flags, and the refusals of bts_class_locations and ops.class_locations that need no device."""
import os
import pickle

import numpy as np
import pytest
import torch

import sampling_ref as S


def _data():
    import bts_amd  # noqa: F401
    from bts_amd import data
    return data


VOL = (10, 12, 9)


def _lin(p):
    return (p[0] * VOL[1] + p[1]) * VOL[2] + p[2]


def _table(rows, k):
    """rows: per class the voxels (z, y, x) the table holds, n_c = their number (<= k: stride 1)"""
    loc = np.full((len(rows), k), -1, np.int32)
    for c, ps in enumerate(rows):
        loc[c, :len(ps)] = sorted(_lin(p) for p in ps)
    return [len(ps) for ps in rows], loc


def _with_u(monkeypatch, u):
    """torch.rand answers `u` (and says what it was asked for)"""
    asked = []

    def fake(n, generator=None, dtype=None):
        asked.append((n, dtype))
        assert n == len(u)
        return torch.tensor(u, dtype=torch.float64)
    monkeypatch.setattr(torch, 'rand', fake)
    return asked


# ---- the reference itself ----------------------------------------------------------------------------------------------------------
def test_the_reference_table_on_a_case_done_by_hand():
    y = np.zeros((2, 3, 4), np.float32)
    y.ravel()[[1, 2, 5, 8, 13, 21, 22]] = 1
    y.ravel()[[0, 23]] = 3
    y.ravel()[7] = 4                                       # above out_ch: in no class
    y.ravel()[9] = 1.5
    counts, loc = S.class_locations_ref(y, 3, 3)
    assert counts.tolist() == [7, 0, 2] and counts.dtype == np.int64 and loc.dtype == np.int32
    assert loc.tolist() == [[1, 8, 22], [-1, -1, -1], [0, 23, -1]]       # 7 voxels, capacity 3: stride 3, ranks 0, 3, 6
    assert [S.table_entries(n, 3) for n in (0, 1, 3, 4, 6, 7, 9, 10)] == [(1, 0), (1, 1), (1, 3), (2, 2), (2, 3), (3, 3), (3, 3), (4, 3)]


# ---- draw_foreground ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('prob,rows', [(0.3, [[(5, 6, 4)], [], []]), (1.0, [[(5, 6, 4)], [], [(1, 1, 1)]]), (1.0, [[], [], []])],
                         ids=['mostly_off', 'on', 'on_but_empty'])
def test_three_values_are_taken_in_every_branch(prob, rows):
    data = _data()
    counts, loc = _table(rows, 4)
    cfg = data.ForegroundConfig(prob, samples=4)
    gen, twin = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    ons = set()
    for _ in range(20):
        got = data.draw_foreground(gen, cfg, counts, loc, VOL, (4, 4, 4), [1, 2, 3])
        state = twin.get_state()
        u = torch.rand(3, generator=twin, dtype=torch.float64).tolist()
        assert torch.equal(gen.get_state(), twin.get_state())
        probe = torch.Generator()
        probe.set_state(state)
        assert got == S.draw_foreground_ref(probe, prob, None, counts, loc, VOL, (4, 4, 4), [1, 2, 3])
        on = u[0] < prob and any(counts)
        assert (got != [1, 2, 3]) == on                     # (no voxel of these tables gives the offsets 1, 2, 3)
        ons.add(on)
    assert ons == ({True, False} if prob < 1.0 else {any(counts)})


def test_the_offsets_clamp_at_both_ends_and_centre_an_odd_crop(monkeypatch):
    data = _data()
    cfg = data.ForegroundConfig(1.0, samples=8)
    # (voxel, crop) -> offsets: p - crop // 2, held inside [0, vol - crop]
    for p, crop, want in (((5, 6, 4), (4, 4, 4), [3, 4, 2]), ((0, 0, 0), (4, 4, 4), [0, 0, 0]), ((9, 11, 8), (4, 4, 4), [6, 8, 5]),
                          ((1, 10, 2), (4, 4, 4), [0, 8, 0]), ((5, 6, 4), (5, 3, 7), [3, 5, 1]), ((8, 11, 7), (5, 3, 7), [5, 9, 2]),
                          ((2, 1, 3), (5, 3, 7), [0, 0, 0]), ((5, 6, 4), (10, 12, 9), [0, 0, 0]), ((5, 6, 4), (1, 1, 1), [5, 6, 4])):
        counts, loc = _table([[p]], 8)
        _with_u(monkeypatch, [0.0, 0.0, 0.0])
        got = data.draw_foreground(None, cfg, counts, loc, VOL, crop, [0, 0, 0])
        assert got == want == S.foreground_offsets([0.0, 0.0, 0.0], 1.0, None, counts, loc, VOL, crop, [0, 0, 0]), (p, crop)
        assert all(isinstance(v, int) for v in got)
        # the voxel is inside the crop, at crop // 2 where nothing was clamped
        assert all(0 <= p[a] - got[a] < crop[a] for a in range(3))


def test_only_present_and_allowed_classes_are_picked_and_u_spans_the_table(monkeypatch):
    data = _data()
    rows = [[(0, 0, 0), (9, 11, 8)], [], [(5, 6, 4)], [(1, 1, 1), (2, 2, 2), (3, 3, 3)]]
    counts, loc = _table(rows, 5)
    crop = (1, 1, 1)                                        # offsets = the voxel itself
    below_one = float(np.nextafter(1.0, 0.0))

    def pick(cfg, u):
        _with_u(monkeypatch, u)
        got = data.draw_foreground(None, cfg, counts, loc, VOL, crop, [7, 7, 7])
        assert got == S.foreground_offsets(u, cfg.prob, cfg.classes, counts, loc, VOL, crop, [7, 7, 7])
        return tuple(got)
    every = data.ForegroundConfig(1.0, samples=5)
    # present = [0, 2, 3]: u_class in thirds; class 1 (absent) is never reached
    assert pick(every, [0.0, 0.0, 0.0]) == (0, 0, 0) and pick(every, [0.0, 0.0, below_one]) == (9, 11, 8)
    assert pick(every, [0.5, 0.34, 0.0]) == (5, 6, 4) == pick(every, [0.5, 0.66, below_one])
    assert pick(every, [below_one, 0.67, 0.0]) == (1, 1, 1) and pick(every, [0.0, below_one, 0.34]) == (2, 2, 2)
    assert pick(every, [0.0, below_one, below_one]) == (3, 3, 3)
    some = data.ForegroundConfig(0.5, samples=5, classes=[3, 1])
    assert some.classes == (1, 3)
    assert pick(some, [0.0, 0.0, 0.0]) == (1, 1, 1) == pick(some, [0.49, below_one, 0.0])     # present = [3]
    assert pick(some, [0.5, 0.0, 0.0]) == (7, 7, 7)                                            # u_on = prob: off
    absent = data.ForegroundConfig(1.0, samples=5, classes=[1])
    assert pick(absent, [0.0, 0.0, 0.0]) == (7, 7, 7)                                          # on, nothing to pick: draw()'s offsets
    # a class larger than the table: n_c = 11 voxels at stride 3 -> 4 entries; u_voxel spans those and never reaches the -1 fill
    ps = [(0, 0, i) for i in range(9)] + [(0, 1, 0), (0, 1, 1)]
    counts, loc = S.class_locations_ref(np.isin(np.arange(np.prod(VOL)), [_lin(p) for p in ps]).astype(np.float32), 1, 4)
    assert counts.tolist() == [11] and loc.tolist() == [[0, 3, 6, 9]]
    got = []
    for u in (0.0, 0.25, 0.5, 0.75, below_one):
        _with_u(monkeypatch, [0.0, 0.0, u])
        got.append(data.draw_foreground(None, data.ForegroundConfig(1.0, samples=4), counts.tolist(), loc, VOL, crop, [7, 7, 7]))
    assert got == [[0, 0, 0], [0, 0, 3], [0, 0, 6], [0, 1, 0], [0, 1, 0]]


def test_the_draw_asks_for_three_float64_values(monkeypatch):
    data = _data()
    counts, loc = _table([[(5, 6, 4)]], 2)
    asked = _with_u(monkeypatch, [0.9, 0.0, 0.0])
    assert data.draw_foreground(None, data.ForegroundConfig(0.5), counts, loc, VOL, (4, 4, 4), [1, 2, 3]) == [1, 2, 3]
    assert asked == [(3, torch.float64)]
    assert 'u_on, u_class, u_voxel' in data.draw_foreground.__doc__


# ---- ForegroundConfig --------------------------------------------------------------------------------------------------------------
def test_config_validation():
    data = _data()
    cfg = data.ForegroundConfig(0.33)
    assert (cfg.prob, cfg.samples, cfg.classes) == (0.33, 10000, None) and cfg.allowed(3) == [0, 1, 2]
    assert data.ForegroundConfig(1, samples=1, classes=(2, 0)).allowed(3) == [0, 2]
    for prob in (0.0, -0.1, 1.0001, float('nan'), None, 'x'):
        with pytest.raises(ValueError):
            data.ForegroundConfig(prob)
    for samples in (0, -5, 2.5, None, True, 2 ** 31):
        with pytest.raises(ValueError):
            data.ForegroundConfig(0.5, samples=samples)
    for classes in ([], [-1], [0, 0], [1.5], ['a'], 3, [8]):
        with pytest.raises(ValueError):
            data.ForegroundConfig(0.5, classes=classes)
    # a class outside range(out_ch): refused as soon as out_ch is known -- by the dataset's constructor, without a device
    with pytest.raises(ValueError):
        data.ForegroundConfig(0.5, classes=[3]).allowed(3)
    for cls in (data._Dataset, data._ChannelsFirstDataset):
        with pytest.raises(ValueError):
            cls([], 1, VOL + (2,), (4, 4, 4), 3, False, 0, None, foreground=data.ForegroundConfig(0.5, classes=[0, 3]))
    ds = data._Dataset([], 1, VOL + (2,), (4, 4, 4), 3, False, 0, None)
    assert ds.foreground is None
    assert data._Dataset([], 1, VOL + (2,), (4, 4, 4), 4, False, 0, None, foreground=data.ForegroundConfig(0.5, classes=[0, 3])).foreground


def test_without_a_config_not_one_extra_value_is_drawn_and_with_one_three_per_example(tmp_path, monkeypatch):
    """on either path of the dataset, with the device work stubbed out: the generator ends where a loop of the documented draws ends"""
    data = _data()
    size, crop = VOL + (2,), (4, 4, 4)
    for i in range(3):
        np.savez(os.path.join(str(tmp_path), 'e%d.npz' % i), x=np.zeros(size, np.float32), y=np.zeros(VOL + (1,), np.float32))
    tables = []
    monkeypatch.setattr(data, 'augment_example', lambda x, y, crop_size, out_ch, dr: (x, y))
    monkeypatch.setattr(data.ops, 'augment_batch', lambda xs, *a, **k: (xs[0], xs[0]))
    monkeypatch.setattr(data.ops, 'channel_moments', lambda x: (None, None))

    def table(y, out_ch, k):
        tables.append(k)
        return torch.tensor([1, 0, 0]), torch.tensor(S.class_locations_ref(np.eye(1, y.numel(), 77), out_ch, k)[1])
    monkeypatch.setattr(data.ops, 'class_locations', table)
    cfg = data.ForegroundConfig(0.5, samples=6)
    for fg in (None, cfg):
        for resident, workers in ((0, 0), (1 << 20, 0)):
            del tables[:]
            ds, _ = data.prepare_dataset(str(tmp_path), 2, size, crop, 3, seed=5, device=torch.device('cpu'), rank=0, world=1,
                                         resident_bytes=resident, workers=workers, foreground=fg)
            list(ds)
            list(ds)
            twin = torch.Generator().manual_seed(5 + 7919)
            for _ in range(6):
                data.draw(twin, 2, VOL, crop)
                if fg is not None:
                    torch.rand(3, generator=twin, dtype=torch.float64)
            assert torch.equal(ds.gen.get_state(), twin.get_state())
            assert sorted(ds.state_dict()) == ['gen', 'order_gen']
            assert tables == ([] if fg is None else [6] * (3 if resident else 6))


# ---- the library and the wrapper, as far as they go without a device -----------------------------------------------------------------
def test_the_library_refuses_bad_arguments_before_any_hip_call():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    assert L._bts_class_locations_workspace(240 * 240 * 155, 3) == (3 * ((240 * 240 * 155 + 4095) // 4096) + 16) * 4
    assert L._bts_class_locations_workspace(2 ** 31 - 1, 8) > 0
    assert L._bts_class_locations_workspace(2 ** 31, 3) == -1 and L._bts_class_locations_workspace(0, 3) == -1
    assert L._bts_class_locations_workspace(64, 0) == -1 and L._bts_class_locations_workspace(64, 9) == -1
    buf = (np.zeros(64, np.int64)).ctypes.data                # a host address: never dereferenced by a refused call
    call = L._bts_class_locations
    assert call(buf, buf, buf, buf, 1 << 20, 2 ** 31, 3, 4, None) == -1
    assert call(buf, buf, buf, buf, 1 << 20, 0, 3, 4, None) == -1
    assert call(buf, buf, buf, buf, 1 << 20, 64, 0, 4, None) == -1 and call(buf, buf, buf, buf, 1 << 20, 64, 9, 4, None) == -1
    assert call(buf, buf, buf, buf, 1 << 20, 64, 3, 0, None) == -1
    assert call(None, buf, buf, buf, 1 << 20, 64, 3, 4, None) == -1
    assert call(buf, None, buf, buf, 1 << 20, 64, 3, 4, None) == -1
    assert call(buf, buf, None, buf, 1 << 20, 64, 3, 4, None) == -1
    assert call(buf, buf, buf, None, 1 << 20, 64, 3, 4, None) == -4
    assert call(buf, buf, buf, buf, 75, 64, 3, 4, None) == -4                 # one byte short of (3 * 1 + 16) * 4


class OnGpu(torch.Tensor):
    """a CPU tensor that says it lives on the GPU (tests/test_ops_surface_host.py)"""
    is_cuda = property(lambda self: True)


def test_the_wrapper_refuses_a_bad_tensor_with_value_error_before_the_library(monkeypatch):
    import bts_amd  # noqa: F401
    from bts_amd import ops

    class Reached(Exception):
        pass

    def reached():
        raise Reached()
    monkeypatch.setattr(ops._core, 'lib', reached)
    on = lambda t: t.as_subclass(OnGpu)      # noqa: E731
    bad = [torch.zeros((4, 5, 6)), on(torch.zeros((4, 5, 6), dtype=torch.float64)), on(torch.zeros((4, 5, 12)))[..., ::2],
           on(torch.zeros((4, 5, 6, 2))), on(torch.zeros((5, 6))), on(torch.zeros((0, 5, 6))), np.zeros((4, 5, 6), np.float32)]
    for y in bad:
        with pytest.raises(ValueError):
            ops.class_locations(y, 3, 8)
    good = on(torch.zeros((4, 5, 6, 1)))
    for out_ch, k in ((0, 8), (9, 8), (3, 0), (3.0, 8), (3, 8.5)):
        with pytest.raises(ValueError):
            ops.class_locations(good, out_ch, k)
    for y in (good, on(torch.zeros((4, 5, 6)))):
        with pytest.raises(Reached):
            ops.class_locations(y, 3, 8)
    # the rule goes through ops._core._check, where tests swap it
    seen = []
    monkeypatch.setattr(ops._core, '_check', lambda t, name='tensor': seen.append(name))
    with pytest.raises(Reached):
        ops.class_locations(torch.zeros((4, 5, 6)), 3, 8)
    assert seen == ['class_locations: y']


# ---- the command line ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 3}, 'norm': {'mean': np.zeros(3), 'std': np.ones(3)}}, allow_pickle=True)
    return path


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + list(more)


def test_flags_parse_with_their_defaults_and_bad_values_are_refused(prepro):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    assert T.FOREGROUND_KEYS == ('foreground_prob', 'foreground_samples', 'foreground_classes')
    a = T.parse_args(_argv(prepro))
    assert (a.foreground_prob, a.foreground_samples, a.foreground_classes) == (0.0, 10000, None)
    assert T.foreground_config(a) is None                                    # off by default
    assert not any(k in vars(T.arg_parser().parse_args(_argv(prepro))) for k in T.FOREGROUND_KEYS)      # a group of its own
    b = T.parse_args(_argv(prepro, '--foreground_prob', '0.33', '--foreground_samples', '500', '--foreground_classes', '2,0'))
    cfg = T.foreground_config(b)
    assert (cfg.prob, cfg.samples, cfg.classes) == (0.33, 500, (0, 2)) and b.foreground_classes == [2, 0]
    assert T.foreground_config(T.parse_args(_argv(prepro, '--foreground_prob', '1'))).classes is None
    for bad in (['--foreground_prob', '1.5'], ['--foreground_prob', '-0.2'], ['--foreground_prob', '0.5', '--foreground_samples', '0'],
                ['--foreground_prob', '0.5', '--foreground_classes', '3'], ['--foreground_prob', '0.5', '--foreground_classes', '0,0'],
                ['--foreground_classes', 'a,b'], ['--foreground_prob', '0.5', '--foreground_classes', '1', '--out_ch', '1']):
        with pytest.raises(ValueError):
            T.parse_args(_argv(prepro, *bad))
    assert T.foreground_config(T.parse_args(_argv(prepro, '--foreground_prob', '0.5', '--foreground_classes', '3', '--out_ch', '4')))


def test_flags_round_trip_through_train_args_and_an_old_pickle_is_off(prepro, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    out = os.path.join(str(tmp_path), 'run')
    a = T.parse_args(_argv(prepro, '--save_folder', out, '--foreground_prob', '0.4', '--foreground_samples', '77', '--foreground_classes',
                           '1,2', '--base_filters', '16', '--groups', '4'))
    stored = T.load_train_args(out)
    assert {k: stored[k] for k in T.FOREGROUND_KEYS} == {'foreground_prob': 0.4, 'foreground_samples': 77, 'foreground_classes': [1, 2]}
    b = T.parse_args(_argv(prepro, '--load_folder', out, '--foreground_prob', '0.9', '--foreground_classes', '0'))      # the folder decides
    assert {k: getattr(b, k) for k in T.FOREGROUND_KEYS} == {k: getattr(a, k) for k in T.FOREGROUND_KEYS}
    cfg = T.foreground_config(b)
    assert (cfg.prob, cfg.samples, cfg.classes) == (0.4, 77, (1, 2))
    # a pickle from before the flags existed
    old = os.path.join(str(tmp_path), 'old')
    os.makedirs(old)
    with open(os.path.join(old, T.ARGS_NAME), 'wb') as f:
        pickle.dump({'model_args': a.model_args, 'crop_size': [16, 16, 16]}, f)
    c = T.parse_args(_argv(prepro, '--load_folder', old, '--foreground_prob', '0.9'))
    assert c.foreground_prob == 0.0 and T.foreground_config(c) is None and c.crop_size == [16, 16, 16]


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
    for flags, want in ((['--foreground_prob', '0.5', '--foreground_samples', '123'], True), ([], False)):
        del calls[:]
        with pytest.raises(Stop):
            T.run(T.parse_args(_argv(prepro, '--resident_gb', '0', *flags)))
        (tr, ktr), (va, kva) = calls
        assert (tr, va) == ('tr', 'va') and 'foreground' not in kva
        assert ('foreground' in ktr) == want
        if want:
            assert isinstance(ktr['foreground'], data.ForegroundConfig)
            assert (ktr['foreground'].prob, ktr['foreground'].samples, ktr['foreground'].classes) == (0.5, 123, None)
