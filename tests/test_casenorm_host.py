"""Per-case normalisation, the host side (no GPU): the numpy restatement of the contract (tests/casenorm_ref.py) against np.percentile and
under scaling by a power of two, the argument guards of csrc/casenorm.hip, which answer before any HIP call, the command line of
bts_amd.preprocess and the prepro.npy round trips."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import casenorm_ref as CR  # noqa: E402

CLIPS = (None, (0.5, 99.5), (0.0, 100.0), (25.0, 75.0))
SHAPES = ((5, 7, 9, 1), (6, 10, 33, 2), (9, 17, 21, 4), (3, 5, 7, 3))


def gamma_volume(shape, seed):
    """integer-valued gamma-distributed intensities with 40 % background"""
    rng = np.random.default_rng(seed)
    x = np.floor(rng.gamma(2.0, 150.0, size=shape)).astype(np.float32) + 1.0
    x[rng.random(shape[:3]) < 0.4] = 0.0
    return x


@pytest.mark.parametrize('shape', SHAPES)
def test_bounds_agree_with_numpy_percentile(shape):
    """both are a handful of rounded float64 operations on the same two order statistics: within 4 ulp of the larger of them"""
    x = gamma_volume(shape, 11 + shape[0])
    inside = CR.inside_mask(x)
    for ch in range(shape[3]):
        vals = np.sort(x[..., ch][inside].astype(np.float64))
        for p in (0.0, 0.5, 1.0, 25.0, 33.3, 50.0, 75.0, 99.5, 100.0):
            got = CR.percentile_bound(vals, p)
            want = np.percentile(vals, p, method='linear')
            h = (vals.size - 1) * p / 100.0
            a, b = vals[int(np.floor(h))], vals[min(int(np.floor(h)) + 1, vals.size - 1)]
            assert abs(got - want) <= 4 * 2.0 ** -52 * max(abs(a), abs(b)), (shape, ch, p, got, want)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('clip', CLIPS)
def test_scaling_by_four_scales_the_statistics_and_leaves_the_output(shape, clip):
    """a power of two commutes with every rounding involved: bit-identical outputs, statistics scaled by exactly 4"""
    x = gamma_volume(shape, 3 + shape[1])
    out1, st1, _ = CR.case_norm(x, None, clip)
    out4, st4, _ = CR.case_norm(4.0 * x, None, clip)
    assert out1.tobytes() == out4.tobytes()
    assert st1[0] == st4[0] and st1[0] > 0
    assert np.array_equal(st4[1:], 4.0 * st1[1:])
    assert np.isfinite(out1).all() and out1[~CR.inside_mask(x)].tobytes() == bytes(out1[~CR.inside_mask(x)].nbytes)


def test_reference_edges():
    x = np.zeros((2, 3, 4, 2), dtype=np.float32)
    out, st, _ = CR.case_norm(x)
    assert st.tolist() == [0.0] * 9 and not out.any()
    x[0, 0, 0] = (3.0, 5.0)
    x[1, 1, 1] = (3.0, 9.0)
    out, st, _ = CR.case_norm(x)                     # channel 0 constant over the two voxels inside
    assert st[0] == 2 and st[2] == 0 and not out[..., 0].any()
    assert out[0, 0, 0, 1] == -1.0 and out[1, 1, 1, 1] == 1.0
    out, st, _ = CR.case_norm(x, None, (50.0, 50.0))
    assert not out.any() and st[1 + 4 + 2] == st[1 + 4 + 3] == 7.0


# ---- the C ABI's guards ------------------------------------------------------------------------------------------------------------
def test_argument_guards_answer_without_a_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    for c in range(1, 17):
        assert L._bts_case_norm_workspace(c) > 0
    for c in (0, -1, 17, 1 << 20):
        assert L._bts_case_norm_workspace(c) < 0
    assert L._bts_case_norm_blocks() >= 64
    SHAPE, WORK = -1, -4
    p = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused before any HIP call
    null = ctypes.c_void_p(None)

    def call(C=2, T=(4, 5, 6), st=None, mask=null, mst=(0, 0), y=null, yst=(0, 0), yo=null, clip=1, p_lo=0.5, p_hi=99.5, ws=p, wsb=None,
             x=p, xo=p, stats=p):
        t0, t1, t2 = T
        st = st if st is not None else (t1 * t2 * C, t2 * C)
        wsb = wsb if wsb is not None else max(L._bts_case_norm_workspace(C), 0)
        return L._bts_case_norm(x, st[0], st[1], mask, mst[0], mst[1], y, yst[0], yst[1], t0, t1, t2, C, clip, p_lo, p_hi, xo, yo, stats,
                                ws, wsb, null)

    for C in (0, -3, 17):
        assert call(C=C) == SHAPE
    for T in ((0, 5, 6), (4, 0, 6), (4, 5, 0), (-1, 5, 6), (4, 5, -6)):
        assert call(T=T) == SHAPE
    assert call(st=(5 * 6 * 2, 6 * 2 - 1)) == SHAPE and call(st=(5 * 6 * 2 - 1, 6 * 2)) == SHAPE
    assert call(mask=p, mst=(30, 5)) == SHAPE and call(mask=p, mst=(29, 6)) == SHAPE
    assert call(y=p, yo=p, yst=(30, 5)) == SHAPE and call(y=p, yo=p, yst=(29, 6)) == SHAPE
    assert call(y=p, yst=(30, 6)) == SHAPE                                            # a label window without an output
    for T in ((1 << 11, 1 << 10, 1 << 10), (65536, 65536, 1), (46341, 46341, 1)):      # 2^31 voxels and more
        assert call(C=1, T=T) == SHAPE
    for lo, hi in ((-0.1, 50.0), (0.0, 100.5), (60.0, 40.0), (float('nan'), 50.0), (10.0, float('nan'))):
        assert call(p_lo=lo, p_hi=hi) == SHAPE
    assert call(ws=null) == WORK
    for C in (1, 2, 4, 16):
        assert call(C=C, wsb=L._bts_case_norm_workspace(C) - 1) == WORK


def test_ops_refuses_what_is_no_spatial_slice_and_bad_percentiles():
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    for clip in ((-1.0, 50.0), (60.0, 40.0), (0.0, 101.0), (1.0,), 'ab'):
        with pytest.raises(ValueError):
            ops.check_clip(clip)
    assert ops.check_clip(None) is None and ops.check_clip((0, 100)) == (0.0, 100.0)
    with pytest.raises(ValueError, match='GPU'):
        ops.case_norm(torch.zeros(2, 3, 4, 2))


# ---- the command line --------------------------------------------------------------------------------------------------------------
BASE = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--truth', 'seg']


def test_command_line():
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    a = preprocess.parse_args(BASE)                                   # the lines tests/test_prepro_host.py pins parse as before
    assert a.in_locs == ['a', 'b'] and a.modalities == ['t1ce', 'flair'] and a.truth == 'seg'
    assert a.create_val is False and a.out_loc == './data'
    assert sorted(vars(a)) == ['create_val', 'in_locs', 'modalities', 'out_loc', 'truth']
    assert preprocess.norm_kwargs(a) == {'norm': 'dataset', 'clip': None}
    a = preprocess.parse_args(['--in_locs', 'a', '--modalities', 't1', '--truth', 'seg', '--create_val', '--out_loc', '/x'])
    assert a.create_val is True and a.out_loc == '/x' and a.in_locs == ['a']
    a = preprocess.parse_args(BASE + ['--norm', 'case'])
    assert preprocess.norm_kwargs(a) == {'norm': 'case', 'clip': None}
    a = preprocess.parse_args(BASE + ['--norm', 'case', '--clip_percentiles', '0.5,99.5'])
    assert preprocess.norm_kwargs(a) == {'norm': 'case', 'clip': (0.5, 99.5)}
    assert preprocess.norm_kwargs(preprocess.parse_args(BASE + ['--norm', 'dataset'])) == {'norm': 'dataset', 'clip': None}
    for bad in (['--clip_percentiles', '0.5,99.5'], ['--norm', 'dataset', '--clip_percentiles', '0.5,99.5'],
                ['--norm', 'case', '--clip_percentiles', '60,40'], ['--norm', 'case', '--clip_percentiles', '-1,50'],
                ['--norm', 'case', '--clip_percentiles', '0,100.5'], ['--norm', 'case', '--clip_percentiles', '5'],
                ['--norm', 'case', '--clip_percentiles', 'a,b'], ['--norm', 'scan']):
        with pytest.raises(SystemExit):
            preprocess.parse_args(BASE + bad)


def test_preprocess_refuses_a_clip_without_case_mode(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    out = tmp_path / 'out'
    with pytest.raises(ValueError, match='case'):
        preprocess.preprocess([str(tmp_path)], ['t1'], 'seg', str(out), clip=(1.0, 99.0))
    with pytest.raises(ValueError, match='norm'):
        preprocess.preprocess([str(tmp_path)], ['t1'], 'seg', str(out), norm='scan')
    assert not out.exists()


# ---- prepro.npy ----------------------------------------------------------------------------------------------------------------------
SIZE = {'h': 12, 'w': 14, 'd': 10, 'c': 2}


def test_prepro_files_round_trip(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    mean, std = np.array([100.0, 120.0]).reshape(1, 1, 1, 2), np.array([40.0, 50.0]).reshape(1, 1, 1, 2)
    old = str(tmp_path / 'old.npy')
    np.save(old, {'size': SIZE, 'norm': {'mean': mean, 'std': std}})                 # a file without 'mode' is dataset
    spec = preprocess.load_norm(old)
    assert isinstance(spec, preprocess.NormSpec) and spec.mode == 'dataset' and spec.clip is None
    assert spec.mean.tolist() == [100.0, 120.0] and spec.std.tolist() == [40.0, 50.0]
    for clip in (None, (0.5, 99.5)):
        path = str(tmp_path / 'case.npy')
        np.save(path, {'size': SIZE, 'norm': {'mode': 'case', 'clip': clip, 'mean': np.zeros((1, 1, 1, 2)), 'std': np.ones((1, 1, 1, 2))}})
        spec = preprocess.load_norm(path)
        assert spec.mode == 'case' and spec.clip == clip
        size, m, s = preprocess.load_prepro(path)                                    # an identity through the old reader
        assert size == (12, 14, 10, 2) and m.tolist() == [0.0, 0.0] and s.tolist() == [1.0, 1.0]
    bad = str(tmp_path / 'bad.npy')
    np.save(bad, {'size': SIZE, 'norm': {'mode': 'scan', 'mean': mean, 'std': std}})
    with pytest.raises(ValueError, match='mode'):
        preprocess.load_norm(bad)
    np.save(bad, {'size': SIZE, 'norm': {'mode': 'case', 'clip': (60.0, 40.0), 'mean': mean, 'std': std}})
    with pytest.raises(ValueError):
        preprocess.load_norm(bad)


def test_dataset_mode_writes_exactly_the_keys_it_always_has(tmp_path, monkeypatch):
    """preprocess() in dataset mode, the device work stubbed out: the dictionary saved holds 'size' and 'norm' = {'mean', 'std'}"""
    import bts_amd  # noqa: F401
    from bts_amd import preprocess

    class View(object):
        device = 'cpu'
    mean, std = np.array([1.0, 2.0]).reshape(1, 1, 1, 2), np.array([3.0, 4.0]).reshape(1, 1, 1, 2)
    monkeypatch.setattr(preprocess, 'create_dataset', lambda *a, **k: ([View()], [View()], dict(SIZE)))
    monkeypatch.setattr(preprocess, 'compute_norm', lambda x, c: (mean, std))
    monkeypatch.setattr(preprocess, '_stats_on', lambda dev, v: v)
    monkeypatch.setattr(preprocess, '_write', lambda *a, **k: None)
    out = str(tmp_path / 'out')
    r = preprocess.preprocess([str(tmp_path / 'in')], ['t1ce', 'flair'], 'seg', out)
    d = np.load(os.path.join(out, 'prepro.npy'), allow_pickle=True).item()
    assert sorted(d) == ['norm', 'size'] and sorted(d['norm']) == ['mean', 'std'] and d['size'] == SIZE
    assert np.array_equal(d['norm']['mean'], mean) and np.array_equal(d['norm']['std'], std)
    assert sorted(r) == ['mean', 'n_train', 'n_val', 'size', 'std']
    monkeypatch.setattr(preprocess, 'compute_norm', lambda x, c: pytest.fail('compute_norm runs in case mode'))
    preprocess.preprocess([str(tmp_path / 'in')], ['t1ce', 'flair'], 'seg', out, norm='case', clip=(0.5, 99.5))
    d = np.load(os.path.join(out, 'prepro.npy'), allow_pickle=True).item()
    assert sorted(d['norm']) == ['clip', 'mean', 'mode', 'std'] and d['norm']['mode'] == 'case' and d['norm']['clip'] == (0.5, 99.5)
    assert preprocess.load_norm(os.path.join(out, 'prepro.npy')).clip == (0.5, 99.5)
