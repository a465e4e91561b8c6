"""CPU: the numpy restatement tests/prepro_ref.py against results recorded from the reference's own create_dataset / compute_norm
(tests/golden/prepro_vectors.npz, written by tests/golden/make_prepro_golden.py), and the host side of bts_amd.preprocess: prepro.npy,
file lookup, the command line, and the argument guards of csrc/prepro.hip, which answer before any HIP call."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import prepro_ref  # noqa: E402

GOLDEN = np.load(os.path.join(HERE, 'golden', 'prepro_vectors.npz'))
SPEC = json.loads(str(GOLDEN['spec']))
SETS = [s['set'] for s in SPEC]


def spec_of(name):
    return [s for s in SPEC if s['set'] == name][0]


def cases_of(name):
    """the raw volumes as get_npy_image gives them: float32, in the order the reference visited the cases"""
    return [(x.astype(np.float32), y.astype(np.float32)) for x, y in zip(GOLDEN[name + '_raw_x'], GOLDEN[name + '_raw_y'])]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_fixture_holds_the_cases_the_kernels_can_break_on():
    assert SETS == ['A', 'B', 'C', 'D']
    assert GOLDEN['A_raw_x'].shape == (5, 19, 13, 11, 2) and GOLDEN['A_raw_x'].dtype == np.int16
    assert GOLDEN['B_raw_x'].shape == (3, 12, 10, 9, 1)
    assert GOLDEN['C_raw_x'].shape == (11, 8, 8, 8, 4) and int(GOLDEN['C_n_val']) == 1
    assert GOLDEN['D_raw_x'].shape == (2, 10, 9, 7, 3) and GOLDEN['D_raw_x'].dtype == np.float32
    a = GOLDEN['A_raw_x']
    assert 0 <= a.min() and a.max() <= 900
    assert set(np.unique(GOLDEN['A_raw_y']).tolist()) == {0, 1, 2, 4}
    assert int(GOLDEN['A_lo'][0]) == 0 and int(GOLDEN['A_hi'][0]) == 18            # a region from the first to the last index of axis 0
    plane = a[:, :, int(GOLDEN['A_hi'][1])]
    assert np.count_nonzero(plane) == 1                                            # one voxel of one channel sets that bound
    for s in ('B', 'D'):
        assert (int(GOLDEN[s + '_lo'][2]) * GOLDEN[s + '_raw_x'].shape[-1]) % 2 == 1   # window origin with odd lo2 * C
    assert (int(GOLDEN['A_lo'][2]) * 2) % 4 != 0                                   # C = 2: even, but no multiple of 16 bytes
    d = GOLDEN['D_raw_x']
    assert np.any(np.signbit(d) & (d == 0)) and np.any(d < 0) and not np.isnan(d).any()
    assert np.any(d != np.round(d))
    last = d[:, int(GOLDEN['D_hi'][0])]
    assert np.count_nonzero(last) == 1 and last[last != 0][0] < 0                  # a plane occupied by one negative value only


@pytest.mark.parametrize('name', SETS)
def test_restatement_reproduces_the_reference(name):
    sp = spec_of(name)
    r = prepro_ref.run(cases_of(name), create_val=sp['create_val'], mode='float32-sum')
    assert list(r['lo']) == GOLDEN[name + '_lo'].tolist() and list(r['hi']) == GOLDEN[name + '_hi'].tolist()
    assert [r['size'][k] for k in 'hwdc'] == GOLDEN[name + '_size'].tolist()
    assert len(r['val']) == int(GOLDEN[name + '_n_val']) and r['val'] == list(range(len(r['val'])))
    assert same_bits(r['mean'], GOLDEN[name + '_mean'])
    assert same_bits(r['std'], GOLDEN[name + '_std'])
    assert same_bits(np.stack(r['x']), GOLDEN[name + '_x'])
    assert same_bits(np.stack(r['y']), GOLDEN[name + '_y'])
    assert set(np.unique(np.stack(r['y'])).tolist()) <= {0.0, 1.0, 2.0, 3.0}


@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_float64_mode_equals_float32_sum_mode_on_integer_volumes(name):
    sp = spec_of(name)
    a = prepro_ref.run(cases_of(name), create_val=sp['create_val'], mode='float64')
    b = prepro_ref.run(cases_of(name), create_val=sp['create_val'], mode='float32-sum')
    for k in ('mean', 'std', 'count', 'sum_x', 'sum_sq'):
        assert same_bits(a[k], b[k]), k
    assert same_bits(np.stack(a['x']), np.stack(b['x']))


def test_float64_mode_is_close_on_float_volumes():
    a = prepro_ref.run(cases_of('D'), mode='float64')
    b = prepro_ref.run(cases_of('D'), mode='float32-sum')
    # a float32 running sum of n terms is within n * 2^-24 * sum|x| of the exact one (the plain summation bound), per volume
    n = float(np.prod(GOLDEN['D_size'][:3]))
    sum_abs = sum(np.abs(prepro_ref.crop(x, a['lo'], a['hi']).astype(np.float64)).sum(axis=(0, 1, 2)) for x, _ in cases_of('D'))
    assert np.all(np.abs(a['sum_x'] - b['sum_x']) <= n * 2.0 ** -24 * sum_abs)
    assert np.any(a['sum_x'] != b['sum_x'])                    # and the two do differ here: the deviation DESIGN section 16 documents
    assert np.array_equal(a['count'], b['count'])


def test_load_prepro_round_trips_the_reference_structure(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    mean = GOLDEN['A_mean'].reshape(1, 1, 1, 2)
    std = GOLDEN['A_std'].reshape(1, 1, 1, 2)
    size = {'h': 18, 'w': 9, 'd': 8, 'c': 2}
    path = str(tmp_path / 'prepro.npy')
    np.save(path, {'size': size, 'norm': {'mean': mean, 'std': std}})
    got_size, got_mean, got_std = preprocess.load_prepro(path)
    assert got_size == (18, 9, 8, 2) and all(isinstance(v, int) for v in got_size)
    assert got_mean.shape == (2,) and same_bits(got_mean, GOLDEN['A_mean']) and same_bits(got_std, GOLDEN['A_std'])
    np.save(path, {'size': dict(size, c=3), 'norm': {'mean': mean, 'std': std}})
    with pytest.raises(ValueError):
        preprocess.load_prepro(path)


def test_get_npy_image_takes_the_first_match_in_sorted_order(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import nifti, preprocess
    vol = GOLDEN['A_raw_x'][0, ..., 0]
    nifti.save(str(tmp_path / 'b_case_t1ce.nii.gz'), vol + 1, np.eye(4))
    nifti.save(str(tmp_path / 'a_case_t1ce.nii'), vol, np.eye(4))
    got = preprocess.get_npy_image(str(tmp_path), 't1ce')
    assert got.dtype == np.float32 and np.array_equal(got, vol.astype(np.float32))
    with pytest.raises(ValueError, match='flair'):
        preprocess.get_npy_image(str(tmp_path), 'flair')


def test_remap_labels_and_make_dirs(tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    y = np.array([0, 1, 2, 3, 4, 5], np.float32)
    assert preprocess.remap_labels(y).tolist() == [0, 1, 2, 3, 3, 3] and y[4] == 4
    out = tmp_path / 'data'
    out.mkdir()
    (out / 'stale').write_text('x')
    train_loc, val_loc = preprocess.make_dirs(str(out))
    assert sorted(os.listdir(str(out))) == ['train', 'val'] and os.path.isdir(train_loc) and os.path.isdir(val_loc)


def test_command_line_takes_the_reference_flags():
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    a = preprocess.parse_args(['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--truth', 'seg'])
    assert a.in_locs == ['a', 'b'] and a.modalities == ['t1ce', 'flair'] and a.truth == 'seg'
    assert a.create_val is False and a.out_loc == './data'
    a = preprocess.parse_args(['--in_locs', 'a', '--modalities', 't1', '--truth', 'seg', '--create_val', '--out_loc', '/x'])
    assert a.create_val is True and a.out_loc == '/x' and a.in_locs == ['a']
    with pytest.raises(SystemExit):
        preprocess.parse_args(['--in_locs', 'a', '--modalities', 't1'])


def test_argument_guards_answer_without_a_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    SHAPE, WORKSPACE = -1, -4
    assert L._bts_prepro_occupancy(None, None, 0, 8, 8, 2, None) == SHAPE
    assert L._bts_prepro_occupancy(None, None, 8, 8, 8, 17, None) == SHAPE
    assert L._bts_prepro_occupancy(None, None, 8, 8, 8, 0, None) == SHAPE
    nb = L._bts_prepro_workspace(4)
    assert nb > 0 and L._bts_prepro_workspace(16) == 4 * nb and L._bts_prepro_workspace(17) < 0 and L._bts_prepro_workspace(0) < 0
    ok = (8 * 8 * 4, 8 * 4, 8, 8, 8, 4)                                   # st0, st1, T0, T1, T2, C of a dense window
    assert L._bts_prepro_sums(None, 256, 32, 8, 8, 8, 17, None, None, None, 1 << 30, None) == SHAPE
    assert L._bts_prepro_sums(None, 256, 32, 0, 8, 8, 4, None, None, None, 1 << 30, None) == SHAPE
    assert L._bts_prepro_sums(None, 256, 31, 8, 8, 8, 4, None, None, None, 1 << 30, None) == SHAPE    # st1 < T2 * C
    assert L._bts_prepro_sums(None, 255, 32, 8, 8, 8, 4, None, None, None, 1 << 30, None) == SHAPE    # st0 < T1 * st1
    assert L._bts_prepro_sums(None, *ok, None, None, None, 1 << 30, None) == WORKSPACE                # no workspace pointer
    import ctypes
    buf = ctypes.create_string_buffer(64)
    assert L._bts_prepro_sums(None, *ok, None, None, ctypes.cast(buf, ctypes.c_void_p), nb - 1, None) == WORKSPACE
    assert L._bts_prepro_crop_norm(None, None, 256, 32, 0, 0, 8, 8, 8, 17, None, None, None, None, None) == SHAPE
    assert L._bts_prepro_crop_norm(None, None, 256, 32, 0, 0, 8, 8, -1, 4, None, None, None, None, None) == SHAPE
    assert L._bts_prepro_crop_norm(None, None, 256, 31, 0, 0, 8, 8, 8, 4, None, None, None, None, None) == SHAPE
    assert L._bts_prepro_crop_norm(None, ctypes.cast(buf, ctypes.c_void_p), 256, 32, 64, 7, 8, 8, 8, 4, None, None, None, None,
                                   None) == SHAPE                                                  # label stride < T2
    # a launch holds fewer than 2^32 threads: 2^24 workgroups of 256 are refused here, not by the launch
    assert L._bts_prepro_occupancy(None, None, 1 << 14, 1 << 13, 1, 1, None) == SHAPE                # 2^27 rows, 8 per workgroup
    assert L._bts_prepro_crop_norm(None, None, 1 << 13, 1, 0, 0, 1 << 14, 1 << 13, 1, 1, None, None, None, None, None) == SHAPE


def test_preprocess_refuses_an_out_loc_that_holds_its_input(tmp_path):
    """out_loc is removed as a whole before anything is read, so an input folder inside it must stop the call first"""
    import bts_amd  # noqa: F401
    from bts_amd import preprocess
    out = tmp_path / 'data'
    scans = out / 'scans'
    scans.mkdir(parents=True)
    (scans / 'keep').write_text('x')
    for in_loc in (str(scans), str(out), os.path.join(str(out), 'train', '..', 'scans')):
        with pytest.raises(ValueError, match='out_loc'):
            preprocess.preprocess([str(tmp_path / 'elsewhere'), in_loc], ['t1'], 'seg', str(out))
        assert (scans / 'keep').read_text() == 'x'
