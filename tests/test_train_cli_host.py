"""No GPU: the argument handling of `python -m bts_amd.train` against the reference's own TrainArgParser, recorded in
tests/golden/train_cli_flags.json (tests/golden/make_train_cli_flags.py), and the argument validation of bts_augment_batch."""
import ctypes
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_cli_flags.json')


def _parser():
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    return T, T.arg_parser()


def _actions(parser):
    return {a.option_strings[0]: a for a in parser._actions if a.option_strings and a.dest != 'help'}


def test_every_reference_flag_is_there_as_recorded():
    _, parser = _parser()
    ours = _actions(parser)
    flags = json.load(open(GOLDEN))['flags']
    assert len(flags) == 21 and flags[0]['flag'] == '--train_loc' and flags[-1]['flag'] == '--out_ch'
    for f in flags:
        a = ours[f['flag']]
        assert a.dest == f['dest'], f['flag']
        assert a.default == f['default'] and type(a.default) is type(f['default']), f['flag']
        assert (a.type.__name__ if a.type is not None else None) == f['type'], f['flag']
        assert (list(a.choices) if a.choices is not None else None) == f['choices'], f['flag']
        assert bool(a.required) == f['required'], f['flag']
        assert (a.nargs == 0 and a.const is True) == f['store_true'], f['flag']


def test_added_flags_and_their_defaults():
    _, parser = _parser()
    ours = _actions(parser)
    recorded = {f['flag'] for f in json.load(open(GOLDEN))['flags']}
    assert set(ours) - recorded == {'--dtype', '--workers', '--resident_gb', '--seed'}
    assert ours['--dtype'].default == 'float32' and sorted(ours['--dtype'].choices) == ['bfloat16', 'float16', 'float32']
    assert ours['--workers'].default == 8 and ours['--workers'].type is int
    assert ours['--resident_gb'].default is None and ours['--resident_gb'].type is float       # None: a quarter of the device's memory
    assert ours['--seed'].default == 0 and ours['--seed'].type is int


@pytest.mark.parametrize('argv', [['--prepro_loc', 'p.npy'], ['--train_loc', 't']])
def test_required_locations(argv):
    T, _ = _parser()
    with pytest.raises(SystemExit):
        T.parse_args(argv)


@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 3}, 'norm': {'mean': np.zeros(3), 'std': np.ones(3)}}, allow_pickle=True)
    return path


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + list(more)


def test_parse_folds_model_args_and_reads_the_dump(prepro):
    T, _ = _parser()
    args = T.parse_args(_argv(prepro, '--crop_size', '16,8,12', '--gpu', '--base_filters', '16', '--groups', '4', '--dtype', 'bfloat16'))
    assert args.crop_size == [16, 8, 12] and args.prepro_size == [20, 18, 22, 3]
    assert args.model_args == dict(data_format='channels_first', base_filters=16, depth=4, l2_scale=1e-5, dropout=0.2, groups=4,
                                   reduction=8, downsampling='conv', upsampling='conv', out_ch=3, in_ch=3)
    assert args.data_format == 'channels_first' and args.dtype == 'bfloat16' and args.save_folder == ''
    assert not any(k.startswith('model_args.') for k in vars(args))


def test_the_two_size_checks_of_the_reference(prepro):
    T, _ = _parser()
    with pytest.raises(AssertionError, match='Base filters must be a multiple of 16 for group normalization at lowest spatial level.'):
        T.parse_args(_argv(prepro, '--base_filters', '8'))
    with pytest.raises(AssertionError, match='Base filters must be a multiple of 6 for squeeze-excitation reduction.'):
        T.parse_args(_argv(prepro, '--reduction', '6'))


def test_refusals_by_name(prepro):
    T, _ = _parser()
    with pytest.raises(ValueError, match='avg'):
        T.parse_args(_argv(prepro, '--downsampling', 'avg'))
    with pytest.raises(ValueError, match='--val_loc'):
        T.parse_args(['--train_loc', 'tr', '--prepro_loc', prepro])


def test_save_folder_gets_train_args_and_load_folder_overrides(prepro, tmp_path):
    T, _ = _parser()
    out = os.path.join(str(tmp_path), 'run')
    args = T.parse_args(_argv(prepro, '--save_folder', out, '--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4',
                              '--reduction', '4', '--depth', '3', '--data_format', 'channels_last'))
    stored = T.load_train_args(out)
    assert type(stored) is dict and stored['model_args'] == args.model_args and stored['model_args']['in_ch'] == 3
    assert stored['crop_size'] == [16, 16, 16]
    # a folder written by save_train_args alone, conflicting flags on the command line
    other = os.path.join(str(tmp_path), 'other')
    margs = dict(args.model_args, base_filters=32, depth=2)
    T.save_train_args(other, {'model_args': margs, 'crop_size': [32, 16, 8]})
    again = T.parse_args(_argv(prepro, '--load_folder', other, '--base_filters', '16', '--crop_size', '64,64,64', '--data_format', 'channels_first'))
    assert again.model_args == margs and again.crop_size == [32, 16, 8] and again.save_folder == other
    assert again.data_format == 'channels_last'
    assert T.load_train_args(other)['model_args'] == margs


# ---- bts_augment_batch: everything invalid is refused before any HIP call ----
def test_augment_batch_argument_validation_without_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    assert L._bts_augment_batch_max() >= 1
    n = 2
    ptrs = (ctypes.c_void_p * n)(64, 64)                    # (never dereferenced on the host, never reached by a refused call)
    offs = (ctypes.c_int * (3 * n))(0, 0, 0, 1, 2, 3)
    flips = (ctypes.c_int * n)(0, 7)
    sh = (ctypes.c_float * (n * 16))()
    sc = (ctypes.c_float * (n * 16))()
    P = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731

    def call(N=n, S=(9, 10, 11), C=2, T=(8, 8, 8), out_ch=3, layout=0, x=ptrs, y=ptrs, var=ptrs, offsets=offs, flip=flips, shift=sh, scale=sc):
        return L._bts_augment_batch(P(x) if x is not None else None, P(y) if y is not None else None, P(var) if var is not None else None,
                                    None, None, N, S[0], S[1], S[2], C, T[0], T[1], T[2], P(offsets) if offsets is not None else None,
                                    P(flip) if flip is not None else None, P(shift) if shift is not None else None,
                                    P(scale) if scale is not None else None, out_ch, layout, None)
    SHAPE = -1
    assert call(N=0) == SHAPE and call(N=-3) == SHAPE
    assert call(C=0) == SHAPE and call(C=17) == SHAPE
    assert call(out_ch=0) == SHAPE
    assert call(layout=2) == SHAPE and call(layout=-1) == SHAPE
    for name in ('x', 'y', 'var', 'offsets', 'flip', 'shift', 'scale'):
        assert call(**{name: None}) == SHAPE, name
    assert call(flip=(ctypes.c_int * n)(0, 8)) == SHAPE
    assert call(offsets=(ctypes.c_int * (3 * n))(0, 0, 0, 2, 2, 3)) == SHAPE          # 2 + 8 > 9 on axis 0 of the second example
    assert call(offsets=(ctypes.c_int * (3 * n))(0, 0, 4, 0, 0, 0)) == SHAPE          # 4 + 8 > 11 on axis 2 of the first
    assert call(offsets=(ctypes.c_int * (3 * n))(0, -1, 0, 0, 0, 0)) == SHAPE
    assert call(T=(8, 8, 12)) == SHAPE                                                # crop larger than the volume
    # the one-example entry point is the same check
    assert L._bts_augment_crop(None, None, None, None, None, 9, 10, 11, 2, 8, 8, 8, 2, 0, 0, 0, P(sh), P(sc), 3, None) == SHAPE
    assert L._bts_augment_crop(None, None, None, None, None, 9, 10, 11, 2, 8, 8, 8, 0, 0, 0, 8, P(sh), P(sc), 3, None) == SHAPE
