"""No GPU: the nested BraTS regions WT, TC, ET -- the definition (tests/regions_ref.py), the argument validation of the three entry points of
csrc/regions.hip through the C ABI, and --targets on the train command's line, in train_args.pkl and in prepare_dataset."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import regions_ref as RR  # noqa: E402

UNSUPPORTED, SHAPE = -3, -1


# ---- the definition ----
def test_round_trip_of_a_label_map():
    rng = np.random.default_rng(11)
    lab = np.array([0, 1, 2, 4])[rng.integers(0, 4, size=(7, 5, 9))]
    assert set(np.unique(lab).tolist()) == {0, 1, 2, 4}
    reg = RR.encode(RR.onehot(lab))
    assert reg.shape == lab.shape + (3,) and set(np.unique(reg).tolist()) == {0.0, 1.0}
    # nested: ET inside TC inside WT
    assert np.all(reg[..., 2] <= reg[..., 1]) and np.all(reg[..., 1] <= reg[..., 0])
    for strict in (False, True):
        assert np.array_equal(RR.decode(reg, None, 0.5, strict), lab)
    # the regions are what the scores call WT, TC, ET
    assert np.array_equal(reg[..., 0] > 0, lab > 0) and np.array_equal(reg[..., 1] > 0, (lab == 1) | (lab == 4))
    assert np.array_equal(reg[..., 2] > 0, lab == 4)


def test_overwrite_and_nested_rule_differ():
    p = np.array([[0.2, 0.3, 0.9], [0.9, 0.2, 0.8], [0.9, 0.8, 0.7], [0.6, 0.1, 0.2], [0.1, 0.7, 0.2]])
    assert RR.decode(p).tolist() == [4, 4, 4, 2, 1]
    assert RR.decode_nested(p).tolist() == [0, 2, 4, 2, 0]
    # the mask, and the two comparisons at the threshold itself
    assert RR.decode(p, np.array([1, 0, 1, 0, 1.0])).tolist() == [4, 0, 4, 0, 1]
    at = np.array([[0.5, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.5]])
    assert RR.decode(at, None, 0.5, strict=False).tolist() == [2, 1, 4] and RR.decode(at, None, 0.5, strict=True).tolist() == [0, 0, 0]


def test_dice_counts_and_value():
    t = RR.encode(RR.onehot(np.array([0, 1, 2, 4, 4, 2])))
    p = np.array([[0.9, 0.1, 0.1], [0.9, 0.9, 0.1], [0.4, 0.1, 0.1], [0.9, 0.9, 0.9], [0.9, 0.5, 0.6], [0.6, 0.6, 0.6]])
    table = RR.dice_counts(t, p)
    assert table.tolist() == [4, 5, 5, 2, 3, 3, 2, 3, 2]
    macro, micro = RR.dice_value(table)
    assert macro == pytest.approx((9 / 11 + 5 / 7 + 5 / 6) / 3, rel=1e-15) and micro == pytest.approx(8 / 21, rel=1e-15)


# ---- the C ABI refuses bad arguments before any HIP call ----
def test_argument_validation_without_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    for c in (2, 4, 1, 0):
        assert L._bts_region_targets(None, 1, 8, c, 0, None) == UNSUPPORTED
        assert L._bts_region_targets(None, 1, 8, c, 1, None) == UNSUPPORTED
        assert L._bts_region_dice_sums(None, None, None, None, 8, c, 3, 3, None) == UNSUPPORTED
        assert L._bts_region_finish(None, None, None, None, 8, c, 0.5, None) == UNSUPPORTED
    for layout in (0, 1):
        assert L._bts_region_targets(None, 0, 8, 3, layout, None) == SHAPE          # N = 0
        assert L._bts_region_targets(None, -1, 8, 3, layout, None) == SHAPE
        assert L._bts_region_targets(None, 1, 0, 3, layout, None) == SHAPE          # V = 0
    assert L._bts_region_dice_sums(None, None, None, None, 0, 3, 3, 3, None) == SHAPE        # NV = 0
    assert L._bts_region_dice_sums(None, None, None, None, 8, 3, 2, 3, None) == SHAPE        # ldt < C
    assert L._bts_region_dice_sums(None, None, None, None, 8, 3, 3, 2, None) == SHAPE        # ldp < C
    assert L._bts_region_finish(None, None, None, None, 0, 3, 0.5, None) == SHAPE            # nvox = 0
    assert L._bts_region_finish(None, None, None, None, -5, 3, 0.5, None) == SHAPE


def test_ops_refuse_other_channel_counts_and_host_tensors():
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import ops
    for fn in (lambda: ops.region_targets(torch.zeros(1, 4, 3)), lambda: ops.region_targets(np.zeros((1, 4, 3), np.float32))):
        with pytest.raises(ValueError, match='dense float32 tensor on the GPU'):
            fn()
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        ops.region_finish(torch.zeros(1, 2, 2, 2, 3), torch.ones(1, 2, 2, 2, 1))
    with pytest.raises(RuntimeError, match='must live on the GPU'):
        ops.region_dice_sums(torch.zeros(1, 2, 2, 2, 3), torch.zeros(1, 2, 2, 2, 3))


# ---- the command line ----
@pytest.fixture()
def prepro(tmp_path):
    path = os.path.join(str(tmp_path), 'prepro.npy')
    np.save(path, {'size': {'h': 20, 'w': 18, 'd': 22, 'c': 2}, 'norm': {'mean': np.zeros(2), 'std': np.ones(2)}}, allow_pickle=True)
    return path


SMALL = ['--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4', '--reduction', '4', '--depth', '3']


def _argv(prepro, *more):
    return ['--train_loc', 'tr', '--val_loc', 'va', '--prepro_loc', prepro] + SMALL + list(more)


def test_the_flag_lives_in_full_parser_only():
    import bts_amd  # noqa: F401
    from bts_amd import data
    from bts_amd import train as T
    assert data.TARGETS == ('labels', 'regions')
    act = {a.option_strings[0]: a for a in T.full_parser()._actions if a.option_strings}
    assert act['--targets'].default == 'labels' and tuple(act['--targets'].choices) == data.TARGETS
    assert '--targets' not in {s for a in T.arg_parser()._actions for s in a.option_strings}
    with pytest.raises(SystemExit):
        T.full_parser().parse_args(['--train_loc', 'a', '--prepro_loc', 'b', '--targets', 'classes'])


def test_train_args_store_and_restore_the_mode(prepro, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    assert T.parse_args(_argv(prepro)).targets == 'labels'
    out = os.path.join(str(tmp_path), 'run')
    args = T.parse_args(_argv(prepro, '--save_folder', out, '--targets', 'regions'))
    assert args.targets == 'regions' and T.load_train_args(out)['targets'] == 'regions'
    plain = os.path.join(str(tmp_path), 'plain')
    assert T.parse_args(_argv(prepro, '--save_folder', plain)).targets == 'labels' and T.load_train_args(plain)['targets'] == 'labels'
    # a resumed run: the folder's mode wins over the flag, both ways, and is written back
    again = T.parse_args(_argv(prepro, '--load_folder', out, '--targets', 'labels'))
    assert again.targets == 'regions' and again.save_folder == out and T.load_train_args(out)['targets'] == 'regions'
    assert T.parse_args(_argv(prepro, '--load_folder', plain, '--targets', 'regions')).targets == 'labels'
    # a pickle from before the flag existed means labels
    old = os.path.join(str(tmp_path), 'old')
    T.save_train_args(old, {'model_args': dict(args.model_args), 'crop_size': [16, 16, 16]})
    assert 'targets' not in T.load_train_args(old)
    assert T.parse_args(_argv(prepro, '--load_folder', old, '--targets', 'regions')).targets == 'labels'


def test_regions_need_three_output_channels(prepro, tmp_path):
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    out = os.path.join(str(tmp_path), 'run')
    with pytest.raises(ValueError, match='--out_ch must be 3'):
        T.parse_args(_argv(prepro, '--targets', 'regions', '--out_ch', '2', '--save_folder', out))
    assert not os.path.exists(os.path.join(out, T.ARGS_NAME))              # refused before anything is written
    assert T.parse_args(_argv(prepro, '--targets', 'labels', '--out_ch', '2')).model_args['out_ch'] == 2


def test_prepare_dataset_checks_the_mode(tmp_path):
    import torch
    import bts_amd  # noqa: F401
    from bts_amd import data
    cpu = torch.device('cpu')
    with pytest.raises(ValueError, match="unknown targets 'x'"):
        data.prepare_dataset(str(tmp_path), 1, (8, 8, 8, 2), (4, 4, 4), 3, device=cpu, rank=0, world=1, targets='x')
    for fmt in ('channels_last', 'channels_first'):
        with pytest.raises(ValueError, match='out_ch must be 3'):
            data.prepare_dataset(str(tmp_path), 1, (8, 8, 8, 2), (4, 4, 4), 2, data_format=fmt, device=cpu, rank=0, world=1, targets='regions')
        ds, n = data.prepare_dataset(str(tmp_path), 1, (8, 8, 8, 2), (4, 4, 4), 3, data_format=fmt, device=cpu, rank=0, world=1, targets='regions')
        assert n == 0 and ds.targets == 'regions'
        assert data.prepare_dataset(str(tmp_path), 1, (8, 8, 8, 2), (4, 4, 4), 2, data_format=fmt, device=cpu, rank=0, world=1)[0].targets == 'labels'


def test_inference_side_checks_the_mode():
    import bts_amd  # noqa: F401
    from bts_amd import infer

    class Decoder(object):
        def __init__(self, out_ch):
            self.out_ch = out_ch

    class FakeModel(object):
        def __init__(self, out_ch):
            self.decoder = Decoder(out_ch)

    assert infer.TARGETS == ('labels', 'regions')
    assert infer.StageSpec(FakeModel(3), None, None, 8).targets == 'labels'
    assert infer.StageSpec(FakeModel(3), None, None, 8, targets='regions').targets == 'regions'
    assert infer.StageSpec(FakeModel(1), None, None, 8, targets='labels').targets == 'labels'
    for make in (lambda: infer.StageSpec(FakeModel(1), None, None, 8, targets='regions'),
                 lambda: infer.TestTimeAugmentor(None, None, FakeModel(2), targets='regions')):
        with pytest.raises(ValueError, match='out_ch = '):
            make()
    with pytest.raises(ValueError, match='unknown targets'):
        infer.StageSpec(FakeModel(3), None, None, 8, targets='nested')
    assert infer.TestTimeAugmentor(None, None, FakeModel(3), targets='regions').targets == 'regions'
