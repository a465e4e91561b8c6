"""CPU: the sliding-window plan (infer.window_plan, infer.WindowSpec) against known answers, its own invariants and the independent
float64 restatement of tests/window_ref.py; the command's --window flags; the argument validation of csrc/window.hip's entry points,
which answers before any HIP call."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import window_ref as WR  # noqa: E402


def product_axis(S, R, overlap=0.5, mode='gaussian', sigma_scale=0.125):
    """one axis of the product's plan (the other two axes are single voxels)"""
    import bts_amd  # noqa: F401
    from bts_amd import infer
    starts, tables = infer.window_plan((S, 1, 1), (R, 1, 1), overlap, mode, sigma_scale)
    assert starts[1] == [0] and starts[2] == [0] and np.array_equal(tables[1], [[1.0]]) and np.array_equal(tables[2], [[1.0]])
    assert tables[0].dtype == np.float64 and tables[0].shape == (len(starts[0]), R)
    return list(starts[0]), tables[0]


def axis_sum(S, R, starts, table):
    """the sum over the windows of the normalised weight at every position of the axis"""
    tot = np.zeros(S, dtype=np.float64)
    for s, row in zip(starts, table):
        n = min(R, S - s)
        tot[s:s + n] += row[:n]
        assert np.all(row[n:] == 0.0), 'a weight beyond the end of the volume'
    return tot


@pytest.mark.parametrize('S,R,overlap,want', [(11, 4, 0.5, [0, 2, 4, 6, 7]), (13, 8, 0.5, [0, 4, 5]), (16, 8, 0.5, [0, 4, 8]),
                                              (5, 8, 0.5, [0]), (16, 4, 0.0, [0, 4, 8, 12]), (10, 4, 0.0, [0, 4, 6]), (8, 8, 0.5, [0])])
def test_known_starts(S, R, overlap, want):
    assert product_axis(S, R, overlap)[0] == want
    assert WR.axis_starts(S, R, overlap) == want


def random_axes(n, seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 41)), int(rng.integers(1, 41)), float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.6, 0.75, 0.9, 0.99])))
            for _ in range(n)]


@pytest.mark.parametrize('mode', ['gaussian', 'constant'])
def test_random_axes_cover_the_volume_and_sum_to_one(mode):
    short = 0
    for S, R, overlap in random_axes(300, 7) + [(5, 8, 0.5), (1, 1, 0.0), (40, 1, 0.5), (3, 40, 0.9)]:
        starts, table = product_axis(S, R, overlap, mode)
        assert all(b >= a for a, b in zip(starts, starts[1:])), 'starts decrease'
        assert starts[0] == 0 and all(0 <= s < S for s in starts), 'a start outside the volume'
        assert starts[-1] + R == max(S, R), 'the last window does not end at the end'
        assert int(WR.axis_coverage(S, starts, R).min()) >= 1, 'a position no window holds'
        tot = axis_sum(S, R, starts, table)
        assert float(np.abs(tot - 1.0).max()) <= 1e-12, (S, R, overlap, float(np.abs(tot - 1.0).max()))
        assert np.all(table >= 0.0) and np.all(table <= 1.0)
        short += S < R
        rs, rt = WR.axis_table(S, R, overlap, mode)                  # product plan == reference plan
        assert rs == starts
        assert float(np.abs(rt - table).max()) <= 1e-15
    assert short > 20


def test_tiling_without_overlap_has_weights_of_exactly_one():
    for mode in ('gaussian', 'constant'):
        for S, R in ((16, 4), (8, 8), (40, 10), (9, 3)):
            starts, table = product_axis(S, R, 0.0, mode)
            assert starts == list(range(0, S, R)) and np.all(table == 1.0)


def test_constant_importance_halves_doubly_covered_positions():
    starts, table = product_axis(16, 8, 0.5, 'constant')
    assert starts == [0, 4, 8]
    assert np.array_equal(table, [[1, 1, 1, 1, .5, .5, .5, .5], [.5] * 8, [.5, .5, .5, .5, 1, 1, 1, 1]])
    starts, table = product_axis(13, 8, 0.5, 'constant')            # 0,4,5: positions 5..7 lie in all three windows
    cover = WR.axis_coverage(13, starts, 8)
    for s, row in zip(starts, table):
        assert np.array_equal(row, 1.0 / cover[s:s + 8])


def test_three_axes_are_planned_independently():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    shape, roi = (13, 9, 16), (8, 16, 8)
    starts, tables = infer.window_plan(shape, roi, 0.5, 'gaussian', 0.125)
    rstarts, rtables = WR.plan(shape, roi, 0.5, 'gaussian', 0.125)
    assert [list(s) for s in starts] == rstarts == [[0, 4, 5], [0], [0, 4, 8]]
    for a in range(3):
        assert float(np.abs(tables[a] - rtables[a]).max()) <= 1e-15
    # the 3-D weights of all windows at every voxel sum to 1
    tot = np.zeros(shape)
    for iz, z in enumerate(starts[0]):
        for iy, y in enumerate(starts[1]):
            for ix, x in enumerate(starts[2]):
                w = tables[0][iz][:, None, None] * tables[1][iy][None, :, None] * tables[2][ix][None, None, :]
                n = [min(r, s - o) for r, s, o in zip(roi, shape, (z, y, x))]
                tot[z:z + n[0], y:y + n[1], x:x + n[2]] += w[:n[0], :n[1], :n[2]]
    assert float(np.abs(tot - 1.0).max()) <= 1e-12


def test_plan_and_spec_refuse_bad_arguments():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    for kw, word in ((dict(overlap=1.0), 'overlap'), (dict(overlap=-0.1), 'overlap'), (dict(mode='linear'), 'mode'),
                     (dict(sigma_scale=0.0), 'sigma_scale'), (dict(sigma_scale=-1.0), 'sigma_scale')):
        with pytest.raises(ValueError, match=word):
            infer.window_plan((8, 8, 8), (4, 4, 4), **kw)
        with pytest.raises(ValueError, match=word):
            infer.WindowSpec((4, 4, 4), **kw)
    for roi in ((4, 4), (4, 0, 4), (4, 4, -4), 4):
        with pytest.raises(ValueError, match='roi'):
            infer.window_plan((8, 8, 8), roi)
        with pytest.raises(ValueError, match='roi'):
            infer.WindowSpec(roi)
    with pytest.raises(ValueError, match='batch'):
        infer.WindowSpec((4, 4, 4), batch=0)
    spec = infer.WindowSpec([8, 16, 8])
    assert (spec.roi, spec.overlap, spec.mode, spec.sigma_scale, spec.batch, spec.skip_empty) == ((8, 16, 8), 0.5, 'gaussian', 0.125, None, True)
    spec.check_resolution(8)
    with pytest.raises(ValueError, match=r'\(8, 16, 8\).*resolution 16'):
        spec.check_resolution(16)
    with pytest.raises(ValueError, match='resolution 16'):
        infer.StageSpec(None, [0.0], [1.0], 16, window=spec)
    assert infer.StageSpec(None, [0.0], [1.0], 8, window=spec).window is spec and infer.StageSpec(None, [0.0], [1.0], 8).window is None
    with pytest.raises(ValueError, match='resolution 16'):
        infer.segment_volume(None, None, None, [0.0], [1.0], 16, window=spec)
    with pytest.raises(ValueError, match='resolution 16'):
        infer.segment_scan(None, None, (1.0, 1.0, 1.0), [0.0], [1.0], 16, window=spec)


REQUIRED = ['--in_locs', 'a,b', '--modalities', 't1ce,flair', '--tumor_model', 'm', '--tumor_prepro', 'p.npy']


def test_window_flags():
    import bts_amd  # noqa: F401
    from bts_amd import test as T
    plain = T.parse_args(REQUIRED)
    assert T.window_kwargs(plain) is None
    assert not any(k.startswith('window') for k in vars(plain))
    a = T.parse_args(REQUIRED + ['--window', '8,16,8', '--window_overlap', '0.25'])
    assert T.window_kwargs(a) == {'roi': (8, 16, 8), 'overlap': 0.25, 'mode': 'gaussian', 'batch': None}
    b = T.parse_args(REQUIRED + ['--window', 'crop', '--window_mode', 'constant', '--window_batch', '3'])
    assert T.window_kwargs(b) == {'roi': 'crop', 'overlap': 0.5, 'mode': 'constant', 'batch': 3}
    for bad in (['--window', '8,16,8', '--window_overlap', '1.0'], ['--window', '8,16,8', '--window_overlap', '-0.5'],
                ['--window', '8,16'], ['--window', '8,x,8'], ['--window', '8,0,8'], ['--window', '8,16,8', '--window_mode', 'linear'],
                ['--window', '8,16,8', '--window_batch', '0'], ['--window_overlap', '0.25']):
        with pytest.raises(SystemExit):
            T.parse_args(REQUIRED + bad)


A = 1 << 20                         # a plausible, never dereferenced address


def ints(*v):
    return ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)


def floats(*v):
    return ctypes.cast((ctypes.c_float * len(v))(*v), ctypes.c_void_p)


def test_argument_validation_without_gpu():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    L = lib()
    cap = L._bts_window_batch_max()
    assert cap == 16
    z3, f1, ms = ints(0, 0, 0), ints(0), floats(0.0, 1.0)

    def gather(D=8, H=8, W=8, C=2, R=(4, 4, 4), B=1, starts=z3, flips=f1, mean=ms, std=ms):
        return L._bts_window_gather(A, A + (1 << 24), D, H, W, C, R[0], R[1], R[2], B, starts, flips, mean, std, None)

    def accumulate(pred=A, acc=A + (1 << 24), n=(1, 1, 1), D=8, H=8, W=8, K=3, R=(4, 4, 4), B=1, starts=z3, flips=f1, rows=z3):
        return L._bts_window_accumulate(pred, acc, A, A, A, n[0], n[1], n[2], D, H, W, K, R[0], R[1], R[2], B, starts, flips, rows, 1.0, None)

    SHAPE, UNSUPPORTED = -1, -3
    for bad in (dict(D=0), dict(H=-1), dict(W=0), dict(C=0), dict(R=(0, 4, 4)), dict(R=(4, 4, -4))):
        assert gather(**bad) == SHAPE, bad
    assert gather(C=17) == UNSUPPORTED
    assert gather(B=0) == UNSUPPORTED and gather(B=cap + 1) == UNSUPPORTED
    assert gather(flips=ints(8)) == SHAPE and gather(flips=ints(-1)) == SHAPE
    assert gather(starts=ints(-1, 0, 0)) == SHAPE and gather(starts=ints(0, 8, 0)) == SHAPE and gather(starts=ints(0, 0, 8)) == SHAPE
    assert gather(B=2, starts=ints(0, 0, 0, 0, 0, 9), flips=ints(0, 0), mean=floats(0, 0, 0, 0), std=floats(1, 1, 1, 1)) == SHAPE
    assert gather(starts=None) == SHAPE and gather(flips=None) == SHAPE and gather(mean=None) == SHAPE and gather(std=None) == SHAPE

    for bad in (dict(D=0), dict(K=0), dict(R=(4, 0, 4)), dict(n=(0, 1, 1)), dict(n=(1, 1, -1))):
        assert accumulate(**bad) == SHAPE, bad
    assert accumulate(B=0) == UNSUPPORTED and accumulate(B=cap + 1) == UNSUPPORTED
    assert accumulate(flips=ints(8)) == SHAPE
    assert accumulate(starts=ints(0, -1, 0)) == SHAPE and accumulate(starts=ints(8, 0, 0)) == SHAPE
    assert accumulate(rows=ints(1, 0, 0)) == SHAPE and accumulate(rows=ints(0, 0, -1)) == SHAPE and accumulate(rows=None) == SHAPE
    assert accumulate(n=(2, 1, 1), rows=ints(2, 0, 0)) == SHAPE
    # acc aliasing pred: the same buffer, pred starting inside acc, acc starting inside pred
    assert accumulate(pred=A, acc=A) == UNSUPPORTED
    assert accumulate(pred=A + 8 * 8 * 8 * 3 * 4 - 4, acc=A) == UNSUPPORTED
    assert accumulate(pred=A, acc=A + 4 * 4 * 4 * 3 * 4 - 4) == UNSUPPORTED

    def occupancy(n=(1, 1, 1), D=8, H=8, W=8, R=(4, 4, 4)):
        return L._bts_window_occupancy(A, A, A, n[0], n[1], n[2], D, H, W, R[0], R[1], R[2], None)

    for bad in (dict(n=(0, 1, 1)), dict(D=0), dict(W=-3), dict(R=(4, 4, 0)), dict(n=(1 << 11, 1 << 11, 1 << 11))):
        assert occupancy(**bad) == SHAPE, bad
