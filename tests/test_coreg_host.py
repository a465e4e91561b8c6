"""CPU: the host side of rigid co-registration by mutual information (bts_amd.coreg) and the float64 / integer
restatement tests/coreg_ref.py that the device tests compare against.

Recovery (test_recovery): fixed grid 28x33x25 at 6 mm, moving grid 21x37x27 at (8.5, 5.4, 5.8) mm, the analytic phantom of coreg_ref with
2 % noise, levels scaled to the 6 mm voxels (lattices of 12 and 6 mm; steps 8 mm / 4 deg -> 2 mm, then 2 mm / 1 deg -> 0.125 mm), 32 bins,
the numpy evaluator plugged into coreg.search through coreg.coregister.  Mean target registration error over the fixed voxels inside the
head, in fixed voxels, measured with this reference on the CPU (the error of the headers alone in brackets):

  (9, -7, 6 mm; 4, -3, 5 deg)                          0.204   (2.28)
  (-11, 5, 8 mm; -6, 5, 2 deg)                         0.190   (2.55)
  the identity                                         0.097   (0.00)
  same grid, (7.3, -4.1, 2.6) mm, no rotation          0.158   (1.46)

Each pose is held to twice its own figure (the search is deterministic: the margin is for another libm), and all of them to the issue's
criterion, a mean error of at most 0.5 fixed voxel.  The same-grid translation is the worst case of the partial-volume artefact: between
two identical grids and without rotation every lattice point has the same eight weights, the histogram is a convex mixture of the eight
grid-aligned ones, and the score peaks ON the grid -- the search ends on (6, -6, 0) mm, the aligned translation nearest to the truth,
0.579 voxel away.  coregister then refines by the parabola through the scores of the aligned neighbours (`refined`), which is the figure
above; test_same_grid_search_ends_on_the_grid pins both halves."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import coreg_ref as R  # noqa: E402

import bts_amd  # noqa: E402,F401
from bts_amd import coreg  # noqa: E402

Q = 32
LEVELS = ((12.0, 8.0, 4.0, 2.0), (6.0, 2.0, 1.0, 0.125))
FIXED6, MOVING6 = ((28, 33, 25), (6.0, 6.0, 6.0)), ((21, 37, 27), (8.5, 5.4, 5.8))
POSES = {'pose_a': (FIXED6, MOVING6, (9.0, -7.0, 6.0, 4.0, -3.0, 5.0), 0.204),
         'pose_b': (FIXED6, MOVING6, (-11.0, 5.0, 8.0, -6.0, 5.0, 2.0), 0.190),
         'identity': (FIXED6, MOVING6, (0.0,) * 6, 0.097),
         'same_grid': (FIXED6, FIXED6, (7.3, -4.1, 2.6, 0.0, 0.0, 0.0), 0.158)}
_recovered = {}


def loop_hist(qf, qm, origin, stride, counts, m, bins):
    """the rule of include/bts_hip.h, point by point"""
    hist = np.zeros((bins, bins), dtype=np.int64)
    nm = qm.shape
    for l0 in range(counts[0]):
        for l1 in range(counts[1]):
            for l2 in range(counts[2]):
                f = [origin[j] + (l0, l1, l2)[j] * stride[j] for j in range(3)]
                a = int(qf[f[0], f[1], f[2]])
                c = [((m[j][0] * f[0] + m[j][1] * f[1]) + m[j][2] * f[2]) + m[j][3] for j in range(3)]
                if not all(0.0 <= c[j] <= nm[j] - 1 for j in range(3)):
                    continue
                i = [int(np.floor(c[j])) for j in range(3)]
                r = [int(np.floor((c[j] - i[j]) * Q + 0.5)) for j in range(3)]
                assert all(0 <= v <= Q for v in r)
                for d0 in (0, 1):
                    for d1 in (0, 1):
                        for d2 in (0, 1):
                            d = (d0, d1, d2)
                            b = int(qm[tuple(min(i[j] + d[j], nm[j] - 1) for j in range(3))])
                            w = 1
                            for j in range(3):
                                w *= r[j] if d[j] else Q - r[j]
                            hist[a, b] += w
    return hist


@pytest.mark.parametrize('name,m', [('identity', R.shift(0, 0, 0)), ('integer shift', R.shift(1, -2, 1)), ('half voxel', R.shift(0.5, 0.5, 0.5)),
                                    ('rigid', R.voxel_map((0.4, -0.3, 0.6, 7.0, -5.0, 9.0), (5, 6, 7), (1.0, 0.8, 0.7), (6, 5, 4), (0.9, 1.1, 1.2)))])
def test_vectorised_reference_equals_the_rule(name, m):
    bins = 8
    rng = np.random.default_rng(3)
    qf, qm = rng.integers(0, bins, (5, 6, 7)).astype(np.uint8), rng.integers(0, bins, (6, 5, 4)).astype(np.uint8)
    for origin, stride, counts in (((0, 0, 0), (1, 1, 1), (5, 6, 7)), ((1, 0, 1), (2, 3, 2), (2, 2, 3))):
        want = loop_hist(qf, qm, origin, stride, counts, m, bins)
        got = R.joint_hist_pv(qf, qm, origin, stride, counts, m[None], bins)[0]
        assert np.array_equal(got, want), name
        assert int(got.sum()) % Q ** 3 == 0
    if name == 'identity':
        assert int(R.joint_hist_pv(qf, qm, (0, 0, 0), (1, 1, 1), (5, 6, 7), m[None], bins).sum()) == 5 * 5 * 4 * Q ** 3


def test_no_case_of_the_device_tests_has_a_tie():
    """the exact equality tests/test_coreg_gpu.py asserts rests on this: on no lattice point of any case could the coordinate's last
    bit decide (and dyadic maps are exact either way)"""
    for name, fs, ms, mats in R.hist_cases():
        for origin, stride, counts in R.LATTICES:
            assert R.ties(mats, origin, stride, counts) == 0, (name, origin, stride)
    assert R.ties(R.shift(1e-10, 0, 0)[None], (0, 0, 0), (1, 1, 1), (3, 3, 3)) == 27       # and `ties` does see one


def test_quantize_edges():
    x = np.array([-1.0, 0.0, 0.25, 0.5, 0.999, 1.0, 2.0, np.nan], dtype=np.float32)
    assert R.quantize(x, 0.0, 1.0, 4).tolist() == [0, 0, 1, 2, 3, 3, 3, 0]
    assert np.array_equal(coreg.quantize_host(x, 0.0, 1.0, 4), R.quantize(x, 0.0, 1.0, 4))


def test_nmi():
    rng = np.random.default_rng(0)
    outer = np.outer(rng.integers(1, 50, 7), rng.integers(1, 50, 7))
    assert abs(coreg.nmi(outer) - 1.0) < 1e-12
    assert abs(coreg.nmi(np.diag([5, 1, 0, 9, 2])) - 2.0) < 1e-12
    assert coreg.nmi(np.zeros((4, 4), dtype=np.int64)) == 0.0
    assert coreg.nmi(np.diag([0, 7, 0])) == 1.0                      # one occupied bin: no entropy to share
    assert coreg.score(np.full((2, 2), Q ** 3), 100, 0.5) == -np.inf and coreg.score(np.full((2, 2), Q ** 3), 8, 0.5) > 0


def test_rigid_matrix():
    c = np.array([3.0, -2.0, 5.0])
    p = (4.0, -1.5, 2.0, 10.0, -20.0, 30.0)
    m = coreg.rigid_matrix(p, c)
    rot = m[:3, :3]
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(rot) - 1.0) < 1e-12
    assert np.array_equal(m[3], [0, 0, 0, 1])
    assert np.abs(coreg.rigid_matrix((0, 0, 0) + p[3:], c) @ np.append(c, 1.0) - np.append(c, 1.0)).max() < 1e-12
    assert np.abs(m @ np.append(c, 1.0) - np.append(c + p[:3], 1.0)).max() < 1e-12
    # the order: the rotation about x first, then y, then z
    assert np.abs(rot - R.rotation(0, 0, 30.0) @ R.rotation(0, -20.0, 0) @ R.rotation(10.0, 0, 0)).max() < 1e-12
    # so the reversed motion is the rotations undone in the opposite order, not rigid_matrix(-p)
    inv = np.linalg.inv(m)
    assert np.abs(inv[:3, :3] - R.rotation(-10.0, 0, 0) @ R.rotation(0, 20.0, 0) @ R.rotation(0, 0, -30.0)).max() < 1e-12
    assert np.abs(inv - coreg.rigid_matrix(tuple(-v for v in p), c)).max() > 1e-2
    one = (0.0, 0.0, 0.0, 0.0, 25.0, 0.0)                            # a single rotation does reverse by its negative
    assert np.abs(np.linalg.inv(coreg.rigid_matrix(one, c)) - coreg.rigid_matrix(tuple(-v for v in one), c)).max() < 1e-12
    with pytest.raises(ValueError):
        coreg.rigid_matrix((1, 2, 3), c)


def test_corrected_affine_reaches_the_conformer():
    from bts_amd.infer import Conformer
    a_f = R.grid_affine((20, 24, 18), (1.0, 0.9, 1.2))
    a_m = R.grid_affine((16, 30, 21), (1.3, 0.8, 1.1), (2.0, -1.0, 0.5))
    t = coreg.rigid_matrix((3.0, -2.0, 1.5, 4.0, -6.0, 2.0), (1.0, 2.0, 3.0))
    plan = Conformer('LPS').plan([(20, 24, 18), (16, 30, 21)], [a_f, np.linalg.inv(t) @ a_m])
    want = (np.linalg.inv(a_m) @ t @ plan['target_affine'])[:3]
    assert np.abs(plan['matrices'][1] - want).max() < 1e-9
    assert np.array_equal(plan['matrices'][0], Conformer('LPS').plan([(20, 24, 18)], [a_f])['matrices'][0])


def test_search_is_a_compass_search():
    """a synthetic evaluate: the score grows towards a known point; one call per sweep, 13 candidates, bounds respected"""
    target = np.array([3.0, -1.0, 0.0, 2.0, 0.0, 0.0])
    calls = []

    def evaluate(level, plist):
        calls.append(len(plist))
        out = []
        for p in plist:
            d = float(np.abs(np.array(p) - target).sum())
            h = np.zeros((2, 2), dtype=np.int64)
            k = int(round(1000 * min(d, 40.0) / 40.0))               # d = 0: diagonal (NMI 2); d large: an outer product (NMI 1)
            h[0, 0] = h[1, 1] = (2000 - k) * Q ** 3
            h[0, 1] = h[1, 0] = k * Q ** 3
            out.append(h)
        return out
    p, trace = coreg.search(evaluate, [coreg.Level(4.0, 4.0, 1.0, 4000), coreg.Level(1.0, 1.0, 0.125, 4000)], (30.0, 20.0))
    assert p == tuple(target.tolist())
    assert max(calls) == 13 and len(calls) == len(trace) and all(t[4] == n for t, n in zip(trace, calls))
    p2, trace2 = coreg.search(evaluate, [coreg.Level(4.0, 4.0, 1.0, 4000), coreg.Level(1.0, 1.0, 0.125, 4000)], (30.0, 20.0))
    assert p2 == p and trace2 == trace                                # deterministic
    pb, _ = coreg.search(evaluate, [coreg.Level(4.0, 4.0, 1.0, 4000)], (2.0, 1.0))
    assert all(abs(v) <= 2.0 for v in pb[:3]) and all(abs(v) <= 1.0 for v in pb[3:])
    # too little overlap everywhere: nothing is better than the start
    p0, _ = coreg.search(evaluate, [coreg.Level(4.0, 4.0, 1.0, 10 ** 9)], (30.0, 20.0))
    assert p0 == (0.0,) * 6


def _recover(key):
    if key not in _recovered:
        (fs, fsp), (ms, msp), pose, _ = POSES[key]
        a_f = R.grid_affine(fs, fsp)
        centre = (a_f @ np.array([(n - 1) // 2 for n in fs] + [1.0]))[:3]
        truth = coreg.rigid_matrix(pose, centre)
        f, a_f, m, a_m = R.phantom_pair(fs, fsp, ms, msp, truth, moving_offset=(1.3, -0.7, 2.1) if ms != fs else (0.0, 0.0, 0.0))
        r = coreg.coregister(f, a_f, m, a_m, levels=LEVELS, evaluate=R.joint_hist_pv)
        tre, before = R.mean_tre(r.matrix, truth, fs, a_f), R.mean_tre(np.eye(4), truth, fs, a_f)
        print('%s: pose %s -> %s, mean TRE %.4f voxel (headers alone %.4f), NMI %.5f -> %.5f, %d evaluations, overlap %.3f'
              % (key, pose, tuple(round(v, 3) for v in r.params), tre, before, r.nmi_before, r.nmi_after, r.evaluations, r.overlap))
        _recovered[key] = (r, tre, a_m)
    return _recovered[key]


@pytest.mark.parametrize('key', sorted(POSES))
def test_recovery(key):
    r, tre, a_m = _recover(key)
    assert tre <= 2.0 * POSES[key][3]
    assert r.nmi_after >= r.nmi_before and 0.5 <= r.overlap <= 1.0
    assert r.evaluations == sum(t[4] for t in r.trace) + 2 + (7 if r.refined else 0) and r.refined == (key == 'same_grid')
    assert np.abs(r.affine - np.linalg.inv(r.matrix) @ a_m).max() < 1e-12


@pytest.mark.parametrize('key', sorted(POSES))
def test_recovery_within_half_a_voxel(key):
    assert _recover(key)[1] <= 0.5


def test_same_grid_search_ends_on_the_grid():
    """the artefact and its remedy: the search itself ends on the grid-aligned translation nearest to the truth; the refinement moves every
    axis towards the truth by less than half a voxel"""
    r, tre, _ = _recover('same_grid')
    end = r.trace[-1][1]
    assert end == (6.0, -6.0, 0.0, 0.0, 0.0, 0.0) and r.refined and r.params[3:] == (0.0, 0.0, 0.0)
    truth = POSES['same_grid'][2]
    for j in range(3):
        assert abs(r.params[j] - end[j]) <= 3.0 and abs(r.params[j] - truth[j]) < abs(end[j] - truth[j])
    assert coreg.parabola_vertex(1.0, 2.0, 1.0) == 0.0 and coreg.parabola_vertex(1.0, 2.0, 2.0) == 0.5
    assert coreg.parabola_vertex(3.0, 2.0, 1.0) == 0.0 and coreg.parabola_vertex(-np.inf, 2.0, 1.0) == 0.0
    # the same volumes with truthful headers: the search does not move, and headers that nothing moved are kept exactly
    fs, fsp = FIXED6
    f, a_f, m, a_m = R.phantom_pair(fs, fsp, fs, fsp, np.eye(4), moving_offset=(0.0, 0.0, 0.0))
    still = coreg.coregister(f, a_f, m, a_m, levels=LEVELS, evaluate=R.joint_hist_pv)
    assert still.params == (0.0,) * 6 and not still.refined and np.array_equal(still.affine, a_m)
    assert coreg.grid_aligned(R.shift(3, -2, 0)) and not coreg.grid_aligned(R.shift(0.5, 0, 0)) and not coreg.grid_aligned(R.thirteen()[0])


def test_coregister_case_keeps_the_reference():
    (fs, fsp), (ms, msp), pose, _ = POSES['identity']
    r, _, a_m = _recover('identity')
    a_f = R.grid_affine(fs, fsp)
    f, _, m, _ = R.phantom_pair(fs, fsp, ms, msp, np.eye(4))
    affines, results = coreg.coregister_case([f, m], [a_f, a_m], levels=LEVELS, evaluate=R.joint_hist_pv)
    assert results[0] is None and np.array_equal(affines[0], a_f)
    assert results[1].params == r.params and np.array_equal(affines[1], r.affine)
    with pytest.raises(RuntimeError):
        coreg.coregister(f, a_f, m, a_m)                             # numpy volumes and the device evaluator
    with pytest.raises(ValueError):
        coreg.coregister(f, a_f, m, a_m, bins=1, evaluate=R.joint_hist_pv)
    with pytest.raises(ValueError):
        coreg.coregister(np.zeros_like(f), a_f, m, a_m, evaluate=R.joint_hist_pv)


BASE = ['--in_locs', 'a', '--modalities', 't1ce,flair', '--tumor_prepro', 'p', '--tumor_model', 'm']


def test_command_line_flags(capsys):
    from bts_amd import test as T
    plain = T.parse_args(BASE)
    assert not any(hasattr(plain, k) for k in ('coregister', 'coregister_max_mm', 'coregister_max_deg', 'coregister_bins'))
    assert T.coregister_kwargs(plain) is None and T.coregister_kwargs(T.parse_args(BASE + ['--conform'])) is None
    a = T.parse_args(BASE + ['--conform', '--coregister'])
    assert a.coregister is True and T.coregister_kwargs(a) == {'bounds': (30.0, 20.0), 'bins': 32}
    a = T.parse_args(BASE + ['--conform', 'RAS', '--coregister', '--coregister_max_mm', '12.5', '--coregister_max_deg', '7', '--coregister_bins', '16'])
    assert T.coregister_kwargs(a) == {'bounds': (12.5, 7.0), 'bins': 16}
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ['--coregister'])
    err = capsys.readouterr().err
    assert '--coregister' in err and '--conform' in err
    for bad in (['--coregister_max_mm', '0'], ['--coregister_max_mm', 'nan'], ['--coregister_max_deg', '181'], ['--coregister_max_deg', '-1'],
                ['--coregister_bins', '1'], ['--coregister_bins', '65']):
        with pytest.raises(SystemExit):
            T.parse_args(BASE + ['--conform', '--coregister'] + bad)
    with pytest.raises(SystemExit):
        T.parse_args(BASE + ['--conform', '--coregister_bins', '16'])   # a bound without --coregister
    capsys.readouterr()
