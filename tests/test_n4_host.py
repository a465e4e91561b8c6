"""CPU: the host side of N4 bias-field correction (bts_amd.n4) and the float64 restatement tests/n4_ref.py that the GPU tests compare the
kernels with: the two statements of every pass (point by point, and vectorised) agree; the basis, the lattice refinement and the
sharpening behave as they must; specs and flags are refused by name; and `n4.correct`, driven by the numpy evaluator, recovers the field
of an analytic phantom."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import n4_ref as R  # noqa: E402

EPS = 2.0 ** -53


def n4():
    import bts_amd  # noqa: F401
    from bts_amd import n4 as mod
    return mod


# ---- basis and refinement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extent,mesh', [(1, 1), (7, 1), (19, 2), (37, 4), (23, 8), (240, 32)])
def test_weights_are_a_partition_of_unity(extent, mesh):
    p = np.arange(extent)
    i, w = n4().bspline_weights(p, extent, mesh)
    assert w.shape == (extent, 4) and (w >= 0).all()
    assert np.abs(w.sum(axis=1) - 1.0).max() <= 8 * EPS
    assert i.min() >= 0 and i.max() <= mesh - 1
    ir, wr = R.weights(p, extent, mesh)
    assert np.array_equal(i, ir) and np.array_equal(w, wr)              # the module and the restatement: the same bits
    for k in (0, extent // 2, extent - 1):
        ip, wp = R.weights_pointwise(k, extent, mesh)
        assert ip == i[k] and wp == list(w[k])


def test_lattice_geometry():
    g = n4().lattice_geometry
    assert g((19, 23, 37), 4) == ((2, 2, 2), (4, 4, 4), (5, 6, 9))
    assert g((19, 23, 37), 1) == ((0, 0, 0), (1, 1, 1), (19, 23, 37))
    assert g((3, 23, 37), 4) == ((1, 2, 2), (3, 4, 4), (1, 6, 9))          # a stride never passes the extent
    for shape, s in (((19, 23, 37), 4), ((3, 5, 2), 7)):
        o, st, n = g(shape, s)
        assert (o, n) == R.lattice(shape, st)
    with pytest.raises(ValueError):
        g((19, 23), 4)
    with pytest.raises(ValueError):
        g((19, 23, 37), 0)


@pytest.mark.parametrize('mesh', [(1, 1, 1), (2, 3, 1), (4, 8, 2)])
def test_refinement_leaves_the_spline_unchanged(mesh):
    """the refined lattice is the same function: at every voxel of a 17x29x21 grid the two evaluations differ by at most
    64 * 2^-53 * sum |phi w| (64 terms each; the prototype saw < 1e-10 absolute on fields of order 0.3)"""
    rng = np.random.default_rng(sum(mesh))
    phi = 0.3 * rng.standard_normal(tuple(m + 3 for m in mesh))
    fine = n4().refine_lattice(phi)
    assert fine.shape == tuple(2 * m + 3 for m in mesh)
    shape = (17, 29, 21)
    a, scale = R.spline(phi, shape, (1, 1, 1), mesh)
    b, _ = R.spline(fine, shape, (1, 1, 1), tuple(2 * m for m in mesh))
    assert (np.abs(a - b) <= 64 * EPS * scale).all()                       # scale: sum |phi w| of the lattice that was refined
    assert np.abs(a - b).max() < 1e-10
    with pytest.raises(ValueError):
        n4().refine_lattice(np.zeros((3, 4, 4)))


# ---- the two statements of every pass -----------------------------------------------------------------------------------------------
def small_case(seed=0, shape=(7, 9, 11), stride=(1, 2, 1)):
    rng = np.random.default_rng(seed)
    x = (50.0 + 100.0 * rng.random(shape)).astype(np.float32)
    x[rng.random(shape) < 0.2] = 0.0
    x[0, 0, 0], x[1, 2, 3], x[2, 2, 2] = np.inf, np.nan, -5.0
    mask = rng.random(shape) < 0.8
    return x, mask, stride


def test_log_lattice_masks_what_it_must():
    x, mask, _ = small_case()
    o, stride, n = n4().lattice_geometry(x.shape, 2)                      # the module's lattice is the one the restatement gathers
    assert stride == (2, 2, 2) and (o, n) == R.lattice(x.shape, stride)
    v, lm = R.log_lattice(x, mask, stride)
    assert v.shape == n and lm.dtype == np.uint8
    for l in np.ndindex(*n):
        p = tuple(oo + ll * s for oo, ll, s in zip(o, l, stride))
        inside = bool(mask[p]) and np.isfinite(x[p]) and x[p] > 0
        assert lm[l] == inside and v[l] == (np.log(np.float64(x[p])) if inside else 0.0)
    assert R.log_lattice(x, None, stride)[1].sum() > lm.sum()


@pytest.mark.parametrize('bins', [2, 7, 200])
def test_histogram_pointwise_equals_vectorised(bins):
    x, mask, stride = small_case(1)
    v, lm = R.log_lattice(x, mask, stride)
    f = 0.1 * np.random.default_rng(2).standard_normal(v.shape)
    r, lo, hi, h = R.hist(v, f, lm, bins)
    rp, lop, hip, hp = R.hist_pointwise(v, f, lm, bins)
    assert np.array_equal(r, rp) and (lo, hi) == (lop, hip) and np.array_equal(h, hp)
    assert int(h.sum()) == int(lm.sum()) * R.Q24 and h.min() >= 0
    table = n4().sharpen_table(h, lo, hi)                                   # ... and it is what the module's sharpening takes
    assert table.shape == (bins,) and np.isfinite(table).all()
    one = n4().correct(np.exp(v).astype(np.float32), lm, n4().N4Spec(shrink=1, levels=1, iters=1, bins=bins), evaluate=R.NumpyEvaluator())
    assert one.sweeps == (1,) and one.points == int(lm.sum())             # the loop's first sweep runs on this very histogram
    empty = R.hist(v, f, np.zeros_like(lm), bins)
    assert empty[1:3] == (np.inf, -np.inf) and not empty[3].any()
    flat = R.hist(np.ones_like(v), np.zeros_like(v), lm, bins)              # hi == lo: everything in bin 0
    assert flat[1] == flat[2] == 1.0 and int(flat[3][0]) == int(lm.sum()) * R.Q24


def test_residual_and_fit_and_spline_pointwise_equal_vectorised():
    x, mask, stride = small_case(3)
    shape = x.shape
    v, lm = R.log_lattice(x, mask, stride)
    r, lo, hi, h = R.hist(v, np.zeros_like(v), lm, 50)
    table = n4().sharpen_table(h, lo, hi)
    sl = (hi - lo) / 49
    res = R.residual(r, lm, table, lo, sl)
    assert np.abs(res - R.residual_pointwise(r, lm, table, lo, sl)).max() == 0.0
    for mesh in ((1, 1, 1), (2, 1, 3)):
        num, den, dphi, n, absn = R.fit(res, lm, shape, stride, mesh)
        nump, denp, dphip = R.fit_pointwise(res, lm, shape, stride, mesh)
        bound = 4 * np.maximum(n, 8) * EPS
        assert (np.abs(num - nump) <= bound * absn).all() and (np.abs(den - denp) <= bound * den).all()
        assert ((den > 0) == (denp > 0)).all() and (dphi[den == 0] == 0).all()
        ok = den > 0
        assert (np.abs(dphi - dphip)[ok] <= (2 * bound * (absn / np.where(ok, den, 1.0)))[ok] + 1e-300).all()
        phi = np.random.default_rng(4).standard_normal(tuple(m + 3 for m in mesh))
        f, scale = R.spline(phi, shape, stride, mesh)
        assert (np.abs(f - R.spline_pointwise(phi, shape, stride, mesh)) <= 256 * EPS * scale).all()


# ---- sharpening --------------------------------------------------------------------------------------------------------------------
def two_peaks(bins):
    k = np.arange(bins, dtype=np.float64)
    h = 4000.0 * np.exp(-0.5 * ((k - 0.3 * bins) / (0.04 * bins)) ** 2) + 2500.0 * np.exp(-0.5 * ((k - 0.7 * bins) / (0.05 * bins)) ** 2) + 3.0
    return np.rint(h * 4096.0).astype(np.int64)


@pytest.mark.parametrize('bins', [50, 200])
def test_sharpen_table_equals_the_transform_written_out(bins):
    """the FFT form against plain O(P^2) sums.  Both quotients carry the rounding of three transforms of P terms each and of the Wiener
    gain (at most 1 / (2 sqrt(noise)) = 5): an absolute error of the order P * 2^-53 * max|xbin| * sum(hist) in numerator and denominator,
    divided by the denominator at that bin.  Held to 64 times that; where the denominator is tiny the bound widens by itself"""
    h = two_peaks(bins)
    lo, hi = 3.9, 5.6
    e = n4().sharpen_table(h, lo, hi)
    ep, den = R.sharpen_pointwise(h, lo, hi)
    assert e.shape == (bins,) and np.isfinite(e).all()
    big = 2 ** (int(np.ceil(np.log2(bins))) + 1)
    sl = (hi - lo) / (bins - 1)
    reach = max(abs(lo - big * sl), abs(hi + big * sl))
    tol = 64 * big * EPS * 5.0 * reach * float(h.sum()) / np.maximum(np.abs(den), 1e-300)
    assert (np.abs(e - ep) <= tol).all()
    assert tol[den > 0.1 * den.max()].max() < 1e-6                        # ... and at the peaks the bound is tight


def test_sharpen_table_is_monotone_and_keeps_a_spike():
    """a Gaussian kernel has a monotone likelihood ratio, so the expected true value is non-decreasing in the observed one whatever the
    deconvolved histogram; a single spike is symmetric about its own centre and maps onto it"""
    bins, lo, hi = 200, 3.9, 5.6
    e = n4().sharpen_table(two_peaks(bins), lo, hi)
    assert (np.diff(e) >= -1e-9).all() and lo - 0.2 < e[0] < e[-1] < hi + 0.2
    sl = (hi - lo) / (bins - 1)
    h = np.zeros(bins, dtype=np.int64)
    h[77] = 12345 * R.Q24
    e = n4().sharpen_table(h, lo, hi)
    assert np.isfinite(e).all() and abs(e[77] - (lo + 77 * sl)) < 1e-9
    with pytest.raises(ValueError):
        n4().sharpen_table(h, 1.0, 1.0)


# ---- spec and flags ----------------------------------------------------------------------------------------------------------------
def test_spec_is_refused_by_name():
    m = n4()
    good = m.N4Spec()
    assert good == (4, 4, 50, 1e-3, (1, 1, 1), 200, 0.15, 0.01) and m.check_spec(good) == good
    bad = dict(shrink=[0, 1.5, True], levels=[0, 7, 2.0], iters=[0, -3], threshold=[-1e-9, float('nan'), 'x'], mesh=[(1, 1), (0, 1, 1), 3, (1, 1, 1.5)],
               bins=[1, 1025, 200.0], fwhm=[0, -1.0, float('inf')], noise=[0, -0.01, None])
    for field, values in bad.items():
        for val in values:
            with pytest.raises(ValueError, match=field):
                m.check_spec(good._replace(**{field: val}))
    with pytest.raises(ValueError, match='mesh'):
        m.check_spec(good._replace(mesh=(4, 1, 1), levels=6))              # 128 elements: past what the kernels take
    with pytest.raises(ValueError):
        m.check_spec((4, 4, 50, 1e-3, (1, 1, 1), 200, 0.15, 0.01))
    rec = m.spec_record(good._replace(iters=7))
    assert rec['mesh'] == [1, 1, 1] and m.spec_from_record(rec) == good._replace(iters=7)
    with pytest.raises(ValueError):
        m.spec_from_record({'shrink': 4})


def test_degenerate_masks_return_the_input():
    m = n4()
    ev = R.NumpyEvaluator()
    x, _, _ = R.phantom((10, 12, 9))
    spec = m.N4Spec(shrink=2, levels=2, iters=3)
    one = np.zeros(x.shape, dtype=bool)
    one[5, 7, 5] = True                                                    # a lattice point of stride 2 (origin 1), inside the head
    assert x[5, 7, 5] > 0
    for mask in (np.zeros(x.shape, dtype=bool), one):
        r = m.correct(x, mask, spec, evaluate=ev)
        assert np.array_equal(r.out, x) and r.out is not x and r.out.dtype == np.float32
        assert not r.phi.any() and r.phi.shape == (4, 4, 4) and r.sweeps == (0, 0) and r.cv == () and r.points == int(mask.sum())
    r = m.correct(np.zeros((4, 5, 6), dtype=np.float32), None, spec, evaluate=ev)        # nothing positive
    assert r.points == 0 and not r.out.any()
    flat = np.full((6, 7, 8), 3.0, dtype=np.float32)                       # single-valued: every level converges at once
    r = m.correct(flat, None, spec, evaluate=ev)
    assert np.array_equal(r.out, flat) and r.sweeps == (1, 1) and r.cv == (0.0, 0.0) and not r.phi.any()
    assert 'sweeps 1+1' in m.format_result('t1', r)
    with pytest.raises(ValueError):
        m.correct(np.zeros((4, 5), dtype=np.float32), None, spec, evaluate=ev)


def test_preprocess_flags():
    import bts_amd  # noqa: F401
    from bts_amd import preprocess as P
    base = ['--in_locs', 'a', '--modalities', 't1,t2', '--truth', 'seg']
    plain = P.parse_args(base)
    assert not any(k.startswith('bias') for k in vars(plain)) and P.bias_spec(plain) is None
    assert P.bias_spec(P.parse_args(base + ['--bias_correct'])) == n4().N4Spec()
    got = P.bias_spec(P.parse_args(base + ['--bias_correct', '--bias_shrink', '2', '--bias_levels', '3', '--bias_iters', '9', '--bias_threshold',
                                           '0.01', '--bias_fwhm', '0.2']))
    assert got == n4().N4Spec(shrink=2, levels=3, iters=9, threshold=0.01, fwhm=0.2)
    for extra in (['--bias_shrink', '2'], ['--bias_levels', '3'], ['--bias_iters', '9'], ['--bias_threshold', '0.01'], ['--bias_fwhm', '0.2'],
                  ['--bias_correct', '--bias_shrink', '0'], ['--bias_correct', '--bias_levels', '7'], ['--bias_correct', '--bias_iters', '0'],
                  ['--bias_correct', '--bias_threshold', '-1'], ['--bias_correct', '--bias_fwhm', '0']):
        with pytest.raises(SystemExit):
            P.parse_args(base + extra)


def test_test_flags():
    import bts_amd  # noqa: F401
    from bts_amd import test as T
    base = ['--in_locs', 'a', '--modalities', 't1,t2', '--tumor_model', 'm', '--tumor_prepro', 'p.npy']
    plain = T.parse_args(base)
    assert not any(k.startswith('bias') for k in vars(plain))
    assert T.bias_spec(T.parse_args(base + ['--bias_correct', '--bias_iters', '5'])) == n4().N4Spec(iters=5)
    recorded = n4().N4Spec(shrink=2, iters=30)
    assert T.bias_spec(plain, None, recorded) == recorded                                    # the record stands as it is
    assert T.bias_spec(T.parse_args(base + ['--bias_correct', '--bias_iters', '5']), None, recorded) == recorded._replace(iters=5)
    for extra in (['--bias_iters', '5'], ['--bias_shrink', '2'], ['--bias_fwhm', '0.1'], ['--bias_correct', '--bias_levels', '0']):
        with pytest.raises(SystemExit):
            T.parse_args(base + extra)


def test_prepro_file_without_the_flag_is_unchanged(tmp_path):
    """the record `preprocess` saves without --bias_correct against the dictionaries it has always saved, byte for byte"""
    import bts_amd  # noqa: F401
    from bts_amd import preprocess as P
    size = {'h': 8, 'w': 9, 'd': 10, 'c': 2}
    mean, std = np.array([1.0, 2.0]).reshape(1, 1, 1, 2), np.array([3.0, 4.0]).reshape(1, 1, 1, 2)
    for k, (kw, old) in enumerate([(dict(), {'size': size, 'norm': {'mean': mean, 'std': std}}),
                                   (dict(norm='case', clip=(0.5, 99.5)), {'size': size, 'norm': {'mode': 'case', 'clip': (0.5, 99.5), 'mean': mean, 'std': std}})]):
        np.save(str(tmp_path / ('new%d.npy' % k)), P.prepro_record(size, mean, std, **kw))
        np.save(str(tmp_path / ('old%d.npy' % k)), old)
        assert (tmp_path / ('new%d.npy' % k)).read_bytes() == (tmp_path / ('old%d.npy' % k)).read_bytes()
        assert P.load_bias(str(tmp_path / ('new%d.npy' % k))) is None
    spec = n4().N4Spec(iters=7)
    np.save(str(tmp_path / 'bias.npy'), P.prepro_record(size, mean, std, bias=spec))
    rec = np.load(str(tmp_path / 'bias.npy'), allow_pickle=True).item()
    assert rec['bias'] == n4().spec_record(spec) and rec['norm'].keys() == {'mean', 'std'}
    assert P.load_bias(str(tmp_path / 'bias.npy')) == spec and P.load_norm(str(tmp_path / 'bias.npy')).mode == 'dataset'


# ---- recovery ----------------------------------------------------------------------------------------------------------------------
def recover(shape, shrink):
    m = n4()
    x, tissue, logb = R.phantom(shape)
    clean, _, _ = R.phantom(shape, bias=False)
    r = m.correct(x, None, m.N4Spec(shrink=shrink, levels=3, iters=20), evaluate=R.NumpyEvaluator())
    out, _, logf = R.apply(x, r.phi, r.mesh)
    assert np.array_equal(out, r.out)
    after, floor = R.tissue_cv(r.out, tissue), R.tissue_cv(clean, tissue)
    err = R.field_error(logf, logb, tissue > 0)
    print('%s shrink %d: sweeps %s, CV before %s, after %s, without bias %s, field error %.4f' % (
        shape, shrink, r.sweeps, ['%.4f' % v for v in R.tissue_cv(x, tissue)], ['%.5f' % v for v in after], ['%.5f' % v for v in floor], err))
    return r, after, floor, err


def test_recovery_at_full_resolution():
    """40x48x36, shrink 1, 3 levels of 20 sweeps.  Measured with this reference: sweeps 20+20+14; per-tissue CV 0.2006 / 0.1426 / 0.0742
    before, 0.02312 / 0.02221 / 0.02163 after, 0.01998 / 0.02009 / 0.02022 for the same phantom without bias (ratios 1.157, 1.106, 1.070);
    RMS error of the log field over the head, means removed, 0.1012 of the true field's RMS (0.1770).  Held to the issue's conditions
    (1.5 x the noise floor, 0.2) and each figure to twice itself, the margin for another libm"""
    r, after, floor, err = recover((40, 48, 36), 1)
    assert all(a <= 1.5 * f for a, f in zip(after, floor)) and err <= 0.2
    assert all(a <= 2 * m for a, m in zip(after, (0.02312, 0.02221, 0.02163))) and err <= 2 * 0.1012
    assert len(r.sweeps) == 3 and max(r.sweeps) <= 20 and r.mesh == (4, 4, 4) and len(r.cv) == sum(r.sweeps)


def test_recovery_at_shrink_2():
    """80x96x72, shrink 2 (a 40x48x36 lattice), 3 levels of 20 sweeps.  Measured with this reference: sweeps 20+20+15; per-tissue CV after
    0.02288 / 0.02174 / 0.02087 against 0.02006 / 0.01998 / 0.02007 without bias (ratios 1.141, 1.088, 1.040); field error 0.0898.  The same
    conditions, and each figure held to twice itself"""
    r, after, floor, err = recover((80, 96, 72), 2)
    assert all(a <= 1.5 * f for a, f in zip(after, floor)) and err <= 0.2
    assert all(a <= 2 * m for a, m in zip(after, (0.02288, 0.02174, 0.02087))) and err <= 2 * 0.0898
    assert r.points == int((R.log_lattice(R.phantom((80, 96, 72))[0], None, (2, 2, 2))[1]).sum())
