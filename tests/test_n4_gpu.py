"""-m gpu: the six device passes of N4 bias-field correction (csrc/n4.hip through bts_amd.ops), `n4.correct` on top of them and the two
command lines, against the float64 restatement tests/n4_ref.py (whose two statements of every pass tests/test_n4_host.py proves equal).
No tolerance is taken from the kernels under test:

  lattice mask, r, lo, hi, histogram   equal: the coordinate, the subtraction, the bin number and its fraction are separately rounded
                                       fp64 operations on both sides, the histogram is integer
  v = log x                            2 ulp (ocml documents 1 ulp for the fp64 log, numpy's is within 1)
  residual                             4 * 2^-53 * max|E| + one ulp of r: three roundings of terms below max|E|, one of the difference
  num, den, dphi, the spline, sums     4 * max(n, 8) * 2^-53 * sum|term|: the any-order summation bound n * 2^-53 * sum|term| for each
                                       side plus the roundings of the terms; n the terms of a sum (the lattice points in a control
                                       point's support; 64 for the spline; the masked points for the sums of e and e^2)
  out, field                           1 fp32 ulp of the float32-rounded reference, at every voxel

Volumes are 19x23x37 and 17x29x21, odd and unequal, so no two axes can be confused and the 1024-point runs of the point-owning kernels
end mid-way (16169 points: sixteen workgroups)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import n4_ref as R  # noqa: E402
from guard_alloc import POISON, install  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SHAPES = [(19, 23, 37), (17, 29, 21)]
SHRINKS = [1, (2, 3, 2), 4, 20]                  # 20 passes the first extent of both volumes: that stride becomes the extent
MESHES = [(1, 1, 1), (2, 2, 2), (4, 8, 2)]
MASKS = ['full', 'half', 'one', 'empty', 'dirty']


def dev():
    return torch.device('cuda', 0)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def host(t):
    return t.cpu().numpy()


def stride_of(shape, shrink):
    return tuple(min(n, s) for n, s in zip(shape, shrink if isinstance(shrink, tuple) else (shrink,) * 3))


def volume(shape, kind, seed=0):
    """-> (x float32, mask or None): a positive textured volume under a smooth field; 'dirty' puts zeros, negatives, an inf and a NaN
    outside its mask (and a zero inside, which the x > 0 rule removes)"""
    rng = np.random.default_rng(seed + sum(shape))
    g = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing='ij')
    x = ((60.0 + 200.0 * rng.random(shape)) * np.exp(0.3 * g[0] - 0.2 * g[1] * g[2])).astype(np.float32)
    if kind == 'full':
        return x, None
    if kind == 'half':
        return x, rng.random(shape) < 0.5
    if kind == 'one':
        m = np.zeros(shape, dtype=bool)
        m[tuple(n // 2 for n in shape)] = True
        return x, m
    if kind == 'empty':
        return x, np.zeros(shape, dtype=bool)
    m = rng.random(shape) < 0.6
    out = np.argwhere(~m)
    x[tuple(out[0])], x[tuple(out[1])] = np.inf, np.nan
    for k in range(2, min(40, len(out))):
        x[tuple(out[k])] = 0.0 if k % 2 else -7.0
    x[tuple(np.argwhere(m)[3])] = 0.0
    return x, m


def ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


def lattice_inputs(shape, shrink, kind, seed=0):
    x, mask = volume(shape, kind, seed)
    stride = stride_of(shape, shrink)
    v, lm = R.log_lattice(x, mask, stride)
    f = 0.05 * np.random.default_rng(seed + 5).standard_normal(v.shape)
    return x, mask, stride, v, lm, f


# ---- bts_n4_log_lattice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', MASKS)
def test_log_lattice(kind):
    import bts_amd  # noqa: F401
    from bts_amd import n4, ops
    for shape in SHAPES:
        for shrink in SHRINKS:
            x, mask = volume(shape, kind)
            stride = stride_of(shape, shrink)
            if not isinstance(shrink, tuple):
                assert stride == n4.lattice_geometry(shape, shrink)[1]
            v, lm = R.log_lattice(x, mask, stride)
            for m in ((None,) if mask is None else (up(mask), up(mask.astype(np.uint8)))):
                gv, gl = ops.n4_log_lattice(up(x), m, stride)
                assert gv.dtype == torch.float64 and gl.dtype == torch.uint8 and tuple(gv.shape) == v.shape == tuple(gl.shape)
                assert np.array_equal(host(gl), lm), (shape, stride)
                assert (np.abs(host(gv) - v) <= 2 * np.spacing(np.abs(v))).all() and (host(gv)[lm == 0] == 0).all()
            if kind == 'one':
                assert lm.sum() <= 1
            if kind == 'empty':
                assert lm.sum() == 0


# ---- bts_n4_range_hist -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', [2, 200, 1024])
def test_histogram_equals_the_reference(bins):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    for shape, shrink, kind in ((SHAPES[0], 1, 'full'), (SHAPES[0], (2, 3, 2), 'half'), (SHAPES[1], 1, 'dirty'), (SHAPES[1], 4, 'full'),
                                (SHAPES[0], 1, 'one'), (SHAPES[1], 20, 'empty'), (SHAPES[0], 4, 'empty')):
        _, _, _, v, lm, f = lattice_inputs(shape, shrink, kind)
        r, lo, hi, h = R.hist(v, f, lm, bins)
        gr, glohi, gh = ops.n4_hist(up(v), up(f), up(lm), bins)
        assert gh.dtype == torch.int64 and tuple(gh.shape) == (bins,) and tuple(glohi.shape) == (2,)
        assert host(gr).tobytes() == r.tobytes(), (shape, shrink, kind)
        assert host(glohi).tobytes() == np.array([lo, hi]).tobytes()
        assert np.array_equal(host(gh), h) and int(gh.sum()) == int(lm.sum()) * R.Q24
    # values exactly on bin centres and on hi: lo = 0, sl = 1 / 8, so c is a whole number for every point
    n = (5, 9, 47)
    v = (np.arange(int(np.prod(n))) % bins).reshape(n) / 8.0
    lm = np.ones(n, dtype=np.uint8)
    r, lo, hi, h = R.hist(v, np.zeros(n), lm, bins)
    assert (lo, hi) == (0.0, (bins - 1) / 8.0) and (h % R.Q24 == 0).all()
    assert np.array_equal(h // R.Q24, np.bincount(np.arange(v.size) % bins, minlength=bins))
    gr, glohi, gh = ops.n4_hist(up(v), up(np.zeros(n)), up(lm), bins)
    assert np.array_equal(host(gh), h) and host(glohi).tolist() == [lo, hi] and host(gr).tobytes() == r.tobytes()
    flat = ops.n4_hist(up(np.full(n, 1.5)), up(np.zeros(n)), up(lm), bins)        # hi == lo: everything in bin 0
    assert host(flat[1]).tolist() == [1.5, 1.5] and int(flat[2][0]) == v.size * R.Q24 and int(flat[2].sum()) == v.size * R.Q24


# ---- bts_n4_residual ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bins', [2, 200, 1024])
def test_residual(bins):
    import bts_amd  # noqa: F401
    from bts_amd import n4, ops
    for shape, shrink, kind in ((SHAPES[0], 1, 'full'), (SHAPES[1], (2, 3, 2), 'half'), (SHAPES[1], 1, 'dirty'), (SHAPES[0], 4, 'one')):
        _, _, _, v, lm, f = lattice_inputs(shape, shrink, kind)
        r, lo, hi, h = R.hist(v, f, lm, bins)
        if hi > lo:
            table, sl = n4.sharpen_table(h, lo, hi), (hi - lo) / (bins - 1)
        else:                                                                # one masked point, or none (the mask's voxel is off this lattice)
            lo = lo if lm.any() else 0.0
            table, sl = np.linspace(lo, lo + 1.0, bins), 0.0
        want = R.residual(r, lm, table, lo, sl)
        got = host(ops.n4_residual(up(r), up(lm), up(table), lo, sl))
        assert (np.abs(got - want) <= 4 * EPS * np.abs(table).max() + np.spacing(np.abs(r))).all(), (shape, shrink, kind)
        assert (got[lm == 0] == 0).all()


# ---- bts_n4_fit --------------------------------------------------------------------------------------------------------------------
def check_fit(got, ref):
    num, den, dphi, n, absn = ref
    gnum, gden, gdphi = (host(t) for t in got)
    bound = 4 * np.maximum(n, 8) * EPS
    assert (np.abs(gnum - num) <= bound * absn).all() and (np.abs(gden - den) <= bound * den).all()
    empty = den == 0
    assert np.array_equal(gden == 0, empty) and (gdphi[empty] == 0).all() and (gnum[empty] == 0).all()
    safe = np.where(empty, 1.0, den)
    quotient = 1.01 * bound * (absn + np.abs(dphi) * den) / safe + 2 * EPS * np.abs(dphi)      # the two bounds carried through num / den
    assert (np.abs(gdphi - dphi)[~empty] <= quotient[~empty]).all()
    return int(empty.sum())


@pytest.mark.parametrize('mesh', MESHES)
def test_fit(mesh):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    unsupported = {}
    for shape, shrink, kind in ((SHAPES[0], 1, 'full'), (SHAPES[0], (2, 3, 2), 'half'), (SHAPES[0], 4, 'full'), (SHAPES[1], 4, 'dirty'),
                                (SHAPES[1], 1, 'one'), (SHAPES[1], 20, 'full'), (SHAPES[0], (2, 3, 2), 'empty')):
        _, _, stride, v, lm, f = lattice_inputs(shape, shrink, kind)
        res = np.where(lm != 0, 0.2 * np.random.default_rng(9).standard_normal(v.shape) + 0.05, 0.0)
        ref = R.fit(res, lm, shape, stride, mesh)
        got = ops.n4_fit(up(res), up(lm), shape, stride, mesh)
        assert all(tuple(t.shape) == tuple(m + 3 for m in mesh) and t.dtype == torch.float64 for t in got)
        unsupported[(shape, shrink, kind)] = check_fit(got, ref)
        phi0 = np.random.default_rng(3).standard_normal(ref[0].shape)
        phi = up(phi0)
        again = ops.n4_fit(up(res), up(lm), shape, stride, mesh, phi=phi)
        assert all(torch.equal(a, b) for a, b in zip(got, again))
        assert np.array_equal(host(phi), phi0 + host(got[2]))                         # phi grows by dphi, one rounded addition
    # control points with no masked lattice point in reach: all but the 4^3 around the only lattice point of the stride that passes the
    # extents (on the full 5x6x9 lattice of stride 4 every control point of the 7x11x5 lattice is reached: the cells hit along the
    # 8-element axis are 0, 2, 3, 5, 6, 7), and none at stride 1
    total = int(np.prod([m + 3 for m in mesh]))
    assert total - 64 <= unsupported[(SHAPES[1], 20, 'full')] < total and unsupported[(SHAPES[1], 1, 'one')] >= total - 64
    assert unsupported[(SHAPES[0], 1, 'full')] == 0 and unsupported[(SHAPES[0], 4, 'full')] == 0
    if mesh == (4, 8, 2):
        assert unsupported[(SHAPES[1], 20, 'full')] > 0
    assert unsupported[(SHAPES[0], (2, 3, 2), 'empty')] == int(np.prod([m + 3 for m in mesh]))


# ---- bts_n4_eval -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mesh', MESHES)
def test_eval(mesh):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    for shape, shrink, kind in ((SHAPES[0], 1, 'full'), (SHAPES[0], (2, 3, 2), 'half'), (SHAPES[1], 4, 'dirty'), (SHAPES[1], 1, 'one'),
                                (SHAPES[1], 20, 'full'), (SHAPES[0], 4, 'empty')):
        _, _, stride, v, lm, f = lattice_inputs(shape, shrink, kind)
        phi = 0.3 * np.random.default_rng(11).standard_normal(tuple(m + 3 for m in mesh))
        want, scale = R.spline(phi, shape, stride, mesh)
        gf, parts = ops.n4_eval(up(phi), up(lm), up(f), shape, stride, mesh)
        assert tuple(gf.shape) == v.shape and tuple(parts.shape) == ((v.size + 1023) // 1024, 2)
        assert (np.abs(host(gf) - want) <= 4 * 64 * EPS * scale).all(), (shape, shrink, kind)
        e = np.exp((want - f)[lm != 0])
        n = max(int(lm.sum()), 8)
        tot = host(parts).sum(axis=0)
        # against the reference spline: the bound is the summation bound alone.  The device's own f_new may differ from `want` by up to
        # 256 * 2^-53 * sum|phi w| (above), and e with it; with |phi| of order 0.3 that is a few 2^-53 of e, inside the factor 4 * max(n, 8)
        assert abs(tot[0] - e.sum()) <= 4 * n * EPS * e.sum() and abs(tot[1] - (e * e).sum()) <= 4 * n * EPS * (e * e).sum()
        # ... and against exp of the f_new the device wrote, where only the summation order and one ulp of exp remain
        eg = np.exp((host(gf) - f)[lm != 0])
        assert abs(tot[0] - eg.sum()) <= 4 * n * EPS * eg.sum() and abs(tot[1] - (eg * eg).sum()) <= 4 * n * EPS * (eg * eg).sum()
        if not lm.any():
            assert not host(parts).any()


# ---- bts_n4_apply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mesh', MESHES + [(32, 64, 16)])
def test_apply(mesh):
    import bts_amd  # noqa: F401
    from bts_amd import ops
    phi = 0.3 * np.random.default_rng(13).standard_normal(tuple(m + 3 for m in mesh))
    for shape, kind in ((SHAPES[0], 'full'), (SHAPES[1], 'dirty'), ((3, 5, 300), 'full'), ((2, 40, 1100), 'full'), ((1, 1, 1), 'full')):
        x, _ = volume(shape, kind)
        want, field, _ = R.apply(x, phi, mesh)
        out, fld = ops.n4_apply(up(x), up(phi), mesh, field=True)
        only = ops.n4_apply(up(x), up(phi), mesh)
        assert out.dtype == torch.float32 and tuple(out.shape) == shape and torch.equal(out.view(torch.int32), only.view(torch.int32))
        got, gfield = host(out), host(fld)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
        assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= ulp32(want[fin])).all(), (shape, kind)
        assert (np.abs(gfield.astype(np.float64) - field) <= ulp32(field)).all()
        if kind == 'dirty':
            assert np.isnan(want).sum() == 1 and np.isinf(want).sum() == 1 and (want < 0).any() and (want == 0).any()


# ---- across the passes -------------------------------------------------------------------------------------------------------------
def all_passes(ops, n4, x, mask, stride, mesh, bins, alloc=None):
    """every pass once, each fed with the one before -> the list of every output"""
    shape = tuple(x.shape)
    put = (lambda a: up(a)) if alloc is None else alloc
    gx = put(x)
    v, lm = ops.n4_log_lattice(gx, None if mask is None else put(mask.astype(np.uint8)), stride)
    f = put(0.05 * np.random.default_rng(1).standard_normal(tuple(v.shape)))
    r, lohi, h = ops.n4_hist(v, f, lm, bins)
    lo, hi = host(lohi).tolist()
    table = n4.sharpen_table(host(h), lo, hi)
    res = ops.n4_residual(r, lm, put(table), lo, (hi - lo) / (bins - 1))
    phi = put(np.zeros(tuple(m + 3 for m in mesh)))
    num, den, dphi = ops.n4_fit(res, lm, shape, stride, mesh, phi=phi)
    f_new, parts = ops.n4_eval(phi, lm, f, shape, stride, mesh)
    out, fld = ops.n4_apply(gx, phi, mesh, field=True)
    return [v, lm, r, lohi, h, res, num, den, dphi, phi, f_new, parts, out, fld]


def test_every_pass_twice_gives_the_same_bits():
    import bts_amd  # noqa: F401
    from bts_amd import n4, ops
    for shape, shrink, kind, mesh in ((SHAPES[0], 1, 'half', (2, 2, 2)), (SHAPES[1], (2, 3, 2), 'dirty', (4, 8, 2))):
        x, mask = volume(shape, kind)
        a = all_passes(ops, n4, x, mask, stride_of(shape, shrink), mesh, 200)
        b = all_passes(ops, n4, x, mask, stride_of(shape, shrink), mesh, 200)
        assert all(host(s).tobytes() == host(t).tobytes() for s, t in zip(a, b))


def test_guard_bands_and_poison(monkeypatch):
    """every input and output carved out of larger pattern-filled allocations (tests/guard_alloc.py): the bands stay intact, and a run on
    0x00-filled memory equals one on 0xFF-filled memory bit for bit, so no pass reads a byte nobody wrote"""
    import bts_amd  # noqa: F401
    from bts_amd import n4, ops
    for shape, shrink, kind, mesh in ((SHAPES[0], 4, 'half', (4, 8, 2)), (SHAPES[1], 1, 'dirty', (1, 1, 1))):
        x, mask = volume(shape, kind)
        results = []
        for fill in (0x00, POISON):
            with monkeypatch.context() as mp:
                g = install(mp, fill)

                def alloc(a):
                    a = np.ascontiguousarray(a)
                    t = g._alloc(a.shape, torch.from_numpy(a).dtype, dev())
                    t.copy_(up(a))
                    return t
                out = all_passes(ops, n4, x, mask, stride_of(shape, shrink), mesh, 200, alloc)
                assert g.check() >= len(out)
                results.append([host(t).copy() for t in out])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(*results))
        want = R.apply(x, results[0][9], mesh)[0]
        fin = np.isfinite(want)
        assert (np.abs(results[0][12][fin].astype(np.float64) - want[fin]) <= ulp32(want[fin])).all()


def test_refusals():
    import bts_amd  # noqa: F401
    from bts_amd import ops
    L, p, s = ops.lib(), ops._p, ops._stream()
    shape, stride, mesh = (6, 7, 8), (2, 2, 2), (1, 2, 1)
    n = ops.n4_lattice(shape, stride)
    assert n == (3, 3, 4) and L._bts_n4_eval_parts(1) == 1 and L._bts_n4_eval_parts(1025) == 2 and L._bts_n4_eval_parts(0) < 0
    x = torch.ones(shape, device=dev())
    v, lm = ops.n4_log_lattice(x, None, stride)
    f = torch.zeros_like(v)
    r, lohi, h = ops.n4_hist(v, f, lm, 8)
    table = torch.zeros(8, dtype=torch.float64, device=dev())
    phi = torch.zeros((4, 5, 4), dtype=torch.float64, device=dev())
    good = [lambda: ops.n4_log_lattice(x, None, stride), lambda: ops.n4_hist(v, f, lm, 8), lambda: ops.n4_residual(r, lm, table, 0.0, 0.0),
            lambda: ops.n4_fit(r, lm, shape, stride, mesh), lambda: ops.n4_eval(phi, lm, f, shape, stride, mesh), lambda: ops.n4_apply(x, phi, mesh)]
    for call in good:
        call()
    bad = [lambda: ops.n4_log_lattice(x, None, (0, 2, 2)), lambda: ops.n4_log_lattice(x, None, (7, 2, 2)), lambda: ops.n4_log_lattice(x.double(), None, stride),
           lambda: ops.n4_log_lattice(x[:, :, ::2], None, stride), lambda: ops.n4_log_lattice(x.cpu(), None, stride), lambda: ops.n4_log_lattice(x[0], None, stride),
           lambda: ops.n4_log_lattice(x, torch.ones((6, 7, 9), dtype=torch.uint8, device=dev()), stride), lambda: ops.n4_log_lattice(x, x, stride),
           lambda: ops.n4_hist(v, f, lm, 1), lambda: ops.n4_hist(v, f, lm, 1025), lambda: ops.n4_hist(v, f, lm, 8.0), lambda: ops.n4_hist(v.float(), f, lm, 8),
           lambda: ops.n4_hist(v, f[:2], lm, 8), lambda: ops.n4_hist(v, f, lm.float(), 8),
           lambda: ops.n4_residual(r, lm, table[:1], 0.0, 1.0), lambda: ops.n4_residual(r, lm, table, float('nan'), 1.0), lambda: ops.n4_residual(r, lm, table, 0.0, -1.0),
           lambda: ops.n4_residual(r, lm, table.float(), 0.0, 1.0),
           lambda: ops.n4_fit(r, lm, shape, stride, (0, 1, 1)), lambda: ops.n4_fit(r, lm, shape, stride, (65, 1, 1)), lambda: ops.n4_fit(r, lm, shape, (1, 1, 1), mesh),
           lambda: ops.n4_fit(r, lm, shape, stride, mesh, phi=phi[:3]), lambda: ops.n4_fit(r, lm, (6, 7), stride, mesh),
           lambda: ops.n4_eval(phi[:3], lm, f, shape, stride, mesh), lambda: ops.n4_eval(phi, lm, f, shape, stride, (1, 1, 1)), lambda: ops.n4_eval(phi, lm, f, (6, 7, 11), stride, mesh),
           lambda: ops.n4_apply(x, phi, (1, 1, 1)), lambda: ops.n4_apply(x, phi.float(), mesh), lambda: ops.n4_apply(x[0], phi, mesh)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert k >= 0
    # the library's own checks, through the raw binding: BTS_ERR_SHAPE (-1), nothing launched
    u8 = torch.zeros(shape, dtype=torch.uint8, device=dev())
    d3 = (6, 7, 8)
    assert L._bts_n4_log_lattice(p(x), None, *d3, 2, 2, 2, p(v), p(lm), s) == 0
    for args in ((None, None) + d3 + (2, 2, 2, p(v), p(lm)), (p(x), None) + d3 + (2, 2, 2, None, p(lm)), (p(x), None) + d3 + (2, 2, 2, p(v), None),
                 (p(x), None, 0, 7, 8, 2, 2, 2, p(v), p(lm)), (p(x), None) + d3 + (0, 2, 2, p(v), p(lm)), (p(x), None) + d3 + (2, 8, 2, p(v), p(lm)),
                 (p(x), p(u8), 2048, 2048, 512, 2, 2, 2, p(v), p(lm))):
        assert L._bts_n4_log_lattice(*(args + (s,))) == -1, args[2:8]
    npts = v.numel()
    r4 = torch.zeros(4, dtype=torch.float64, device=dev())
    assert L._bts_n4_range_hist(p(v), p(f), p(lm), npts, 8, p(r), p(r4), p(h), s) == 0
    for args in ((p(v), p(f), p(lm), 0, 8, p(r), p(r4), p(h)), (p(v), p(f), p(lm), 2 ** 31, 8, p(r), p(r4), p(h)), (p(v), p(f), p(lm), npts, 1, p(r), p(r4), p(h)),
                 (p(v), p(f), p(lm), npts, 1025, p(r), p(r4), p(h)), (None, p(f), p(lm), npts, 8, p(r), p(r4), p(h)), (p(v), None, p(lm), npts, 8, p(r), p(r4), p(h)),
                 (p(v), p(f), None, npts, 8, p(r), p(r4), p(h)), (p(v), p(f), p(lm), npts, 8, None, p(r4), p(h)), (p(v), p(f), p(lm), npts, 8, p(r), None, p(h)),
                 (p(v), p(f), p(lm), npts, 8, p(r), p(r4), None)):
        assert L._bts_n4_range_hist(*(args + (s,))) == -1, args[3:5]
    assert L._bts_n4_residual(p(r), p(lm), p(table), npts, 8, 0.0, 0.5, p(f), s) == 0
    for args in ((p(r), p(lm), p(table), 0, 8, 0.0, 0.5, p(f)), (p(r), p(lm), p(table), npts, 1, 0.0, 0.5, p(f)), (p(r), p(lm), p(table), npts, 1025, 0.0, 0.5, p(f)),
                 (p(r), p(lm), p(table), npts, 8, float('inf'), 0.5, p(f)), (p(r), p(lm), p(table), npts, 8, 0.0, float('nan'), p(f)),
                 (p(r), p(lm), p(table), npts, 8, 0.0, -0.5, p(f)), (None, p(lm), p(table), npts, 8, 0.0, 0.5, p(f)), (p(r), None, p(table), npts, 8, 0.0, 0.5, p(f)),
                 (p(r), p(lm), None, npts, 8, 0.0, 0.5, p(f)), (p(r), p(lm), p(table), npts, 8, 0.0, 0.5, None)):
        assert L._bts_n4_residual(*(args + (s,))) == -1, args[3:7]
    num, den, dphi = (torch.zeros_like(phi) for _ in range(3))
    geo = d3 + (2, 2, 2) + mesh
    assert L._bts_n4_fit(p(r), p(lm), *geo, p(num), p(den), p(dphi), None, s) == 0
    for g in (d3 + (2, 2, 2, 0, 2, 1), d3 + (2, 2, 2, 1, 65, 1), d3 + (2, 0, 2) + mesh, d3 + (2, 2, 9) + mesh, (6, 0, 8, 2, 2, 2) + mesh,
              (600, 7, 8, 1, 2, 2) + mesh):                                              # the last: 600 lattice points on an axis
        assert L._bts_n4_fit(p(r), p(lm), *g, p(num), p(den), p(dphi), None, s) == -1, g
    for ptrs in ((None, p(lm), p(num), p(den), p(dphi)), (p(r), None, p(num), p(den), p(dphi)), (p(r), p(lm), None, p(den), p(dphi)),
                 (p(r), p(lm), p(num), None, p(dphi)), (p(r), p(lm), p(num), p(den), None)):
        assert L._bts_n4_fit(ptrs[0], ptrs[1], *geo, ptrs[2], ptrs[3], ptrs[4], None, s) == -1
    parts = torch.zeros((1, 2), dtype=torch.float64, device=dev())
    assert L._bts_n4_eval(p(phi), *geo, p(f), p(lm), p(r), p(parts), s) == 0
    for g in (d3 + (2, 2, 2, 0, 2, 1), d3 + (2, 2, 2, 1, 2, 65), d3 + (7, 2, 2) + mesh, (6, 7, -1, 2, 2, 2) + mesh):
        assert L._bts_n4_eval(p(phi), *g, p(f), p(lm), p(r), p(parts), s) == -1, g
    for ptrs in ((None, p(f), p(lm), p(r), p(parts)), (p(phi), None, p(lm), p(r), p(parts)), (p(phi), p(f), None, p(r), p(parts)),
                 (p(phi), p(f), p(lm), None, p(parts)), (p(phi), p(f), p(lm), p(r), None)):
        assert L._bts_n4_eval(ptrs[0], *geo, ptrs[1], ptrs[2], ptrs[3], ptrs[4], s) == -1
    out = torch.zeros_like(x)
    assert L._bts_n4_apply(p(x), *d3, p(phi), *mesh, p(out), None, s) == 0
    for args in ((None,) + d3 + (p(phi),) + mesh + (p(out),), (p(x),) + d3 + (None,) + mesh + (p(out),), (p(x),) + d3 + (p(phi),) + mesh + (None,),
                 (p(x), 6, 7, 0, p(phi)) + mesh + (p(out),), (p(x),) + d3 + (p(phi), 1, 0, 1, p(out)), (p(x),) + d3 + (p(phi), 1, 2, 65, p(out)),
                 (p(x), 2048, 2048, 512, p(phi)) + mesh + (p(out),)):
        assert L._bts_n4_apply(*(args + (None, s))) == -1, args[1:4]
    torch.cuda.synchronize()


# ---- n4.correct on the device ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def head():
    x, tissue, logb = R.phantom((40, 48, 36))
    clean, _, _ = R.phantom((40, 48, 36), bias=False)
    return x, tissue, logb, R.tissue_cv(clean, tissue)


def test_correct_recovers_the_field(head):
    """the two recovery conditions of tests/test_n4_host.py on the 40x48x36 phantom, shrink 1, 3 levels of 20 sweeps, run on the device;
    twice, the same bits.  (The numpy evaluator gives CV 0.02312 / 0.02221 / 0.02163 after and a field error of 0.1012.)"""
    import bts_amd  # noqa: F401
    from bts_amd import n4
    x, tissue, logb, floor = head
    spec = n4.N4Spec(shrink=1, levels=3, iters=20)
    r = n4.correct(up(x), None, spec)
    after = R.tissue_cv(host(r.out), tissue)
    logf = np.log(host(n4.bias_field(r, x.shape, like=r.out)).astype(np.float64))
    err = R.field_error(logf, logb, tissue > 0)
    print('device: sweeps %s, CV after %s (floor %s), field error %.4f' % (r.sweeps, ['%.5f' % v for v in after], ['%.5f' % v for v in floor], err))
    assert all(a <= 1.5 * f for a, f in zip(after, floor)) and err <= 0.2
    assert r.mesh == (4, 4, 4) and r.phi.shape == (7, 7, 7) and len(r.cv) == sum(r.sweeps) and r.points == int((x > 0).sum())
    again = n4.correct(up(x), None, spec)
    assert torch.equal(r.out.view(torch.int32), again.out.view(torch.int32)) and r.phi.tobytes() == again.phi.tobytes()
    assert r.sweeps == again.sweeps and r.cv == again.cv and torch.equal(r.f, again.f)
    masked = n4.correct(up(x), up(tissue > 100), spec._replace(levels=1, iters=2))      # an explicit mask: fewer points, still every voxel written
    assert masked.points == int((tissue > 100).sum()) and bool((masked.out[up(tissue == 100)] > 0).all())


def test_correct_is_closer_to_the_reference_than_float32_input_is(head):
    """levels=2, iters=3, threshold=0: both sides take the same six sweeps.  The numpy evaluator as it is, and with its log image rounded
    to float32 (a perturbation of some 2^29 fp64 ulps): the device's final lattice-point field must lie closer to the unperturbed
    reference, in max-abs terms, than the perturbed reference does.  Measured on an MI355X: device 2.8e-17, float32 input 7.1e-09."""
    import bts_amd  # noqa: F401
    from bts_amd import n4
    x = head[0]
    spec = n4.N4Spec(shrink=1, levels=2, iters=3, threshold=0.0)
    ref = n4.correct(x, None, spec, evaluate=R.NumpyEvaluator())
    rounded = n4.correct(x, None, spec, evaluate=R.NumpyEvaluator(round_v=True))
    got = n4.correct(up(x), None, spec)
    assert ref.sweeps == rounded.sweeps == got.sweeps == (3, 3)
    d_dev, d_f32 = float(np.abs(host(got.f) - ref.f).max()), float(np.abs(rounded.f - ref.f).max())
    print('max |f - f_ref| over the lattice: device %.3e, reference with float32 log image %.3e' % (d_dev, d_f32))
    assert d_f32 > 0 and d_dev < d_f32


# ---- the command lines -------------------------------------------------------------------------------------------------------------
KW = dict(base_filters=4, groups=2, reduction=2, depth=2)


def test_commands_end_to_end(tmp_path, capsys):
    """two tiny NIfTI cases -> `preprocess --bias_correct` records the spec and writes other examples than a run without the flag;
    `python -m bts_amd.test` then corrects every case by that record without any flag, by the overridden spec with --bias_correct
    --bias_iters, and prints what it always has without either"""
    import bts_amd  # noqa: F401
    from bts_amd import n4, nifti, preprocess
    from bts_amd import test as T
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    from oracle import torch_ref as O
    from segment_ref import padded, randomised_params
    vol = (20, 24, 18)
    src = tmp_path / 'in'
    for k in range(2):
        os.makedirs(str(src / ('case%d' % k)))
        x, tissue, _ = R.phantom(vol, seed=k)
        nifti.save(str(src / ('case%d' % k) / 'c_t1ce.nii.gz'), x, np.eye(4))
        nifti.save(str(src / ('case%d' % k) / 'c_flair.nii'), (x[::-1] * np.float32(0.5)).copy(), np.eye(4))
        nifti.save(str(src / ('case%d' % k) / 'c_seg.nii.gz'), (tissue == 220).astype(np.int16), np.eye(4))
    base = ['--in_locs', str(src), '--modalities', 't1ce,flair', '--truth', 'seg']
    flags = ['--bias_correct', '--bias_shrink', '2', '--bias_levels', '2', '--bias_iters', '4']
    assert preprocess.main(base + ['--out_loc', str(tmp_path / 'plain')]) == 0
    assert preprocess.main(base + ['--out_loc', str(tmp_path / 'bias')] + flags) == 0
    capsys.readouterr()
    spec = n4.N4Spec(shrink=2, levels=2, iters=4)
    rec = np.load(str(tmp_path / 'bias' / 'prepro.npy'), allow_pickle=True).item()
    old = np.load(str(tmp_path / 'plain' / 'prepro.npy'), allow_pickle=True).item()
    assert rec['bias'] == n4.spec_record(spec) and 'bias' not in old and rec['size'] == old['size']
    assert preprocess.load_bias(str(tmp_path / 'bias' / 'prepro.npy')) == spec and preprocess.load_bias(str(tmp_path / 'plain' / 'prepro.npy')) is None
    np.save(str(tmp_path / 'today.npy'), {'size': old['size'], 'norm': {'mean': old['norm']['mean'], 'std': old['norm']['std']}})
    assert (tmp_path / 'today.npy').read_bytes() == (tmp_path / 'plain' / 'prepro.npy').read_bytes()
    a, b = np.load(str(tmp_path / 'plain' / 'train' / '1.npz')), np.load(str(tmp_path / 'bias' / 'train' / '1.npz'))
    assert a['x'].shape == b['x'].shape and not np.array_equal(a['x'], b['x']) and np.array_equal(a['y'], b['y'])
    # the stored example is the corrected scan: the same crop, statistics and normalisation applied to n4.correct's output
    xs, _, _ = preprocess.create_dataset([str(src)], ['t1ce', 'flair'], 'seg', bias=spec)
    raw = np.asarray(nifti.load(str(src / 'case0' / 'c_t1ce.nii.gz'))[0]).astype(np.float32)
    direct = n4.correct(up(raw), None, spec)
    lo = [int(np.nonzero(raw.any(axis=tuple(j for j in range(3) if j != i)))[0][0]) for i in range(3)]
    sz = rec['size']
    assert np.array_equal(host(xs[0][..., 0]), host(direct.out)[lo[0]:lo[0] + sz['h'], lo[1]:lo[1] + sz['w'], lo[2]:lo[2] + sz['d']])
    # the segmentation command
    build = padded(vol, 4)
    model = Model(**KW)
    model.build((1,) + tuple(build) + (2,))
    model.set_weights_from(randomised_params(O.default_config(**KW), tuple(build), 31))
    save_checkpoint(str(tmp_path / 'tumor'), model)
    save_train_args(str(tmp_path / 'tumor'), {'model_args': dict(KW), 'crop_size': list(build)})
    common = ['--in_locs', str(src), '--modalities', 't1ce,flair', '--gpu', '--tumor_model', str(tmp_path / 'tumor'), '--workers', '0']
    capsys.readouterr()                                                # what create_dataset printed above
    assert T.main(common + ['--tumor_prepro', str(tmp_path / 'plain' / 'prepro.npy'), '--out_loc', str(tmp_path / 'o1')]) == 0
    plain_text = capsys.readouterr().out
    assert 'Bias' not in plain_text and '2 cases segmented' in plain_text
    assert T.main(common + ['--tumor_prepro', str(tmp_path / 'bias' / 'prepro.npy'), '--out_loc', str(tmp_path / 'o2')]) == 0
    text = capsys.readouterr().out
    assert 'Bias-field correction (recorded by' in text and 'iters 4' in text
    flair = np.asarray(nifti.load(str(src / 'case0' / 'c_flair.nii'))[0]).astype(np.float32)
    lines = ['case0. Bias-corrected ' + '; '.join([n4.format_result('t1ce', direct), n4.format_result('flair', n4.correct(up(flair), None, spec))])]
    assert lines[0] in text and text.count('Bias-corrected') == 2 and len(direct.sweeps) == 2 and 1 <= min(direct.sweeps) <= max(direct.sweeps) <= 4
    assert T.main(common + ['--tumor_prepro', str(tmp_path / 'bias' / 'prepro.npy'), '--out_loc', str(tmp_path / 'o3'), '--bias_correct',
                            '--bias_iters', '2']) == 0
    text = capsys.readouterr().out
    assert 'Bias-field correction (--bias_correct over the record of' in text and 'iters 2' in text and 'shrink 2' in text
    assert 'case0. Bias-corrected ' + n4.format_result('t1ce', n4.correct(up(raw), None, spec._replace(iters=2))) in text
    assert T.main(common + ['--tumor_prepro', str(tmp_path / 'plain' / 'prepro.npy'), '--out_loc', str(tmp_path / 'o4'), '--bias_correct']) == 0
    assert 'Bias-field correction (--bias_correct): shrink 4' in capsys.readouterr().out

    def strip(t):                                                      # the run's own folders and its timing aside, the same words
        keep = [ln for ln in t.replace(str(tmp_path / 'o5'), 'OUT').replace(str(tmp_path / 'o1'), 'OUT').splitlines() if 'cases segmented' not in ln]
        return keep
    assert T.main(common + ['--tumor_prepro', str(tmp_path / 'plain' / 'prepro.npy'), '--out_loc', str(tmp_path / 'o5')]) == 0
    assert strip(capsys.readouterr().out) == strip(plain_text)
    for case in ('case0', 'case1'):
        assert np.array_equal(nifti.load(str(tmp_path / 'o1' / case / 'mask.nii'))[0], nifti.load(str(tmp_path / 'o5' / case / 'mask.nii'))[0])


def test_command_with_conform_coregister_and_a_recorded_bias(tmp_path, capsys):
    """python -m bts_amd.test --conform --coregister where the tumour stage's prepro.npy records a bias spec, and again with --bias_correct
    over it: every modality is corrected on its own grid first, the registration runs on the corrected volumes, and both lines appear,
    the correction's before the registration's"""
    import bts_amd  # noqa: F401
    import coreg_ref as C
    from bts_amd import coreg, n4, nifti
    from bts_amd import test as T
    from bts_amd.model import Model
    from bts_amd.train import save_checkpoint, save_train_args
    from oracle import torch_ref as O
    from segment_ref import randomised_params
    fs, ms = (28, 33, 25), (24, 37, 27)
    shrink = np.diag([1.0 / 6.0] * 3 + [1.0])                             # the phantom's 6 mm world stored as 1 mm headers
    a6 = C.grid_affine(fs, (6.0,) * 3)
    truth = coreg.rigid_matrix((9.0, -6.0, 6.0, 3.0, -2.0, 4.0), (a6 @ np.array([13, 16, 12, 1.0]))[:3])
    f, a_f, m, a_m = C.phantom_pair(fs, (6.0,) * 3, ms, (6.6, 5.4, 5.8), truth)
    shade = [np.exp(0.3 * np.linspace(-1, 1, s[0]))[:, None, None] for s in (fs, ms)]       # a coil gradient along the first axis
    f, m = (f * shade[0]).astype(np.float32), (m * shade[1]).astype(np.float32)
    kw, res = dict(base_filters=8, groups=2, reduction=2, depth=3), 8
    padded = tuple(s + res - s % res for s in fs)
    model = Model(**kw)
    model.build((1,) + padded + (2,))
    model.set_weights_from(randomised_params(O.default_config(**kw), padded, seed=5))
    save_checkpoint(str(tmp_path / 'tumor'), model)
    save_train_args(str(tmp_path / 'tumor'), {'model_args': dict(kw), 'crop_size': list(padded)})
    spec = n4.N4Spec(shrink=2, levels=2, iters=3)
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2}, 'bias': n4.spec_record(spec),
                                       'norm': {'mean': np.array([0.2, 0.2]).reshape(1, 1, 1, 2), 'std': np.array([0.2, 0.2]).reshape(1, 1, 1, 2)}})
    os.makedirs(str(tmp_path / 'data' / 'one'))
    nifti.save(str(tmp_path / 'data' / 'one' / 'c_t1ce.nii.gz'), f, shrink @ a_f)
    nifti.save(str(tmp_path / 'data' / 'one' / 'c_flair.nii.gz'), m, shrink @ a_m)
    base = ['--in_locs', str(tmp_path / 'data'), '--modalities', 't1ce,flair', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy'), '--workers', '0', '--conform', 'RAS', '--coregister', '--coregister_max_mm', '4',
            '--coregister_bins', '16']
    case = T.decode_case(str(tmp_path / 'data' / 'one'), ['t1ce', 'flair'], '', True)
    for extra, used in (([], spec), (['--bias_correct', '--bias_iters', '2'], spec._replace(iters=2))):
        assert T.main(base + ['--out_loc', str(tmp_path / ('out%d' % len(extra)))] + extra) == 0
        text = capsys.readouterr().out
        vols, _ = T.upload_conform_case(case, dev())
        vols, corrected = n4.correct_case([v.contiguous() for v in vols], used)
        assert [tuple(r.out.shape) for r in corrected] == [fs, ms] and all(max(r.sweeps) <= used.iters for r in corrected)
        _, found = coreg.coregister_case(vols, case['affines'], bounds=(4.0, 20.0), bins=16)
        bias_line = 'one. Bias-corrected ' + '; '.join(n4.format_result(mod, r) for mod, r in zip(('t1ce', 'flair'), corrected))
        coreg_line = 'one. Coregistered ' + coreg.format_result('flair', found[1])
        assert bias_line in text and coreg_line in text and text.index(bias_line) < text.index(coreg_line)
        assert ('recorded by' in text) == (not extra) and ('--bias_correct over the record of' in text) == bool(extra)
        mask, hdr = nifti.load(str(tmp_path / ('out%d' % len(extra)) / 'one' / 'mask.nii'))
        assert tuple(mask.shape) == fs and np.array_equal(hdr['affine'], (shrink @ a_f).astype(np.float32))
