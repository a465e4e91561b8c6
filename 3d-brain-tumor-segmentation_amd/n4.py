"""N4 bias-field correction of MRI volumes (Tustison et al. 2010, "N4ITK: improved N3 bias correction").

Receive coils leave a smooth multiplicative shading on every scan, 10-40 % across a head.  N4 estimates it as exp of a cubic B-spline:
the log image is corrected by the current field, its histogram is sharpened by a Wiener deconvolution with a Gaussian, every voxel is
moved to the expected true value of its bin, and the difference is smoothed by one level of multilevel B-spline approximation (Lee,
Wolberg and Shin 1997) and added to the spline; coarse mesh to fine, the control lattice refined exactly between levels.

What runs where: the six passes over voxels are kernels of csrc/n4.hip (`ops.n4_log_lattice`, `n4_hist`, `n4_residual`, `n4_fit`, `n4_eval`
on the shrunken lattice, `n4_apply` on the volume); the host sharpens the histogram, `bins` integers read back per sweep, decides
convergence from two sums, and refines the 4^3 .. 35^3 control lattice between levels.  `correct` is written once against an evaluator
object that provides the passes: `DeviceEvaluator` here, the numpy one in tests/n4_ref.py; the loop neither knows nor cares which.

The reference project has no such stage (preprocess.py, test.py): it expects scans that were corrected beforehand, or not at all."""
import collections
import math

import numpy as np

MAX_MESH = 64                      # mesh elements per axis the kernels take

N4Spec = collections.namedtuple('N4Spec', 'shrink levels iters threshold mesh bins fwhm noise')
N4Spec.__new__.__defaults__ = (4, 4, 50, 1e-3, (1, 1, 1), 200, 0.15, 0.01)
N4Result = collections.namedtuple('N4Result', 'out phi mesh sweeps cv f points')


def check_spec(spec):
    """-> the spec with plain Python numbers; ValueError naming the field that is out of range"""
    if not isinstance(spec, N4Spec):
        raise ValueError('n4: spec must be an N4Spec, got %r' % (spec,))

    def whole(v):
        return not isinstance(v, bool) and isinstance(v, (int, np.integer))

    def number(v):
        return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(float(v))
    if not whole(spec.shrink) or spec.shrink < 1:
        raise ValueError('n4: shrink must be an integer >= 1, got %r' % (spec.shrink,))
    if not whole(spec.levels) or not 1 <= spec.levels <= 6:
        raise ValueError('n4: levels must be an integer in 1..6, got %r' % (spec.levels,))
    if not whole(spec.iters) or spec.iters < 1:
        raise ValueError('n4: iters must be an integer >= 1, got %r' % (spec.iters,))
    if not number(spec.threshold) or spec.threshold < 0:
        raise ValueError('n4: threshold must be a number >= 0, got %r' % (spec.threshold,))
    try:
        mesh = tuple(spec.mesh)
    except TypeError:
        mesh = ()
    if len(mesh) != 3 or not all(whole(m) and m >= 1 for m in mesh):
        raise ValueError('n4: mesh must be three integers >= 1, got %r' % (spec.mesh,))
    if max(mesh) * 2 ** (int(spec.levels) - 1) > MAX_MESH:
        raise ValueError('n4: mesh %r doubled over %d levels passes %d elements per axis' % (spec.mesh, spec.levels, MAX_MESH))
    if not whole(spec.bins) or not 2 <= spec.bins <= 1024:
        raise ValueError('n4: bins must be an integer in 2..1024, got %r' % (spec.bins,))
    if not number(spec.fwhm) or not spec.fwhm > 0:
        raise ValueError('n4: fwhm must be a number > 0, got %r' % (spec.fwhm,))
    if not number(spec.noise) or not spec.noise > 0:
        raise ValueError('n4: noise must be a number > 0, got %r' % (spec.noise,))
    return N4Spec(int(spec.shrink), int(spec.levels), int(spec.iters), float(spec.threshold), tuple(int(m) for m in mesh), int(spec.bins),
                  float(spec.fwhm), float(spec.noise))


def spec_record(spec):
    """the spec as the plain dict prepro.npy's `bias` entry holds; `spec_from_record` is its inverse"""
    d = dict(check_spec(spec)._asdict())
    d['mesh'] = list(d['mesh'])
    return d


def spec_from_record(d):
    try:
        return check_spec(N4Spec(**dict(d, mesh=tuple(d['mesh']))))
    except (TypeError, KeyError) as e:
        raise ValueError('n4: not a recorded spec: %r (%s)' % (d, e))


def lattice_geometry(shape, shrink):
    """-> (origin, stride, counts) of the working lattice: per axis stride min(extent, shrink), origin stride // 2, and as many points
    as fit (the form of coreg.lattice)"""
    shape = tuple(int(n) for n in shape)
    if len(shape) != 3 or min(shape) < 1 or int(shrink) < 1:
        raise ValueError('n4: a (D,H,W) shape and shrink >= 1, got %r and %r' % (shape, shrink))
    stride = tuple(min(n, int(shrink)) for n in shape)
    origin = tuple(s // 2 for s in stride)
    counts = tuple((n - 1 - o) // s + 1 for n, o, s in zip(shape, origin, stride))
    return origin, stride, counts


def bspline_weights(p, extent, mesh):
    """full-resolution indices p along an axis of `extent` voxels and `mesh` elements -> (cell i, weights (len(p), 4)) of the control
    points i .. i+3: u = (p + 0.5) / extent * mesh, i = min(floor(u), mesh - 1), t = u - i, uniform cubic B-spline weights of t.
    float64, the operations in the order of csrc/n4.hip's n4_basis, so the two agree bit for bit"""
    p = np.asarray(p, dtype=np.float64)
    u = (p + 0.5) / float(extent) * float(mesh)
    i = np.minimum(np.floor(u), float(mesh - 1))
    t = u - i
    t2 = t * t
    t3 = t2 * t
    m = 1.0 - t
    w = np.stack([((m * m) * m) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0, (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0], axis=-1)
    return i.astype(np.int64), w


def sharpen_table(hist, lo, hi, spec=N4Spec()):
    """the sharpened intensity map of one sweep: integer histogram of the corrected log image over [lo, hi] -> E (bins float64), the
    expected true log intensity of a voxel observed at each bin centre.  The histogram, padded centrally into P = 2^(ceil(log2 bins)+1)
    entries, is deconvolved by a wrap-around Gaussian F of the spec's FWHM (in log units) with the Wiener filter conj(F^) / (|F^|^2 +
    noise), clamped at 0 to U, and E = ((xbin U) * F) / (U * F), 0 where the denominator is 0, xbin the bin centres.  float64, numpy FFT"""
    h = np.asarray(hist)
    bins = int(h.size)
    if h.ndim != 1 or bins < 2 or not hi > lo:
        raise ValueError('sharpen_table: one histogram of at least 2 bins and lo < hi, got shape %s, %r, %r' % (h.shape, lo, hi))
    sl = (float(hi) - float(lo)) / (bins - 1)
    big = 1 << (int(math.ceil(math.log2(bins))) + 1)
    off = (big - bins) // 2
    v = np.zeros(big, dtype=np.float64)
    v[off:off + bins] = h.astype(np.float64)
    sigma = float(spec.fwhm) / (2.0 * math.sqrt(2.0 * math.log(2.0))) / sl
    k = np.arange(big, dtype=np.float64)
    d = np.minimum(k, big - k)
    f = np.exp(-0.5 * (d / sigma) ** 2)
    f = f / f.sum()
    fh = np.fft.fft(f)
    g = np.conj(fh) / (np.abs(fh) ** 2 + float(spec.noise))
    u = np.maximum(np.real(np.fft.ifft(np.fft.fft(v) * g)), 0.0)
    xbin = float(lo) + (k - off) * sl
    num = np.real(np.fft.ifft(np.fft.fft(xbin * u) * fh))
    den = np.real(np.fft.ifft(np.fft.fft(u) * fh))
    e = np.zeros(big, dtype=np.float64)
    np.divide(num, den, out=e, where=den != 0.0)
    return np.ascontiguousarray(e[off:off + bins])


def refine_lattice(phi):
    """the control lattice of a mesh of (m0, m1, m2) elements, shape m + 3 -> that of the mesh of 2 m elements, shape 2 m + 3, of the SAME
    spline, by dyadic knot insertion per axis: new[2k] = (phi[k] + phi[k+1]) / 2, new[2k+1] = (phi[k] + 6 phi[k+1] + phi[k+2]) / 8"""
    a = np.asarray(phi, dtype=np.float64)
    if a.ndim != 3 or min(a.shape) < 4:
        raise ValueError('refine_lattice: a control lattice of at least 4 points per axis, got shape %s' % (a.shape,))
    for axis in range(3):
        a = np.moveaxis(a, axis, 0)
        m = a.shape[0] - 3
        out = np.empty((2 * m + 3,) + a.shape[1:], dtype=np.float64)
        out[0::2] = (a[:m + 2] + a[1:m + 3]) / 2.0
        out[1::2] = ((a[:m + 1] + 6.0 * a[1:m + 2]) + a[2:m + 3]) / 8.0
        a = np.moveaxis(out, 0, axis)
    return np.ascontiguousarray(a)


class DeviceEvaluator(object):
    """the six passes on the GPU (csrc/n4.hip through bts_amd.ops), all on the current stream.  Read back: the histogram with lo / hi, one
    copy per sweep; the partial sums of exp(f_new - f); the count of masked lattice points once; the control lattice once per level"""

    def log_lattice(self, x, mask, stride):
        import torch
        from . import ops
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError('n4: the volume must live on the GPU, or be a numpy array with a numpy evaluator')
        self.device = x.device
        return ops.n4_log_lattice(x.to(torch.float32).contiguous(), mask, stride)

    def count(self, lm):
        return int(lm.sum())

    def zeros_like(self, v):
        import torch
        return torch.zeros_like(v)

    def control(self, phi):
        import torch
        return torch.from_numpy(np.ascontiguousarray(phi, dtype=np.float64)).to(self.device)

    def host(self, a):
        return a.cpu().numpy()

    def copy(self, x):
        import torch
        return x.to(torch.float32).clone()

    def hist(self, v, f, lm, bins):
        import torch
        from . import ops
        r, lohi, hist = ops.n4_hist(v, f, lm, bins)
        both = torch.cat([lohi.view(torch.int64), hist]).cpu().numpy()     # one copy, one synchronisation per sweep
        lo, hi = (float(t) for t in both[:2].view(np.float64))
        return r, lo, hi, both[2:]

    def residual(self, r, lm, table, lo, sl):
        from . import ops
        return ops.n4_residual(r, lm, self.control(table), lo, sl)

    def fit(self, res, lm, shape, stride, mesh, phi):
        from . import ops
        ops.n4_fit(res, lm, shape, stride, mesh, phi=phi)
        return phi

    def eval(self, phi, lm, f, shape, stride, mesh):
        from . import ops
        f_new, parts = ops.n4_eval(phi, lm, f, shape, stride, mesh)
        p = parts.cpu().numpy()
        return f_new, math.fsum(p[:, 0]), math.fsum(p[:, 1])

    def apply(self, x, phi, mesh, field=False):
        import torch
        from . import ops
        return ops.n4_apply(x.to(torch.float32).contiguous(), phi, mesh, field=field)


def correct(x, mask=None, spec=N4Spec(), evaluate=None):
    """correct one (D,H,W) volume for its bias field -> N4Result.

    x: a float32 device tensor (or a numpy array, with a numpy evaluator).  mask: None (x > 0) or a (D,H,W) array of the evaluator's
    kind, non-zero = inside; in every case and-ed with x > 0 and finite.  spec: N4Spec(shrink, levels, iters, threshold, mesh, bins, fwhm,
    noise); evaluate: the object that provides the passes (DeviceEvaluator by default).
    Per level at most `iters` sweeps of: histogram of r = log x - f on the lattice -> `sharpen_table` -> residual -> one MBA fit added to
    the control lattice -> f evaluated anew; a level ends when cv = std / mean (population) of exp(f_new - f) over the masked lattice
    points falls below `threshold`, or at once where r is constant.  Between levels the mesh doubles and the lattice is refined exactly.
    -> N4Result: out = float32(x / exp(spline)) at EVERY voxel, phi (numpy float64, mesh + 3), the final mesh, the sweeps per level, the
    cv of every sweep, f (the log field at the lattice points, the evaluator's array) and points (masked lattice points).  With fewer
    than two masked lattice points: a copy of x, a zero phi on the first mesh and zero sweeps."""
    spec = check_spec(spec)
    ev = DeviceEvaluator() if evaluate is None else evaluate
    shape = tuple(int(n) for n in x.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('n4.correct: x must be a non-empty (D,H,W) volume, got shape %s' % (shape,))
    _, stride, _ = lattice_geometry(shape, spec.shrink)
    v, lm = ev.log_lattice(x, mask, stride)
    points = ev.count(lm)
    mesh = spec.mesh
    phi_h = np.zeros(tuple(m + 3 for m in mesh), dtype=np.float64)
    f = ev.zeros_like(v)
    if points < 2:
        return N4Result(ev.copy(x), phi_h, mesh, (0,) * spec.levels, (), f, points)
    phi = ev.control(phi_h)
    sweeps, trace = [], []
    for level in range(spec.levels):
        if level:
            mesh = tuple(2 * m for m in mesh)
            phi = ev.control(refine_lattice(ev.host(phi)))
        k = 0
        while k < spec.iters:
            k += 1
            r, lo, hi, hist = ev.hist(v, f, lm, spec.bins)
            if not hi > lo:
                trace.append(0.0)
                break
            table = sharpen_table(hist, lo, hi, spec)
            res = ev.residual(r, lm, table, lo, (hi - lo) / (spec.bins - 1))
            phi = ev.fit(res, lm, shape, stride, mesh, phi)
            f, se, se2 = ev.eval(phi, lm, f, shape, stride, mesh)
            mean = se / points
            cv = math.sqrt(max(se2 / points - mean * mean, 0.0)) / mean
            trace.append(cv)
            if cv < spec.threshold:
                break
        sweeps.append(k)
    return N4Result(ev.apply(x, phi, mesh), ev.host(phi), mesh, tuple(sweeps), tuple(trace), f, points)


def correct_case(vols, spec=N4Spec(), evaluate=None):
    """one correction per modality, each on its own positive voxels -> ([corrected volumes], [N4Result, ...])"""
    results = [correct(v, None, spec, evaluate) for v in vols]
    return [r.out for r in results], results


def bias_field(result, shape, evaluate=None, like=None):
    """the multiplicative field exp(spline) of a result on a (D,H,W) grid, float32, the evaluator's array.  like: any array that lives where
    the field shall (the device evaluator needs it to find the device; default: the current one)"""
    ev = DeviceEvaluator() if evaluate is None else evaluate
    shape = tuple(int(n) for n in shape)
    if isinstance(ev, DeviceEvaluator):
        import torch
        dev = like.device if like is not None else torch.device('cuda', torch.cuda.current_device())
        ev.device = dev
        ones = torch.ones(shape, dtype=torch.float32, device=dev)
    else:
        ones = np.ones(shape, dtype=np.float32)
    return ev.apply(ones, ev.control(result.phi), result.mesh, field=True)[1]


def format_result(name, r):
    """the one line the command line prints per corrected modality"""
    return '%s: sweeps %s, final cv %s, mesh %dx%dx%d, %d lattice points' % (
        name, '+'.join('%d' % k for k in r.sweeps), ('%.3e' % r.cv[-1]) if r.cv else 'none', r.mesh[0], r.mesh[1], r.mesh[2], r.points)
