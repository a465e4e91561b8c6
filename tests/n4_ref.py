"""float64 numpy restatement of N4 bias-field correction (bts_amd.n4, csrc/n4.hip), imported the way coreg_ref is.

Every pass is given twice: `*_pointwise`, one lattice point (or one bin) at a time in plain Python floats exactly as the rules read, and
vectorised; tests/test_n4_host.py proves the two equal.  Python floats and numpy float64 are the same IEEE doubles, every operation
rounded once, so the coordinate, the weights, r, the bin number and its fraction are also the bits the kernels form.  `NumpyEvaluator`
provides the passes to `n4.correct`; `phantom` is the analytic head the recovery tests use."""
import math

import numpy as np

Q24 = 1 << 24


# ---- geometry and basis ------------------------------------------------------------------------------------------------------------
def lattice(shape, stride):
    """-> (origin, counts) of the strided sub-grid: origin stride // 2, as many points as fit"""
    origin = tuple(s // 2 for s in stride)
    return origin, tuple((n - 1 - o) // s + 1 for n, o, s in zip(shape, origin, stride))


def weights_pointwise(p, extent, mesh):
    """one index -> (cell, [B0, B1, B2, B3])"""
    u = (float(p) + 0.5) / float(extent) * float(mesh)
    i = min(int(math.floor(u)), mesh - 1)
    t = u - float(i)
    t2 = t * t
    t3 = t2 * t
    m = 1.0 - t
    return i, [((m * m) * m) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0, (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0]


def weights(p, extent, mesh):
    """indices -> (cells, weights (len, 4)), vectorised, the same operations"""
    u = (np.asarray(p, dtype=np.float64) + 0.5) / float(extent) * float(mesh)
    i = np.minimum(np.floor(u), float(mesh - 1))
    t = u - i
    t2 = t * t
    t3 = t2 * t
    m = 1.0 - t
    w = np.stack([((m * m) * m) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0, (((3.0 * t2 - 3.0 * t3) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0], axis=-1)
    return i.astype(np.int64), w


def axis_matrix(extent, stride, mesh):
    """(lattice points, mesh + 3): the weight of every control point at every lattice point of one axis, and the sum of squares per point"""
    o, n = stride // 2, (extent - 1 - stride // 2) // stride + 1
    i, w = weights(o + stride * np.arange(n), extent, mesh)
    a = np.zeros((n, mesh + 3), dtype=np.float64)
    for k in range(4):
        a[np.arange(n), i + k] = w[:, k]
    q = ((w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]) + w[:, 3] * w[:, 3]
    return a, q


def matrices(shape, stride, mesh):
    return [axis_matrix(n, s, m) for n, s, m in zip(shape, stride, mesh)]


# ---- log image on the lattice ------------------------------------------------------------------------------------------------------
def log_lattice(x, mask, stride):
    """-> (v float64, lmask uint8)"""
    x = np.asarray(x, dtype=np.float32)
    o, n = lattice(x.shape, stride)
    sel = tuple(slice(oo, oo + s * (nn - 1) + 1, s) for oo, s, nn in zip(o, stride, n))
    xs = x[sel].astype(np.float64)
    ok = (xs > 0) & np.isfinite(xs)
    if mask is not None:
        ok &= np.asarray(mask)[sel] != 0
    v = np.zeros(n, dtype=np.float64)
    v[ok] = np.log(xs[ok])
    return v, ok.astype(np.uint8)


# ---- histogram ---------------------------------------------------------------------------------------------------------------------
def bin_of(r, lo, sl, bins):
    """vectorised (i, o): everything in bin 0 where sl == 0"""
    if not sl > 0.0:
        return np.zeros(r.shape, dtype=np.int64), np.zeros(r.shape, dtype=np.float64)
    c = (r - lo) / sl
    i = np.clip(np.floor(c), 0.0, float(bins - 2))
    return i.astype(np.int64), c - i


def hist(v, f, lm, bins):
    """-> (r, lo, hi, hist int64)"""
    m = lm != 0
    r = np.where(m, v - f, 0.0)
    if not m.any():
        return r, math.inf, -math.inf, np.zeros(bins, dtype=np.int64)
    rm = r[m]
    lo, hi = float(rm.min()), float(rm.max())
    sl = (hi - lo) / (bins - 1)
    i, o = bin_of(rm, lo, sl, bins)
    q = np.clip(np.rint(o * float(Q24)), 0, Q24).astype(np.int64)
    h = np.zeros(bins, dtype=np.int64)
    np.add.at(h, i, Q24 - q)
    np.add.at(h, i + 1, q)
    return r, lo, hi, h


def hist_pointwise(v, f, lm, bins):
    vs, fs, ms = v.reshape(-1), f.reshape(-1), lm.reshape(-1)
    r = [float(vs[k]) - float(fs[k]) if ms[k] else 0.0 for k in range(vs.size)]
    inside = [r[k] for k in range(vs.size) if ms[k]]
    h = [0] * bins
    if not inside:
        return np.array(r).reshape(v.shape), math.inf, -math.inf, np.array(h, dtype=np.int64)
    lo, hi = min(inside), max(inside)
    sl = (hi - lo) / (bins - 1)
    for z in inside:
        if sl > 0.0:
            c = (z - lo) / sl
            i = max(min(int(math.floor(c)), bins - 2), 0)
            o = c - float(i)
        else:
            i, o = 0, 0.0
        q = max(min(int(np.rint(o * float(Q24))), Q24), 0)
        h[i] += Q24 - q
        h[i + 1] += q
    return np.array(r).reshape(v.shape), lo, hi, np.array(h, dtype=np.int64)


# ---- sharpening, by the discrete Fourier transform written out ----------------------------------------------------------------------
def sharpen_pointwise(h, lo, hi, fwhm=0.15, noise=0.01):
    """-> (E (bins), den (bins)): the rules of the issue with every transform a plain O(P^2) sum; den is the denominator U * F at the
    kept entries (where it is small against its maximum the quotient is ill-conditioned, and no two FFTs agree there)"""
    h = np.asarray(h)
    bins = h.size
    sl = (hi - lo) / (bins - 1)
    big = 2 ** (int(math.ceil(math.log2(bins))) + 1)
    off = (big - bins) // 2
    k = np.arange(big)
    dft = np.exp(-2j * np.pi * np.outer(k, k) / big)
    idft = np.conj(dft) / big
    v = np.zeros(big)
    v[off:off + bins] = h.astype(np.float64)
    sigma = fwhm / (2.0 * math.sqrt(2.0 * math.log(2.0))) / sl
    d = np.minimum(k, big - k).astype(np.float64)
    f = np.exp(-0.5 * (d / sigma) ** 2)
    f = f / f.sum()
    fh = dft @ f
    g = np.conj(fh) / (np.abs(fh) ** 2 + noise)
    u = np.maximum(np.real(idft @ ((dft @ v) * g)), 0.0)
    xbin = lo + (k - off) * sl
    num = np.real(idft @ ((dft @ (xbin * u)) * fh))
    den = np.real(idft @ ((dft @ u) * fh))
    e = np.array([num[j] / den[j] if den[j] != 0.0 else 0.0 for j in range(big)])
    return e[off:off + bins], den[off:off + bins]


# ---- residual ----------------------------------------------------------------------------------------------------------------------
def residual(r, lm, table, lo, sl):
    i, o = bin_of(r, lo, sl, table.size)
    return np.where(lm != 0, r - (table[i] * (1.0 - o) + table[np.minimum(i + 1, table.size - 1)] * o), 0.0)


def residual_pointwise(r, lm, table, lo, sl):
    out = np.zeros(r.size)
    rs, ms, bins = r.reshape(-1), lm.reshape(-1), table.size
    for k in range(rs.size):
        if ms[k]:
            c = (float(rs[k]) - lo) / sl
            i = max(min(int(math.floor(c)), bins - 2), 0)
            o = c - float(i)
            out[k] = float(rs[k]) - (float(table[i]) * (1.0 - o) + float(table[i + 1]) * o)
    return out.reshape(r.shape)


# ---- fit ---------------------------------------------------------------------------------------------------------------------------
def fit(res, lm, shape, stride, mesh):
    """-> (num, den, dphi, n, absterm_num): n = masked lattice points in each control point's support, absterm_num = sum |w^3 z / S|
    (the terms of den are positive: its own sum)"""
    (a0, q0), (a1, q1), (a2, q2) = matrices(shape, stride, mesh)
    m = (lm != 0).astype(np.float64)
    s = (q0[:, None, None] * q1[None, :, None]) * q2[None, None, :]
    zs = m * res / s
    num = np.einsum('ai,bj,ck,abc->ijk', a0 ** 3, a1 ** 3, a2 ** 3, zs, optimize=True)
    absn = np.einsum('ai,bj,ck,abc->ijk', a0 ** 3, a1 ** 3, a2 ** 3, np.abs(zs), optimize=True)
    den = np.einsum('ai,bj,ck,abc->ijk', a0 ** 2, a1 ** 2, a2 ** 2, m, optimize=True)
    n = np.einsum('ai,bj,ck,abc->ijk', (a0 > 0) * 1.0, (a1 > 0) * 1.0, (a2 > 0) * 1.0, m, optimize=True)
    dphi = np.zeros_like(num)
    np.divide(num, den, out=dphi, where=den > 0)
    return num, den, dphi, n, absn


def fit_pointwise(res, lm, shape, stride, mesh):
    """scatter form, one lattice point at a time -> (num, den, dphi)"""
    o, n = lattice(shape, stride)
    num = np.zeros(tuple(m + 3 for m in mesh))
    den = np.zeros_like(num)
    for l0 in range(n[0]):
        i0, w0 = weights_pointwise(o[0] + l0 * stride[0], shape[0], mesh[0])
        for l1 in range(n[1]):
            i1, w1 = weights_pointwise(o[1] + l1 * stride[1], shape[1], mesh[1])
            for l2 in range(n[2]):
                if not lm[l0, l1, l2]:
                    continue
                i2, w2 = weights_pointwise(o[2] + l2 * stride[2], shape[2], mesh[2])
                s = (sum(w * w for w in w0) * sum(w * w for w in w1)) * sum(w * w for w in w2)
                z = float(res[l0, l1, l2])
                for a in range(4):
                    for b in range(4):
                        for c in range(4):
                            w = (w0[a] * w1[b]) * w2[c]
                            num[i0 + a, i1 + b, i2 + c] += ((w * w) * w) * z / s
                            den[i0 + a, i1 + b, i2 + c] += w * w
    dphi = np.zeros_like(num)
    np.divide(num, den, out=dphi, where=den > 0)
    return num, den, dphi


# ---- the spline ------------------------------------------------------------------------------------------------------------------
def spline(phi, shape, stride, mesh):
    """-> (f, absterm): the spline at every lattice point and sum |w phi| per point"""
    (a0, _), (a1, _), (a2, _) = matrices(shape, stride, mesh)
    f = np.einsum('ai,bj,ck,ijk->abc', a0, a1, a2, phi, optimize=True)
    return f, np.einsum('ai,bj,ck,ijk->abc', a0, a1, a2, np.abs(phi), optimize=True)


def spline_pointwise(phi, shape, stride, mesh):
    o, n = lattice(shape, stride)
    f = np.zeros(n)
    for l0 in range(n[0]):
        i0, w0 = weights_pointwise(o[0] + l0 * stride[0], shape[0], mesh[0])
        for l1 in range(n[1]):
            i1, w1 = weights_pointwise(o[1] + l1 * stride[1], shape[1], mesh[1])
            for l2 in range(n[2]):
                i2, w2 = weights_pointwise(o[2] + l2 * stride[2], shape[2], mesh[2])
                acc = 0.0
                for a in range(4):
                    for b in range(4):
                        for c in range(4):
                            acc += w0[a] * w1[b] * w2[c] * float(phi[i0 + a, i1 + b, i2 + c])
                f[l0, l1, l2] = acc
    return f


def evaluate(phi, lm, f_old, shape, stride, mesh):
    """-> (f_new, sum e, sum e^2) with e = exp(f_new - f_old) over the mask"""
    f_new, _ = spline(phi, shape, stride, mesh)
    e = np.exp((f_new - f_old)[lm != 0])
    return f_new, float(e.sum()), float((e * e).sum())


def apply(x, phi, mesh):
    """-> (out float32, field float32, log field float64) at every voxel"""
    x = np.asarray(x, dtype=np.float32)
    logf, _ = spline(phi, x.shape, (1, 1, 1), mesh)
    b = np.exp(logf)
    with np.errstate(all='ignore'):
        return (x.astype(np.float64) / b).astype(np.float32), b.astype(np.float32), logf


class NumpyEvaluator(object):
    """the passes of n4.correct in numpy.  round_v: round log x to float32 first, the perturbation tests/test_n4_gpu.py measures the
    device's distance from this reference against"""

    def __init__(self, round_v=False):
        self.round_v = round_v

    def log_lattice(self, x, mask, stride):
        v, lm = log_lattice(x, mask, stride)
        return (v.astype(np.float32).astype(np.float64) if self.round_v else v), lm

    def count(self, lm):
        return int(lm.sum())

    def zeros_like(self, v):
        return np.zeros_like(v)

    def control(self, phi):
        return np.array(phi, dtype=np.float64)

    def host(self, a):
        return np.array(a)

    def copy(self, x):
        return np.array(x, dtype=np.float32)

    def hist(self, v, f, lm, bins):
        return hist(v, f, lm, bins)

    def residual(self, r, lm, table, lo, sl):
        return residual(r, lm, table, lo, sl)

    def fit(self, res, lm, shape, stride, mesh, phi):
        return phi + fit(res, lm, shape, stride, mesh)[2]

    def eval(self, phi, lm, f, shape, stride, mesh):
        return evaluate(phi, lm, f, shape, stride, mesh)

    def apply(self, x, phi, mesh, field=False):
        out, b, _ = apply(x, phi, mesh)
        return (out, b) if field else out


# ---- the phantom -------------------------------------------------------------------------------------------------------------------
def phantom(shape=(40, 48, 36), bias=True, seed=0):
    """-> (x float32, tissue (0, 100, 160, 220), true log bias with zero mean over the head): three nested tissues inside an ellipsoid,
    a smooth multiplicative field, 2 % multiplicative noise; the same seed gives the same noise with and without the field"""
    g0, g1, g2 = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    rho2 = (g0 / 0.9) ** 2 + (g1 / 0.85) ** 2 + (g2 / 0.8) ** 2
    tissue = np.zeros(shape)
    tissue[rho2 < 1.0] = 100.0
    tissue[rho2 < 0.55] = 160.0
    tissue[(g0 - 0.2) ** 2 + g1 ** 2 + g2 ** 2 < 0.12] = 220.0
    head = tissue > 0
    logb = 0.35 * g0 + 0.25 * g1 ** 2 - 0.3 * g0 * g2 + 0.15 * np.sin(2.0 * g1)
    logb = logb - logb[head].mean()
    noise = 1.0 + 0.02 * np.random.default_rng(seed).standard_normal(shape)
    x = tissue * noise * (np.exp(logb) if bias else 1.0)
    x = np.where(head, np.maximum(x, 1.0), 0.0)
    return x.astype(np.float32), tissue, logb


def tissue_cv(vol, tissue):
    """std / mean of the volume over each tissue, in the order 100, 160, 220"""
    v = np.asarray(vol, dtype=np.float64)
    return [float(v[tissue == t].std() / v[tissue == t].mean()) for t in (100.0, 160.0, 220.0)]


def field_error(log_est, log_true, head):
    """RMS over the head of the difference of the two log fields, means removed, over the RMS of the true one (mean removed)"""
    a = log_est[head] - log_est[head].mean()
    b = log_true[head] - log_true[head].mean()
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))
