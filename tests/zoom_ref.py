"""numpy restatement of scipy.ndimage.zoom(order in {0,1,3}, mode='reflect') per channel, parametrised by dtype (helper module, not
collected).  This is the arithmetic csrc/resample.hip implements; tests/test_resample_host.py pins its float64 form to SciPy itself.

  output extent     int(round(n * zoom))            Python's round: ties to even
  coordinate        o * (n-1)/(nout-1)              formed in float64 as zoom() does, whatever `dtype` is; nout == 1 -> 0
  order 3           prefilter every axis (line *= 6; causal c_i += z c_{i-1} from c0 + z/(1-z^2n) sum_i z^i (c_i + z^n c_{n-1-i});
                    anti-causal from c_{n-1} *= z/(z-1), c_i = z (c_{i+1} - c_i); z = sqrt(3) - 2), then 4 taps per axis at
                    floor(c)-1 .. floor(c)+2 with B-spline weights, summed separably, W innermost
  order 1           8 taps summed as zoom() does: ((v * wd) * wh) * ww in row-major tap order
  order 0           the sample at floor(c + 0.5)
  out of range      half-sample symmetric reflection: -1 -> 0, n -> n-1
"""
import numpy as np

POLE = np.sqrt(3.0) - 2.0


def zoom_output_shape(shape, factors):
    return tuple(int(round(int(n) * float(f))) for n, f in zip(shape, factors))


def _reflect(i, n):
    i = np.where(i < 0, -i - 1, i)
    i = np.where(i >= n, 2 * n - 1 - i, i)
    return np.clip(i, 0, n - 1)


def prefilter_axis(a, axis, dtype):
    """cubic B-spline coefficients along `axis`, all lines at once"""
    a = np.moveaxis(np.array(a, dtype=dtype, copy=True), axis, 0)
    n = a.shape[0]
    z = dtype(POLE)
    a *= dtype(6.0)
    pw = (POLE ** np.arange(n)).astype(dtype)
    zn = dtype(POLE ** n)
    gain = dtype(POLE / (1.0 - POLE ** (2 * n)))
    s = np.tensordot(pw, a + zn * a[::-1], axes=(0, 0)).astype(dtype)
    a[0] = a[0] + gain * s
    for i in range(1, n):
        a[i] = a[i] + z * a[i - 1]
    a[n - 1] = a[n - 1] * dtype(POLE / (POLE - 1.0))
    for i in range(n - 2, -1, -1):
        a[i] = z * (a[i + 1] - a[i])
    return np.moveaxis(a, 0, axis)


def prefilter3d(x, dtype=np.float64):
    """x: (D,H,W) or (D,H,W,C) -> coefficients, filtered along D, H and W"""
    dtype = np.dtype(dtype).type
    for ax in range(3):
        x = prefilter_axis(x, ax, dtype)
    return np.ascontiguousarray(x)


def taps(n, nout, order, dtype):
    """-> (index (nout, nt) int64, weight (nout, nt) dtype) of one axis"""
    scale = (n - 1) / (nout - 1) if nout > 1 else 1.0
    c = np.arange(nout, dtype=np.float64) * scale
    if order == 0:
        return _reflect(np.floor(c + 0.5).astype(np.int64), n)[:, None], np.ones((nout, 1), dtype)
    fl = np.floor(c)
    i0 = fl.astype(np.int64)
    t = (c - fl).astype(dtype)
    one, two, three, four, six = (dtype(v) for v in (1, 2, 3, 4, 6))
    if order == 1:
        w0 = one - t
        return _reflect(np.stack([i0, i0 + 1], 1), n), np.stack([w0, one - w0], 1)        # zoom() forms the last weight as 1 - the others
    u = one - t
    w1 = (t * t * (t - two) * three + four) / six
    w2 = (u * u * (u - two) * three + four) / six
    w0 = u * u * u / six
    w3 = one - w0 - w1 - w2
    return _reflect(np.stack([i0 - 1, i0, i0 + 1, i0 + 2], 1), n), np.stack([w0, w1, w2, w3], 1)


def _bc(w, axis, ndim):
    sh = [1] * ndim
    sh[axis] = w.shape[0]
    return w.reshape(sh)


def interpolate(coef, out_shape, order, dtype=np.float64):
    """coef: (D,H,W) or (D,H,W,C) -> values on the zoom() grid of spatial extent out_shape"""
    dtype = np.dtype(dtype).type
    a = np.asarray(coef, dtype=dtype)
    nd = a.ndim
    tp = [taps(a.shape[ax], out_shape[ax], order, dtype) for ax in range(3)]
    if order == 0:
        return np.ascontiguousarray(a[tp[0][0][:, 0]][:, tp[1][0][:, 0]][:, :, tp[2][0][:, 0]])
    if order == 1:
        (idd, wd), (ih, wh), (iw, ww) = tp
        out = np.zeros(tuple(out_shape) + a.shape[3:], dtype)
        for i in range(2):
            ai = a[idd[:, i]]
            for j in range(2):
                aij = ai[:, ih[:, j]]
                for k in range(2):
                    v = aij[:, :, iw[:, k]]
                    out += ((v * _bc(wd[:, i], 0, nd)) * _bc(wh[:, j], 1, nd)) * _bc(ww[:, k], 2, nd)
        return out
    # order 3, separable with W innermost: out = sum_a wd[a] * (sum_b wh[b] * (sum_k ww[k] * v))
    (idd, wd), (ih, wh), (iw, ww) = tp
    aw = np.zeros(a.shape[:2] + (out_shape[2],) + a.shape[3:], dtype)
    for k in range(4):
        aw += _bc(ww[:, k], 2, nd) * a[:, :, iw[:, k]]
    ah = np.zeros(a.shape[:1] + (out_shape[1], out_shape[2]) + a.shape[3:], dtype)
    for b in range(4):
        ah += _bc(wh[:, b], 1, nd) * aw[:, ih[:, b]]
    out = np.zeros(tuple(out_shape) + a.shape[3:], dtype)
    for i in range(4):
        out += _bc(wd[:, i], 0, nd) * ah[idd[:, i]]
    return out


def zoom(x, out_shape, order=3, dtype=np.float64):
    """the whole chain on (D,H,W) or (D,H,W,C) with an explicit output extent"""
    x = np.asarray(x)
    return interpolate(prefilter3d(x, dtype) if order == 3 else x.astype(dtype), out_shape, order, dtype)


def brain_mask(y):
    """test.py:53-54 on a (D,H,W,C) volume -> (D,H,W,1) float32"""
    return (np.max(y, axis=-1, keepdims=True) > 0).astype(np.float32)
