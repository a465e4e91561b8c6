"""N4 bias-field correction (csrc/n4.hip): the log lattice, the sharpening histogram, the B-spline fit and its evaluation."""
import numpy as np
import torch

from . import _core


N4_MAX_BINS, N4_MAX_MESH, N4_MAX_AXIS = 1024, 64, 512


def n4_lattice(shape, stride, who='n4'):
    """-> the lattice counts per axis of the strided sub-grid origin stride // 2 (bts_n4_*); 1 <= stride <= extent per axis"""
    shape, stride = _core.int3(shape, 'shape', who), _core.int3(stride, 'stride', who)
    if min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError('%s: the volume must have 1 .. 2^31 - 1 voxels, got shape %s' % (who, shape))
    if any(not 1 <= s <= n for s, n in zip(stride, shape)):
        raise ValueError('%s: stride %s must lie in 1..extent per axis of %s' % (who, stride, shape))
    return tuple((n - 1 - s // 2) // s + 1 for n, s in zip(shape, stride))


def _n4_mesh(mesh, who):
    mesh = _core.int3(mesh, 'mesh', who)
    if any(not 1 <= m <= N4_MAX_MESH for m in mesh):
        raise ValueError('%s: mesh must lie in 1..%d per axis, got %s' % (who, N4_MAX_MESH, mesh))
    return mesh


def _n4_points(t, name):
    """a lattice array: dense float64 on the GPU, three-dimensional, non-empty -> its shape"""
    if _core.dense(t, torch.float64, name, rank=3).numel() < 1:
        raise ValueError('%s must be a non-empty (n0,n1,n2) lattice array' % name)
    return tuple(t.shape)


def n4_log_lattice(x, mask=None, stride=(1, 1, 1)):
    """dense float32 (D,H,W) device volume -> (v float64, lmask uint8) on the lattice of `stride`: v = log(x) and lmask = 1 where x > 0 and
    finite and mask (uint8 or bool (D,H,W), non-zero = inside; None: everywhere) allows it, 0 and 0 elsewhere (bts_n4_log_lattice)"""
    who = 'n4_log_lattice'
    _core.dense(x, torch.float32, who + ': x', rank=3)
    n = n4_lattice(x.shape, stride, who)
    s = _core.int3(stride, 'stride', who)
    if mask is not None:
        if isinstance(mask, torch.Tensor) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        _core.dense(mask, torch.uint8, who + ': mask', shape=x.shape)
    v = torch.empty(n, dtype=torch.float64, device=x.device)
    lm = torch.empty(n, dtype=torch.uint8, device=x.device)
    _core.lib().call('bts_n4_log_lattice', _core._p(x), _core._p(mask), x.shape[0], x.shape[1], x.shape[2], s[0], s[1], s[2], _core._p(v),
                     _core._p(lm), _core._stream())
    return v, lm


def n4_hist(v, f, lmask, bins=200):
    """-> (r, lohi, hist): r = v - f on the lattice mask (0 elsewhere), lohi = its exact (min, max) over the mask as 2 float64 on the device
    ((+inf, -inf) for an empty mask), hist = `bins` int64 counts with linear two-bin weights, 2^24 per masked point (bts_n4_range_hist)"""
    who = 'n4_hist'
    bins = _core.bin_count(bins, N4_MAX_BINS, who)
    n = _n4_points(v, who + ': v')
    _core.dense(f, torch.float64, who + ': f', shape=n)
    _core.dense(lmask, torch.uint8, who + ': lmask', shape=n)
    r = torch.empty(n, dtype=torch.float64, device=v.device)
    range4 = torch.empty(4, dtype=torch.float64, device=v.device)
    hist = torch.empty(bins, dtype=torch.int64, device=v.device)
    _core.lib().call('bts_n4_range_hist', _core._p(v), _core._p(f), _core._p(lmask), v.numel(), bins, _core._p(r), _core._p(range4), _core._p(hist),
                     _core._stream())
    return r, range4[:2], hist


def n4_residual(r, lmask, table, lo, sl):
    """-> res = r - (E[i] (1 - o) + E[i+1] o) on the mask, 0 elsewhere: the table E (`bins` float64 on the device) looked up at
    c = (r - lo) / sl, i = min(floor(c), bins - 2), o = c - i (bts_n4_residual); lo finite, sl >= 0 finite"""
    who = 'n4_residual'
    n = _n4_points(r, who + ': r')
    _core.dense(lmask, torch.uint8, who + ': lmask', shape=n)
    if not isinstance(table, torch.Tensor) or table.dim() != 1:
        raise ValueError('%s: the table must be a vector of float64 on the GPU' % who)
    bins = _core.bin_count(int(table.numel()), N4_MAX_BINS, who)
    _core.dense(table, torch.float64, who + ': table', shape=(bins,))
    lo, sl = float(lo), float(sl)
    if not (np.isfinite(lo) and np.isfinite(sl) and sl >= 0.0):
        raise ValueError('%s: lo must be finite and sl finite and not negative, got %r and %r' % (who, lo, sl))
    res = torch.empty(n, dtype=torch.float64, device=r.device)
    _core.lib().call('bts_n4_residual', _core._p(r), _core._p(lmask), _core._p(table), r.numel(), bins, lo, sl, _core._p(res), _core._stream())
    return res


def _n4_geometry(shape, stride, mesh, lmask, who):
    n = n4_lattice(shape, stride, who)
    mesh = _n4_mesh(mesh, who)
    _core.dense(lmask, torch.uint8, who + ': lmask', shape=n)
    shape, stride = _core.int3(shape, 'shape', who), _core.int3(stride, 'stride', who)
    return n, mesh, shape + stride + mesh


def n4_fit(res, lmask, shape, stride, mesh, phi=None):
    """one level of multilevel B-spline approximation of the residuals on the lattice of `stride` in a volume of `shape` -> (num, den,
    dphi), float64 of shape mesh + 3: num = sum w^3 z / S, den = sum w^2 over the masked lattice points in each control point's support,
    dphi = num / den, 0 where den == 0; phi (the same shape), when given, grows by dphi in place (bts_n4_fit)"""
    who = 'n4_fit'
    n, mesh, geo = _n4_geometry(shape, stride, mesh, lmask, who)
    if max(n) > N4_MAX_AXIS:
        raise ValueError('%s: at most %d lattice points per axis, got %s' % (who, N4_MAX_AXIS, n))
    _core.dense(res, torch.float64, who + ': res', shape=n)
    cp = tuple(m + 3 for m in mesh)
    if phi is not None:
        _core.dense(phi, torch.float64, who + ': phi', shape=cp)
    num, den, dphi = (torch.empty(cp, dtype=torch.float64, device=res.device) for _ in range(3))
    _core.lib().call('bts_n4_fit', _core._p(res), _core._p(lmask),
                     *(geo + (_core._p(num), _core._p(den), _core._p(dphi), _core._p(phi), _core._stream())))
    return num, den, dphi


def n4_eval(phi, lmask, f_old, shape, stride, mesh):
    """-> (f_new, parts): the spline of phi (float64, mesh + 3) at every lattice point, and parts (B,2) float64, the sums of
    e = exp(f_new - f_old) and e^2 over the masked points of each run of 1024 lattice points (bts_n4_eval)"""
    who = 'n4_eval'
    n, mesh, geo = _n4_geometry(shape, stride, mesh, lmask, who)
    _core.dense(phi, torch.float64, who + ': phi', shape=tuple(m + 3 for m in mesh))
    _core.dense(f_old, torch.float64, who + ': f_old', shape=n)
    f_new = torch.empty(n, dtype=torch.float64, device=phi.device)
    parts = torch.empty((_core.lib().query('bts_n4_eval_parts', n[0] * n[1] * n[2]), 2), dtype=torch.float64, device=phi.device)
    _core.lib().call('bts_n4_eval', _core._p(phi), *(geo + (_core._p(f_old), _core._p(lmask), _core._p(f_new), _core._p(parts), _core._stream())))
    return f_new, parts


def n4_apply(x, phi, mesh, field=False):
    """dense float32 (D,H,W) device volume -> float32(x / exp(spline of phi)) at every voxel; with field=True also float32(exp(spline))
    (bts_n4_apply)"""
    who = 'n4_apply'
    _core.dense(x, torch.float32, who + ': x', rank=3)
    n4_lattice(x.shape, (1, 1, 1), who)
    mesh = _n4_mesh(mesh, who)
    _core.dense(phi, torch.float64, who + ': phi', shape=tuple(m + 3 for m in mesh))
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    fld = torch.empty(x.shape, dtype=torch.float32, device=x.device) if field else None
    _core.lib().call('bts_n4_apply', _core._p(x), x.shape[0], x.shape[1], x.shape[2], _core._p(phi), mesh[0], mesh[1], mesh[2], _core._p(out),
                     _core._p(fld), _core._stream())
    return (out, fld) if field else out
