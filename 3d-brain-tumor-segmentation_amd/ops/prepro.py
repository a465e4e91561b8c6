"""Dataset preprocessing on the device (csrc/prepro.hip; preprocess.py:17-131) and the per-case normalisation over the brain voxels
(csrc/casenorm.hip).  Both read WINDOWS: views made by slicing a dense channels-last volume on its spatial axes."""
import torch

from . import _core


def _window(v, name, shape=None):
    """THE window rule: a float32 (T0,T1,T2,C) view on the GPU (of `shape`, where given) made by slicing a dense (S0,S1,S2,C) parent on its
    three spatial axes -> its strides (st0, st1); no copy is ever made here"""
    if not isinstance(v, torch.Tensor) or v.dim() != 4 or (shape is not None and tuple(v.shape) != tuple(shape)):
        raise ValueError('%s must be a (T0,T1,T2,C) window%s' % (name, '' if shape is None else ' of shape %s' % (tuple(shape),)))
    if not v.is_cuda or v.dtype != torch.float32:
        raise ValueError('%s must be a float32 tensor on the GPU' % name)
    c = v.shape[3]
    if min(v.shape) < 1:
        raise ValueError('%s must have shape (T0,T1,T2,%d), got %s' % (name, c, tuple(v.shape)))
    if v.stride(3) != 1 or v.stride(2) != c:
        raise ValueError('%s must be a spatial slice of a dense channels-last volume (strides (*,*,%d,1)), got strides %s'
                         % (name, c, v.stride()))
    if v.stride(1) < v.shape[2] * c or v.stride(0) < v.shape[1] * v.stride(1):
        raise ValueError('%s: strides %s overlap for shape %s' % (name, v.stride(), tuple(v.shape)))
    return v.stride(0), v.stride(1)


def prepro_occupancy(x, occ):
    """sets occ[a] = 1 (int32, S0+S1+S2 entries, axis 0 first) for every plane of every axis of the dense (S0,S1,S2,C) volume x that
    holds an x != 0; never clears a flag, so one zeroed buffer collects a whole dataset"""
    _window(x, 'prepro_occupancy: x')
    if not x.is_contiguous():
        raise ValueError('prepro_occupancy: x must be dense, got strides %s' % (x.stride(),))
    s0, s1, s2, c = x.shape
    _core.dense(occ, torch.int32, 'prepro_occupancy: occ', numel=s0 + s1 + s2)
    _core.lib().call('bts_prepro_occupancy', _core._p(x), _core._p(occ), s0, s1, s2, c, _core._stream())
    return occ


def prepro_sums(v, acc, mean=None):
    """window v (T0,T1,T2,C) of a dense volume.  mean None: acc[0:C] += sum x, acc[C:2C] += #(x > 0); mean (C float64 on the GPU):
    acc[0:C] += sum (x - mean)^2.  acc: float64 on the GPU (2C / C values); fp64 throughout, fixed summation order"""
    st0, st1 = _window(v, 'prepro_sums: v')
    c = v.shape[3]
    _core.dense(acc, torch.float64, 'prepro_sums: acc', numel=c if mean is not None else 2 * c)
    if mean is not None:
        _core.dense(mean, torch.float64, 'prepro_sums: mean', numel=c)
    ws, nb = _core.scratch('bts_prepro_workspace', v.device, c)
    _core.lib().call('bts_prepro_sums', _core._p(v), st0, st1, v.shape[0], v.shape[1], v.shape[2], c, _core._p(mean), _core._p(acc), _core._p(ws), nb,
                     _core._stream())
    return acc


def prepro_crop_norm(v, yv, mean, std):
    """windows v (T0,T1,T2,C) and yv (T0,T1,T2,1) (or None) -> dense (float((double(x) - mean) / std), y with labels >= 4 -> 3);
    mean, std: C float64 values on the GPU"""
    st0, st1 = _window(v, 'prepro_crop_norm: x')
    t0, t1, t2, c = v.shape
    _core.dense(mean, torch.float64, 'prepro_crop_norm: mean', numel=c)
    _core.dense(std, torch.float64, 'prepro_crop_norm: std', numel=c)
    xo = torch.empty((t0, t1, t2, c), dtype=torch.float32, device=v.device)
    yo, yst0, yst1 = None, 0, 0
    if yv is not None:
        yst0, yst1 = _window(yv, 'prepro_crop_norm: y', shape=(t0, t1, t2, 1))
        yo = torch.empty((t0, t1, t2, 1), dtype=torch.float32, device=v.device)
    _core.lib().call('bts_prepro_crop_norm', _core._p(v), _core._p(yv), st0, st1, yst0, yst1, t0, t1, t2, c, _core._p(mean), _core._p(std),
                     _core._p(xo), _core._p(yo), _core._stream())
    return xo, yo


def check_clip(clip, who='clip'):
    """None | (lo, hi) with 0 <= lo <= hi <= 100 -> None | (float, float)"""
    if clip is None:
        return None
    try:
        lo, hi = (float(v) for v in clip)
    except (TypeError, ValueError):
        raise ValueError('%s must be None or two percentiles (lo, hi), got %r' % (who, clip))
    if not 0.0 <= lo <= hi <= 100.0:
        raise ValueError('%s: percentiles must satisfy 0 <= lo <= hi <= 100, got %r' % (who, clip))
    return lo, hi


def case_norm(x, mask=None, clip=None, y=None, out=None):
    """normalise one case on its own voxels: window x (T0,T1,T2,C) of a dense channels-last volume -> (xn, stats), or (xn, yn, stats)
    with a label window y (T0,T1,T2,1) (labels >= 4 -> 3, as prepro_crop_norm).  mask: float32 window (T0,T1,T2) or (T0,T1,T2,1),
    non-zero = inside; None: a voxel is inside when any of its channels is > 0.  clip: None or the percentiles (lo, hi) the inside values of
    each channel are clamped to first.  xn (dense, `out` when given) = float32((clamp(x) - mean_c) / std_c) inside, evaluated in
    float64, +0.0 outside, +0.0 throughout a channel whose deviation is 0; mean_c and std_c (population) over the inside voxels.
    stats: 1 + 4C float64 on the device: n, then (mean, std, lo, hi) per channel.  Everything stays on the stream (bts_case_norm)."""
    st0, st1 = _window(x, 'case_norm: x')
    t0, t1, t2, c = x.shape
    clip = check_clip(clip, 'case_norm: clip')
    mst0 = mst1 = 0
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or tuple(mask.shape) not in ((t0, t1, t2), (t0, t1, t2, 1)):
            raise ValueError('case_norm: mask must have shape %s or %s' % ((t0, t1, t2), (t0, t1, t2, 1)))
        mask = mask if mask.dim() == 4 else mask.unsqueeze(-1)
        mst0, mst1 = _window(mask, 'case_norm: mask')
    yo, yst0, yst1 = None, 0, 0
    if y is not None:
        yst0, yst1 = _window(y, 'case_norm: y', shape=(t0, t1, t2, 1))
        yo = torch.empty((t0, t1, t2, 1), dtype=torch.float32, device=x.device)
    out = _core.out_or_new(out, (t0, t1, t2, c), torch.float32, x.device, 'case_norm: out')
    stats = torch.empty(1 + 4 * c, dtype=torch.float64, device=x.device)
    ws, nb = _core.scratch('bts_case_norm_workspace', x.device, c)
    lo, hi = clip if clip is not None else (0.0, 100.0)
    _core.lib().call('bts_case_norm', _core._p(x), st0, st1, _core._p(mask), mst0, mst1, _core._p(y), yst0, yst1, t0, t1, t2, c,
                     1 if clip is not None else 0, lo, hi, _core._p(out), _core._p(yo), _core._p(stats), _core._p(ws), nb, _core._stream())
    return (out, stats) if y is None else (out, yo, stats)
