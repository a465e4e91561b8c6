"""Whole-volume inference: test-time augmentation, resampling a scan to the 1 mm^3 grid and back (csrc/resample.hip;
test.py:15-72), conforming it to an oriented grid by its affine (csrc/conform.hip; infer.Conformer) and the two-stage hand-over
(csrc/segment.hip; test.py:181-270)."""
import torch

from . import _core


def flip_affine(src, flip_mask=0, mean=None, std=None, scale=1.0, out=None, accumulate=False):
    """out (+)= scale * t(flip(src)); flip_mask bits 4|2|1 = reverse D|H|W; t = (v - mean[c]) / std[c] when given"""
    _core._check(src, 'src')
    if not src.is_contiguous():
        raise ValueError('flip_affine: src must be a dense NDHWC tensor')
    n, d, h, w, c = src.shape
    if out is None:
        if accumulate:
            raise ValueError('flip_affine: accumulate needs an output tensor')
        out = torch.empty_like(src)
    _core.lib().call('bts_flip_affine', _core._p(src), _core._p(out), _core._p(mean), _core._p(std), n, d, h, w, c, int(flip_mask), float(scale),
                     1 if accumulate else 0, _core._stream())
    return out


def tta_finish(prob, bmask, threshold=0.5, want_probabilities=True, want_labels=True):
    """-> (prob * bmask, uint8 label map): argmax + 1, >= 3 -> 4, 0 where masked out / below threshold"""
    n, d, h, w, c = prob.shape
    y = torch.empty_like(prob) if want_probabilities else None
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=prob.device) if want_labels else None
    _core.lib().call('bts_tta_finish', _core._p(prob.contiguous()), _core._p(bmask.contiguous()), _core._p(y), _core._p(labels), n * d * h * w, c,
                     float(threshold), _core._stream())
    return y, labels


def ensemble_update(p, mean, m2, k):
    """member k (counted from 1) of an ensemble, in place: d = p - mean; mean += d / k; m2 += d * (p - mean) over dense float32 tensors of
    one size (Welford's recurrence, the float32 numpy expression bit for bit).  k == 1 writes mean = p and m2 = 0 without reading them.
    mean None (k == 1 only): a new tensor of p's shape; m2 None: only the mean is kept  -> (mean, m2)   [csrc/ensemble.hip]"""
    f32 = torch.float32
    _core.dense(p, f32, 'ensemble_update: p')
    k = int(k)
    if k < 1:
        raise ValueError('ensemble_update: k counts the members from 1, got %r' % (k,))
    if mean is None and k != 1:
        raise ValueError('ensemble_update: member %d needs the mean of the members before it' % k)
    mean = _core.out_or_new(mean, p.shape, f32, p.device, 'ensemble_update: mean', numel=p.numel())
    if m2 is not None:
        _core.dense(m2, f32, 'ensemble_update: m2', numel=p.numel())
    _core.lib().call('bts_ensemble_update', _core._p(p), _core._p(mean), _core._p(m2), p.numel(), k, _core._stream())
    return mean, m2


UNCERTAINTY_MODES = ('entropy', 'std')


def uncertainty_finish(mean, bmask, mode='entropy', spread=None, scale=1.0, out=None):
    """-> uint8 levels 0..100 of `mean`'s shape (..., C), channels last, 0 where bmask (one float per voxel) == 0.
    'entropy': of p = clamp(mean, 0, 1), h = -(p log2 p + (1 - p) log2(1 - p)), level = min(100, floor(100 h + 0.5)).
    'std': level = min(100, floor(200 sqrt(max(spread, 0) * scale) + 0.5)); spread (of mean's shape) = ensemble_update's m2 with
    scale = 1 / members, or a variance with scale = 1; only the shape of `mean` is read.  out: a dense uint8 tensor of that many
    values to write into   [csrc/ensemble.hip]"""
    f32 = torch.float32
    if mode not in UNCERTAINTY_MODES:
        raise ValueError('uncertainty_finish: mode must be one of %s, got %r' % (UNCERTAINTY_MODES, mode))
    _core.dense(mean, f32, 'uncertainty_finish: mean')
    if mean.dim() < 1 or mean.numel() == 0:
        raise ValueError('uncertainty_finish: mean must have shape (..., C), got %s' % (tuple(mean.shape),))
    c = int(mean.shape[-1])
    nvox = mean.numel() // c
    _core.dense(bmask, f32, 'uncertainty_finish: bmask', numel=nvox)
    if mode == 'std':
        if spread is None:
            raise ValueError("uncertainty_finish: mode 'std' needs the spread")
        _core.dense(spread, f32, 'uncertainty_finish: spread', numel=mean.numel())
    out = _core.out_or_new(out, mean.shape, torch.uint8, mean.device, 'uncertainty_finish: out', numel=mean.numel())
    _core.lib().call('bts_uncertainty_finish', _core._p(mean), _core._p(spread if mode == 'std' else None), _core._p(bmask), _core._p(out), nvox,
                     c, UNCERTAINTY_MODES.index(mode), float(scale), _core._stream())
    return out


def spline_prefilter3d(x, out=None):
    """cubic B-spline coefficients of a dense (D,H,W,C) volume along D, H and W (the spline_filter half of
    scipy.ndimage.zoom(order=3, mode='reflect')); C <= 8, spatial extents >= 4"""
    _core.volume(x, 'spline_prefilter3d: x')
    d, h, w, c = x.shape
    out = _core.out_or_new(out, x.shape, torch.float32, x.device, 'spline_prefilter3d: out')
    _core.lib().call('bts_spline_prefilter3d', _core._p(x), _core._p(out), d, h, w, c, _core._stream())
    return out


def zoom3d(coef, out_shape, order=3, pad_to=None, want_mask=False, mean=None, std=None):
    """coef (D,H,W,C) evaluated on zoom()'s grid of spatial extent out_shape: order 3 takes spline_prefilter3d coefficients, orders 0
    and 1 the samples themselves.  pad_to >= out_shape: extent of the result, zero outside out_shape (pad_to_spatial_res in the same
    pass).  want_mask: also (max_c value > 0) as float32 (..., 1).  mean/std (C,): the result is normalised after the mask test.
    -> volume, or (volume, mask) with want_mask"""
    _core.volume(coef, 'zoom3d: coef')
    (do, ho, wo), (dp, hp, wp) = _core.grid('zoom3d', out_shape, pad_to, order)
    if (mean is None) != (std is None):
        raise ValueError('zoom3d: mean and std go together')
    d, h, w, c = coef.shape
    out = torch.empty((dp, hp, wp, c), dtype=torch.float32, device=coef.device)
    mask = torch.empty((dp, hp, wp, 1), dtype=torch.float32, device=coef.device) if want_mask else None
    _core.lib().call('bts_zoom3d', _core._p(coef), _core._p(out), _core._p(mask), _core._p(mean), _core._p(std), d, h, w, do, ho, wo, c, dp, hp, wp,
                     int(order), _core._stream())
    return (out, mask) if want_mask else out


def reorient3d(x, perm, flip, out=None):
    """x (D,H,W,C) -> the exact copy np.flip(np.transpose(x, perm + (3,)), [a for a in range(3) if flip[a]]): output axis a runs along
    axis perm[a] of x, reversed where flip[a]; C <= 8"""
    _core.volume(x, 'reorient3d: x')
    try:
        perm = tuple(int(v) for v in perm)
        flip = tuple(bool(v) for v in flip)
    except TypeError:
        perm, flip = (), ()
    if sorted(perm) != [0, 1, 2] or len(flip) != 3:
        raise ValueError('reorient3d: perm must be a permutation of (0, 1, 2) and flip three booleans, got %r and %r' % (perm, flip))
    d, h, w, c = x.shape
    given, out = out is not None, _core.out_or_new(out, tuple(x.shape[p] for p in perm) + (c,), torch.float32, x.device, 'reorient3d: out')
    if given and out.data_ptr() == x.data_ptr():
        raise ValueError('reorient3d: out must not be x')
    _core.lib().call('bts_reorient3d', _core._p(x), _core._p(out), d, h, w, c, perm[0], perm[1], perm[2], 4 * flip[0] + 2 * flip[1] + 1 * flip[2],
                     _core._stream())
    return out


def affine_resample3d(coef, matrix, out_shape, order=3, pad_to=None, out=None, channel=0, want_mask=False):
    """coef (D,H,W,C) evaluated where the 3x4 (or 4x4) float64 `matrix` sends the voxels of a grid of spatial extent out_shape: source
    voxel coordinate = matrix @ (o0, o1, o2, 1).  order 3 takes spline_prefilter3d coefficients, orders 0 and 1 the samples themselves;
    taps and the reflect rule are zoom3d's (order 1 is weighted and summed in float64 and rounded once).  Voxels whose coordinate lies outside [-0.5, n - 0.5] on any axis are 0, as are
    those of pad_to >= out_shape outside out_shape.  out: a dense float32 (pad_to, K) volume, K >= channel + C, whose channels
    channel .. channel+C-1 are written and whose others are left as they are (modalities on different grids: one call each).
    want_mask: also (max_c value > 0) as float32 (..., 1); only a call that writes every channel of the result can give it.
    -> volume, or (volume, mask) with want_mask"""
    _core.volume(coef, 'affine_resample3d: coef')
    (do, ho, wo), (dp, hp, wp) = _core.grid('affine_resample3d', out_shape, pad_to, order)
    m12, _ = _core.matrix12(matrix, 'affine_resample3d: matrix')
    d, h, w, c = coef.shape
    c0 = int(channel)
    if out is None:
        if c0 != 0:
            raise ValueError('affine_resample3d: channel %d needs an output volume to write into' % c0)
        out = torch.empty((dp, hp, wp, c), dtype=torch.float32, device=coef.device)
    else:
        _core.volume(out, 'affine_resample3d: out')
        if tuple(out.shape[:3]) != (dp, hp, wp) or c0 < 0 or c0 + c > out.shape[3]:
            raise ValueError('affine_resample3d: out has shape %s; channels %d .. %d of a %s volume are asked for'
                             % (tuple(out.shape), c0, c0 + c - 1, (dp, hp, wp)))
    ld = int(out.shape[3])
    if want_mask and (c0 != 0 or ld != c):
        raise ValueError('affine_resample3d: the mask is the maximum over all channels; this call writes %d of %d' % (c, ld))
    mask = torch.empty((dp, hp, wp, 1), dtype=torch.float32, device=coef.device) if want_mask else None
    _core.lib().call('bts_affine_resample3d', _core._p(coef), d, h, w, c, _core._p(out), ld, c0, _core._p(mask), do, ho, wo, dp, hp, wp, m12,
                     int(order), _core._stream())
    return (out, mask) if want_mask else out


def label_resample3d(y, matrix, out_shape, pad_to=None, out=None):
    """a label map through `matrix` (as affine_resample3d takes it): y, dense float32 (D,H,W) or (D,H,W,1) of label values (any finite
    values), read at the source voxel coordinate matrix @ (o0, o1, o2, 1) of every voxel of a grid of extent out_shape.  The 8 taps of
    order 1 vote with their float64 weights: the value with the largest summed weight wins, of exactly equal weights the smallest value
    -- the arg-max over classes of each class indicator interpolated linearly, in one gather.  0 outside the source's field of view
    [-0.5, n - 0.5] and in the padding of pad_to >= out_shape.  out: a dense float32 (pad_to, 1) volume to write into
    -> (pad_to or out_shape) + (1,) float32   [csrc/conform.hip]"""
    f32 = torch.float32
    _core.dense(y, f32, 'label_resample3d: y')
    if y.dim() not in (3, 4) or (y.dim() == 4 and y.shape[3] != 1) or y.numel() == 0:
        raise ValueError('label_resample3d: y must have shape (D,H,W) or (D,H,W,1), got %s' % (tuple(y.shape),))
    (do, ho, wo), (dp, hp, wp) = _core.grid('label_resample3d', out_shape, pad_to, 0)
    m12, _ = _core.matrix12(matrix, 'label_resample3d: matrix')
    d, h, w = (int(v) for v in y.shape[:3])
    given, out = out is not None, _core.out_or_new(out, (dp, hp, wp, 1), f32, y.device, 'label_resample3d: out')
    if given and out.data_ptr() == y.data_ptr():
        raise ValueError('label_resample3d: out must not be y')
    _core.lib().call('bts_label_resample3d', _core._p(y), d, h, w, _core._p(out), do, ho, wo, dp, hp, wp, m12, _core._stream())
    return out


def skull_strip(x, p, m, orig, pad_to, out=None):
    """x (Da,Ha,Wa,C), p and m (Da,Ha,Wa,1) dense float32; orig = the unpadded extent (D,H,W); pad_to = (Db,Hb,Wb) >= orig
    -> (xo (Db,Hb,Wb,C) = x * (1 - p) inside orig, 0 outside; mo (Db,Hb,Wb,1) = m inside, 0 outside)   [test.py:244-254]
    out: (xo, mo) dense float32 tensors of those shapes to write into"""
    _core.volume(x, 'skull_strip: x')
    da, ha, wa, c = x.shape
    _core.volume(p, 'skull_strip: p', shape=(da, ha, wa, 1))
    _core.volume(m, 'skull_strip: m', shape=(da, ha, wa, 1))
    d, h, w = (int(v) for v in orig)
    db, hb, wb = (int(v) for v in pad_to)
    xo, mo = (None, None) if out is None else (_core.volume(out[0], 'skull_strip: xo'), _core.volume(out[1], 'skull_strip: mo'))
    xo = _core.out_or_new(xo, (db, hb, wb, c), torch.float32, x.device, 'skull_strip: xo', rule=_core.volume)
    mo = _core.out_or_new(mo, (db, hb, wb, 1), torch.float32, x.device, 'skull_strip: mo', rule=_core.volume)
    _core.lib().call('bts_skull_strip', _core._p(x), _core._p(p), _core._p(m), _core._p(xo), _core._p(mo), da, ha, wa, d, h, w, db, hb, wb, c,
                     _core._stream())
    return xo, mo
