"""Training-time augmentation on the device: crop / flip / intensity shift (csrc/augment.hip), the spatial transform, and the
intensity stages applied to an augmented batch (csrc/intensity.hip)."""
import ctypes

import torch

from . import _core

INTENSITY_NOISE, INTENSITY_BLUR, INTENSITY_BRIGHT, INTENSITY_CONTRAST, INTENSITY_GAMMA, INTENSITY_INVERT = 1, 2, 4, 8, 16, 32


def channel_moments(x):
    """per-channel (mean, population variance) over all voxels of a dense (..., C) tensor, C <= 16 -> two (C,) tensors"""
    _core._check(x, 'x')
    c = x.shape[-1]
    nvox = x.numel() // c
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    var = torch.empty(c, dtype=torch.float32, device=x.device)
    ws, nb = _core.scratch('bts_channel_moments_workspace', x.device, c)
    _core.lib().call('bts_channel_moments', _core._p(x.contiguous()), _core._p(mean), _core._p(var), _core._p(ws), nb, nvox, c, c, _core._stream())
    return mean, var


CLASS_LOCATIONS_MAX_CLASSES = 8


def class_locations(y, out_ch, k):
    """the class-location table of a label volume (bts_class_locations), for foreground-oversampled crops.  y: dense float32 labels on
    the GPU as the dataset stores them, (S0,S1,S2) or (S0,S1,S2,1), label c+1 = class c (the convention of augment_crop's one-hot); out_ch
    in 1..8; k >= 1 the table's capacity per class -> (counts int64 (out_ch,), loc int32 (out_ch, k)) on the device: counts[c] = n_c, the
    voxels whose label is exactly c+1; loc[c, j] the linear index of the class's voxel of rank j * s_c in ascending index order,
    s_c = max(1, ceil(n_c / k)), for j < ceil(n_c / s_c), and -1 from there on.  Bit-identical from call to call.  Every refusal is a
    ValueError raised before the library is reached."""
    who = 'class_locations'
    if not isinstance(y, torch.Tensor):
        raise ValueError('%s: y must be a dense float32 tensor on the GPU' % who)
    try:
        _core._check(y, who + ': y')
    except RuntimeError as e:      # (_check speaks RuntimeError for the training step's wrappers; this one refuses with ValueError throughout)
        raise ValueError(str(e))
    if y.dim() not in (3, 4) or (y.dim() == 4 and y.shape[3] != 1) or not y.is_contiguous():
        raise ValueError('%s: y must be a dense (S0,S1,S2) or (S0,S1,S2,1) volume, got shape %s' % (who, tuple(y.shape)))
    for name, v, lo, hi in (('out_ch', out_ch, 1, CLASS_LOCATIONS_MAX_CLASSES), ('k', k, 1, 2 ** 31 - 1)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError('%s: %s must be an integer in %d..%d, got %r' % (who, name, lo, hi, v))
    nvox = y.numel()
    if not 1 <= nvox < 2 ** 31:
        raise ValueError('%s: y must hold between 1 and 2^31 - 1 voxels, got %d' % (who, nvox))
    counts = torch.empty(out_ch, dtype=torch.int64, device=y.device)
    loc = torch.empty((out_ch, k), dtype=torch.int32, device=y.device)
    ws, nb = _core.scratch('bts_class_locations_workspace', y.device, nvox, out_ch)
    _core.lib().call('bts_class_locations', _core._p(y), _core._p(counts), _core._p(loc), _core._p(ws), nb, nvox, out_ch, k, _core._stream())
    return counts, loc


def augment_crop(x, y, var, crop, offsets, flip_mask, shift, scale, out_ch):
    """x: (S0,S1,S2,C), y: (S0,S1,S2) or (S0,S1,S2,1) float labels, var: (C,) device tensor; shift/scale: C python floats
    -> (x_out (T0,T1,T2,C), y_out (T0,T1,T2,out_ch))"""
    s0, s1, s2, c = x.shape
    t0, t1, t2 = crop
    xo = torch.empty((t0, t1, t2, c), dtype=torch.float32, device=x.device)
    yo = torch.empty((t0, t1, t2, out_ch), dtype=torch.float32, device=x.device)
    _core.lib().call('bts_augment_crop', _core._p(x.contiguous()), _core._p(y.contiguous()), _core._p(var), _core._p(xo), _core._p(yo), s0, s1, s2, c,
                     t0, t1, t2, int(offsets[0]), int(offsets[1]), int(offsets[2]), int(flip_mask), _core.carray(ctypes.c_float, shift, c),
                     _core.carray(ctypes.c_float, scale, c), int(out_ch), _core._stream())
    return xo, yo


def _count(who, xs, *lists):
    """the number of examples of a batch launch, which every one of `lists` (labels, variances, host draws) must match"""
    if len(xs) == 0 or any(len(a) != len(xs) for a in lists):
        raise ValueError('%s: %d examples need as many labels, variances and draws' % (who, len(xs)))
    return len(xs)


def _examples(who, xs, ys, variances):
    """every volume of a batch launch is a dense float32 tensor on the GPU of one shape (S0,S1,S2,C), with S0*S1*S2 labels and C variances
    -> (S0, S1, S2, C)"""
    s0, s1, s2, c = xs[0].shape
    for x, y, v in zip(xs, ys, variances):
        _core._check(x, 'x'), _core._check(y, 'y'), _core._check(v, 'var')
        if tuple(x.shape) != (s0, s1, s2, c) or y.numel() != s0 * s1 * s2 or v.numel() != c:
            raise ValueError('%s: every example must be a (%d,%d,%d,%d) volume with its labels and %d variances' % (who, s0, s1, s2, c, c))
        if not (x.is_contiguous() and y.is_contiguous() and v.is_contiguous()):
            raise ValueError('%s: dense tensors only' % who)
    return s0, s1, s2, c


def _batch_out(who, out, n, crop, c, out_ch, channels_first, device):
    """the batch tensors a launch writes -> (x, y): new, or the caller's pair checked to be dense float32 of the launch's shapes"""
    xo, yo = (None, None) if out is None else out
    if out is not None:      # (device and dtype of both before the shape of either)
        _core._check(xo, who + ': out x'), _core._check(yo, who + ': out y')
    xo = _core.out_or_new(xo, (n, c) + crop if channels_first else (n,) + crop + (c,), torch.float32, device, who + ': out x', rule=_core.volume)
    yo = _core.out_or_new(yo, (n, out_ch) + crop if channels_first else (n,) + crop + (out_ch,), torch.float32, device, who + ': out y',
                          rule=_core.volume)
    return xo, yo


def _ptrs(tensors):
    """the addresses of a list of tensors (None: a null pointer) as a host array of pointers"""
    return ctypes.cast((ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors]), ctypes.c_void_p)


def _draws(n, c, offsets, flip_masks, shifts, scales):
    """the per-example draws of augment_crop as host arrays: 3N ints, N ints, N*C floats, N*C floats"""
    return (_core.carray(ctypes.c_int, [o for tri in offsets for o in tri], 3 * n), _core.carray(ctypes.c_int, flip_masks, n),
            _core.carray(ctypes.c_float, [v for row in shifts for v in row], n * c),
            _core.carray(ctypes.c_float, [v for row in scales for v in row], n * c))


def augment_batch_max():
    """examples one launch of bts_augment_batch carries (ops.augment_batch takes any number: the call splits)"""
    return int(_core.lib().query('bts_augment_batch_max'))


def augment_batch(xs, ys, variances, crop, offsets, flip_masks, shifts, scales, out_ch, channels_first=False, out=None):
    """augment_crop for N examples in one launch, written straight into the batch tensors.  xs: N dense (S0,S1,S2,C) tensors of one
    shape, ys: their labels, variances: N (C,) device tensors; offsets: N triples, flip_masks: N ints, shifts / scales: N lists of
    C floats -> (x (N,T0,T1,T2,C), y (N,T0,T1,T2,out_ch)), or with channels_first (N,C,T0,T1,T2), (N,out_ch,T0,T1,T2).
    out: (x, y) dense tensors of those shapes to write into (views of larger buffers are fine)"""
    n = _count('augment_batch', xs, ys, variances, offsets, flip_masks, shifts, scales)
    s0, s1, s2, c = _examples('augment_batch', xs, ys, variances)
    t0, t1, t2 = (int(t) for t in crop)
    xo, yo = _batch_out('augment_batch', out, n, (t0, t1, t2), c, out_ch, channels_first, xs[0].device)
    off, fl, sh, sc = _draws(n, c, offsets, flip_masks, shifts, scales)
    _core.lib().call('bts_augment_batch', _ptrs(xs), _ptrs(ys), _ptrs(variances), _core._p(xo), _core._p(yo), n, s0, s1, s2, c, t0, t1, t2, off, fl,
                     sh, sc, int(out_ch), 1 if channels_first else 0, _core._stream())
    return xo, yo


def augment_spatial_batch_max():
    """examples one launch of bts_augment_spatial_batch carries (ops.augment_spatial_batch takes any number: the call splits)"""
    return int(_core.lib().query('bts_augment_spatial_batch_max'))


def augment_spatial_batch(xs, ys, variances, crop, offsets, flip_masks, shifts, scales, out_ch, spatial, matrices, phis, spacings,
                          fills=None, channels_first=False, out=None):
    """augment_batch with a spatial transform per example (bts_augment_spatial_batch: s = o + (T-1)/2 + M (t~ - (T-1)/2) + u(t~),
    trilinear image with `fill` outside the volume, nearest labels).  The arguments of augment_batch plus, per example: spatial (a
    false flag: the plain copy, bit-equal to augment_batch), matrices (9 floats, row-major, or a 3x3 nesting), phis (a dense fp32
    (G0,G1,G2,3) device tensor with G_k = (T_k-1)//spacing + 4, or None for no elastic part), spacings (ints >= 1) and fills (C floats
    each; None: zeros) -> the tensors of augment_batch"""
    who = 'augment_spatial_batch'
    n = _count(who, xs, ys, variances, offsets, flip_masks, shifts, scales)
    if not (len(spatial) == len(matrices) == len(phis) == len(spacings) == n) or (fills is not None and len(fills) != n):
        raise ValueError('augment_spatial_batch: %d examples need as many flags, matrices, fields, spacings and fills' % n)
    s0, s1, s2, c = _examples(who, xs, ys, variances)
    t0, t1, t2 = (int(t) for t in crop)
    mats = []
    for m in matrices:
        flat = [float(v) for row in m for v in row] if len(m) == 3 else [float(v) for v in m]
        if len(flat) != 9:
            raise ValueError('augment_spatial_batch: a matrix is 9 floats')
        mats += flat
    for ph, sp in zip(phis, spacings):
        if int(sp) < 1:
            raise ValueError('augment_spatial_batch: spacing must be >= 1, got %r' % (sp,))
        if ph is None:
            continue
        _core._check(ph, 'phi')
        g = tuple((t - 1) // int(sp) + 4 for t in (t0, t1, t2)) + (3,)
        if tuple(ph.shape) != g or not ph.is_contiguous():
            raise ValueError('augment_spatial_batch: phi must be a dense %s tensor for spacing %d, got %s' % (g, int(sp), tuple(ph.shape)))
    if fills is None:
        fills = [[0.0] * c] * n
    if any(len(f) != c for f in fills):
        raise ValueError('augment_spatial_batch: a fill is %d floats' % c)
    xo, yo = _batch_out(who, out, n, (t0, t1, t2), c, out_ch, channels_first, xs[0].device)
    off, fl, sh, sc = _draws(n, c, offsets, flip_masks, shifts, scales)
    _core.lib().call('bts_augment_spatial_batch', _ptrs(xs), _ptrs(ys), _ptrs(variances), _core._p(xo), _core._p(yo), n, s0, s1, s2, c, t0, t1, t2,
                     off, fl, sh, sc, _core.carray(ctypes.c_int, [1 if f else 0 for f in spatial]), _core.carray(ctypes.c_float, mats), _ptrs(phis),
                     _core.carray(ctypes.c_int, spacings), _core.carray(ctypes.c_float, [v for row in fills for v in row], n * c), int(out_ch),
                     1 if channels_first else 0, _core._stream())
    return xo, yo


def intensity_blur_weights(sigma):
    """(radius, the radius + 1 float weights w[|j|]) of the Gaussian blur of `sigma` as bts_intensity_batch applies it (host only)"""
    buf = (ctypes.c_float * 17)()
    r = _core.lib().probe('bts_intensity_blur_weights', float(sigma), ctypes.cast(buf, ctypes.c_void_p))
    if r < 0:
        raise ValueError('intensity_blur_weights: sigma must be positive with a radius int(4 sigma + 0.5) <= 16, got %r' % (sigma,))
    return int(r), [float(buf[k]) for k in range(r + 1)]


def intensity_batch(x, params, keys, channels_first=False):
    """Gaussian noise, Gaussian blur, brightness, contrast and gamma on the batch an augment launch wrote, IN PLACE (-> x).
    x: dense fp32 (N,T0,T1,T2,C), or (N,C,T0,T1,T2) with channels_first.  params: N rows of C entries
    (flags, s, sigma, m, f, gamma), flags a sum of INTENSITY_*; a stage whose flag is off ignores its number.  keys: N pairs
    (k0, k1) of uint32, the Philox key of each example's noise.  The semantics are written above bts_intensity_batch in
    include/bts_hip.h; an (n, c) without a flag is not written."""
    _core.volume(x, 'intensity_batch: x', rank=5)
    if channels_first:
        n, c, t0, t1, t2 = x.shape
    else:
        n, t0, t1, t2, c = x.shape
    if n == 0 or len(params) != n or len(keys) != n:
        raise ValueError('intensity_batch: %d examples need as many parameter rows and keys' % n)
    fl, pr, ky = [], [], []
    for row, key in zip(params, keys):
        if len(row) != c or len(key) != 2:
            raise ValueError('intensity_batch: a parameter row has %d entries of (flags, s, sigma, m, f, gamma), a key two words' % c)
        for e in row:
            if len(e) != 6:
                raise ValueError('intensity_batch: an entry is (flags, s, sigma, m, f, gamma)')
            fl.append(int(e[0]))
            pr.extend(float(v) for v in e[1:])
        ky.extend(int(k) & 0xffffffff for k in key)
    ws, nb = _core.scratch('bts_intensity_batch_workspace', x.device, n, t0, t1, t2, c)
    _core.lib().call('bts_intensity_batch', _core._p(x), n, t0, t1, t2, c, 1 if channels_first else 0, _core.carray(ctypes.c_int, fl),
                     _core.carray(ctypes.c_float, pr), _core.carray(ctypes.c_uint32, ky), _core._p(ws), ws.numel(), _core._stream())
    return x
