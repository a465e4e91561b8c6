"""Sliding-window inference (csrc/window.hip): gather a batch of windows, blend the predictions back, count a mask per window."""
import ctypes

import torch

from . import _core


def window_batch_max():
    """jobs one launch of bts_window_gather / bts_window_accumulate carries"""
    return int(_core.lib().query('bts_window_batch_max'))


def _window_jobs(who, starts, flips):
    """the host side of a job list -> (B, 3B ints, B ints) as host arrays"""
    n = len(flips)
    if n == 0 or len(starts) != n or any(len(s) != 3 for s in starts):
        raise ValueError('%s: %d flips need as many (z0,y0,x0) starts, got %d' % (who, n, len(starts)))
    return n, _core.carray(ctypes.c_int, [v for tri in starts for v in tri], 3 * n), _core.carray(ctypes.c_int, flips)


def window_gather(x, roi, starts, flips, means, stds, out=None):
    """x (D,H,W,C) dense float32; roi (R0,R1,R2); per job b: starts[b] = (z0,y0,x0) inside the volume, flips[b] (bits 4|2|1 = D|H|W),
    means[b] / stds[b] = C host floats -> out (B,R0,R1,R2,C): the window normalised and flipped, (0 - mean) / std beyond the volume's end.
    out: a dense float32 tensor of that shape to write into"""
    _core.volume(x, 'window_gather: x')
    d, h, w, c = x.shape
    r0, r1, r2 = (int(v) for v in roi)
    n, st, fl = _window_jobs('window_gather', starts, flips)
    if len(means) != n or len(stds) != n or any(len(m) != c for m in means) or any(len(s) != c for s in stds):
        raise ValueError('window_gather: every one of the %d jobs needs %d means and %d stds' % (n, c, c))
    out = _core.out_or_new(out, (n, r0, r1, r2, c), torch.float32, x.device, 'window_gather: out', rule=_core.volume)
    mean = _core.carray(ctypes.c_float, [v for row in means for v in row])
    std = _core.carray(ctypes.c_float, [v for row in stds for v in row])
    _core.lib().call('bts_window_gather', _core._p(x), _core._p(out), d, h, w, c, r0, r1, r2, n, st, fl, mean, std, _core._stream())
    return out


def window_accumulate(pred, acc, tables, starts, flips, rows, scale=1.0):
    """pred (B,R0,R1,R2,K): the forward's output for the jobs, still flipped; acc (D,H,W,K), updated IN PLACE; tables = (nz (n0,R0),
    ny (n1,R1), nx (n2,R2)) dense float32 on the GPU (infer.window_plan's, as float32); per job b: starts[b], flips[b] as in
    window_gather and rows[b] = (iz,iy,ix), its window's rows in the tables.
    acc[z0+d, y0+h, x0+w, k] += scale * nz[iz][d] * ny[iy][h] * nx[ix][w] * pred[b, fd(d), fh(h), fw(w), k] inside the volume -> acc"""
    _core.volume(acc, 'window_accumulate: acc')
    _core._check(pred, 'window_accumulate: pred')
    d, h, w, k = acc.shape
    if pred.dim() != 5 or not pred.is_contiguous() or pred.shape[4] != k:
        raise ValueError('window_accumulate: pred must be a dense (B,R0,R1,R2,%d) tensor, got shape %s strides %s'
                         % (k, tuple(pred.shape), pred.stride()))
    n, st, fl = _window_jobs('window_accumulate', starts, flips)
    r0, r1, r2 = (int(v) for v in pred.shape[1:4])
    if pred.shape[0] != n or len(rows) != n or any(len(r) != 3 for r in rows):
        raise ValueError('window_accumulate: pred holds %d jobs, the lists %d starts and %d rows' % (pred.shape[0], n, len(rows)))
    if len(tables) != 3:
        raise ValueError('window_accumulate: tables must be (nz, ny, nx)')
    for t, r, name in zip(tables, (r0, r1, r2), ('nz', 'ny', 'nx')):
        _core._check(t, 'window_accumulate: ' + name)
        if t.dim() != 2 or t.shape[1] != r or t.shape[0] < 1 or not t.is_contiguous():
            raise ValueError('window_accumulate: %s must be a dense (windows, %d) tensor, got shape %s' % (name, r, tuple(t.shape)))
    rw = _core.carray(ctypes.c_int, [v for tri in rows for v in tri])
    _core.lib().call('bts_window_accumulate', _core._p(pred), _core._p(acc), _core._p(tables[0]), _core._p(tables[1]), _core._p(tables[2]),
                     tables[0].shape[0], tables[1].shape[0], tables[2].shape[0], d, h, w, k, r0, r1, r2, n, st, fl, rw, float(scale), _core._stream())
    return acc


def window_occupancy(mask, roi, starts, out=None):
    """mask (D,H,W,1) dense float32; starts = (z starts, y starts, x starts) of a window plan -> int32 (n0,n1,n2) on the GPU: the voxels
    with mask > 0 inside each window, clipped to the volume.  out: a dense int32 tensor of that shape to write into"""
    _core.volume(mask, 'window_occupancy: mask')
    d, h, w, c = mask.shape
    if c != 1:
        raise ValueError('window_occupancy: mask must have shape (D,H,W,1), got %s' % (tuple(mask.shape),))
    if len(starts) != 3 or any(len(s) == 0 for s in starts):
        raise ValueError('window_occupancy: starts must be three non-empty lists, got %r' % (starts,))
    r0, r1, r2 = (int(v) for v in roi)
    n0, n1, n2 = (len(s) for s in starts)
    out = _core.out_or_new(out, (n0, n1, n2), torch.int32, mask.device, 'window_occupancy: out')
    st = torch.tensor([int(v) for s in starts for v in s], dtype=torch.int32).to(mask.device)
    _core.lib().call('bts_window_occupancy', _core._p(mask), _core._p(st), _core._p(out), n0, n1, n2, d, h, w, r0, r1, r2, _core._stream())
    return out
