"""What every subject module of ops shares: the ABI's constants, pointers and the launch stream, the scratch buffers, and the argument rules,
each stated once.

The subject modules reach `lib`, `workspace`, `_check`, `_p` and `_stream` as attributes of this module (`_core.workspace(...)`) and never
bind them by from-import: tests swap them HERE (tests/guard_alloc.py the workspace, tests/test_norm_kernels_host.py the tensor check) and
every wrapper has to see the swap.

Two generations of argument rules live side by side, and which one a wrapper uses decides the exception it raises: the training step's
wrappers and the older inference helpers go through `_check` / `ld_of` / `volume` (RuntimeError off the GPU or for a dtype other than
float32), everything newer through `dense` (ValueError throughout).
"""
import ctypes

import numpy as np
import torch

from .._lib import ERRORS, lib      # noqa: F401  (ops.lib, ops.ERRORS)

K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
ROLE_FWD, ROLE_BWD = 0, 1
FLAG_SIGMOID, FLAG_ACCUM = 1, 2
GN_SLAB, GN_CHANNEL = 0, 1

_workspaces = {}
_RANK = {3: '(D,H,W)', 4: '(D,H,W,C)', 5: '(N,D,H,W,C)'}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def workspace(nbytes, device):
    """one grow-only scratch buffer per device AND stream; all users of a buffer are ordered on that stream"""
    key = (device.type, device.index, torch.cuda.current_stream().cuda_stream if device.type == 'cuda' else 0)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def scratch(query, device, *dims, optional=False):
    """-> (the workspace the size query `query(*dims)` asks for, its bytes); optional: None where the query asks for no bytes"""
    nb = lib().query(query, *dims)
    return (workspace(nb, device) if nb > 0 or not optional else None), nb


def _check(t, name='tensor'):
    if not t.is_cuda:
        raise RuntimeError('%s must live on the GPU (no CPU fallback exists for the product path)' % name)
    if t.dtype != torch.float32:
        raise RuntimeError('%s must be float32' % name)


def ld_of(t):
    """voxel stride of an NDHWC view (validates that the view is a channel slice of a dense NDHWC buffer)"""
    _check(t)
    if t.dim() != 5 or t.stride(4) != 1 and t.shape[4] != 1:
        raise RuntimeError('expected an [N,D,H,W,C] tensor with unit channel stride, got strides %s' % (t.stride(),))
    n, d, h, w, c = t.shape
    ld = t.stride(3)
    if w == 1:
        ld = t.stride(2) if h > 1 else (t.stride(1) if d > 1 else (t.stride(0) if n > 1 else c))
    exp = (d * h * w * ld, h * w * ld, w * ld, ld)
    for i in range(4):
        if t.shape[i] > 1 and t.stride(i) != exp[i]:
            raise RuntimeError('tensor is not a channel slice of a dense NDHWC buffer: strides %s' % (t.stride(),))
    if ld < c:
        raise RuntimeError('bad voxel stride')
    return ld


def nvc(t):
    """(N, voxels of one item, C) of an [N,D,H,W,C] tensor"""
    return t.shape[0], t.shape[1] * t.shape[2] * t.shape[3], t.shape[4]


def dense(t, dtype, name, rank=None, shape=None, numel=None):
    """THE tensor rule: `t` is a dense tensor of `dtype` on the GPU -- of `rank` dimensions, of exactly `shape`, of `numel` elements where
    those are given -> t, ValueError otherwise.  name: 'wrapper: argument', the head of the message"""
    what = str(dtype).replace('torch.', '')
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise ValueError('%s must be a dense %s tensor on the GPU' % (name, what))
    if rank is not None and t.dim() != rank:
        raise ValueError('%s must have shape %s, got %s' % (name, _RANK[rank], tuple(t.shape)))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError('%s must be a dense %s tensor of shape %s, got %s' % (name, what, tuple(shape), tuple(t.shape)))
    if numel is not None and t.numel() != numel:
        raise ValueError('%s must hold %d %s values, got %d' % (name, numel, what, t.numel()))
    return t


def volume(t, name, rank=4, shape=None):
    """the older rule for a dense float32 (D,H,W,C) volume (or a batch of `rank` 5): RuntimeError off the GPU or for another dtype, as
    `_check` raises it, then `dense`"""
    _check(t, name)
    return dense(t, torch.float32, name, rank=rank, shape=shape)


def out_or_new(out, shape, dtype, device, name, numel=None, zero=False, rule=dense):
    """THE output rule: out None -> a new tensor of `shape` (zeroed with zero=True: a count that is added into); else the caller's, which
    must be dense, of `dtype`, on the GPU and of `shape` -- or, where `numel` is given, of that many elements in any shape.  rule=volume
    for the wrappers whose device and dtype failures are RuntimeError"""
    if out is None:
        return (torch.zeros if zero else torch.empty)(tuple(shape), dtype=dtype, device=device)
    if rule is volume:
        return volume(out, name, rank=len(shape), shape=shape)
    return dense(out, dtype, name, shape=None if numel is not None else shape, numel=numel)


def carray(ctype, values, size=None):
    """a host sequence of numbers -> the pointer the ABI takes to a C array of `ctype` holding them (the pointer keeps the array alive).
    size: the elements the library will read where the caller has not checked the sequence's length: fewer values are padded with zeros,
    more are an IndexError"""
    conv = float if ctype in (ctypes.c_float, ctypes.c_double) else int
    values = [conv(v) for v in values]
    return ctypes.cast((ctype * max(len(values) if size is None else size, 1))(*values), ctypes.c_void_p)


def matrix12(matrices, name, most=None):
    """a finite 3x4 or 4x4 float64 matrix -- with `most`, a stack of 1..most of them -> (their top three rows as a C array of 12 doubles
    each, their number)"""
    try:
        m = np.asarray(matrices, dtype=np.float64)
    except (TypeError, ValueError):
        if most is None:      # (affine_resample3d has always let numpy's own error out)
            raise
        m = np.zeros(0)
    if most is None:
        m = m[None] if m.ndim == 2 else np.zeros(0)
    if m.ndim == 3 and m.shape[1:] == (4, 4):
        m = m[:, :3]
    if m.ndim != 3 or m.shape[1:] != (3, 4) or not 1 <= m.shape[0] <= (most or 1) or not np.all(np.isfinite(m)):
        raise ValueError('%s must be %s, got %r' % (name, 'a finite 3x4 or 4x4 array' if most is None else
                                                   '1..%d finite 3x4 or 4x4 arrays' % most, matrices))
    return (ctypes.c_double * m.size)(*[float(v) for v in m.reshape(-1)]), m.shape[0]


def int3(v, name, who):
    try:
        out = tuple(int(t) for t in v)
        ok = len(out) == 3 and all(float(t) == int(t) for t in v)
    except (TypeError, ValueError):
        out, ok = (), False
    if not ok:
        raise ValueError('%s: %s must be three integers, got %r' % (who, name, v))
    return out


def grid(who, out_shape, pad_to, order):
    """the target of zoom3d and affine_resample3d: order 0 | 1 | 3 and a positive extent out_shape inside pad_to (None: out_shape itself)
    -> (do, ho, wo), (dp, hp, wp)"""
    if order not in (0, 1, 3):
        raise ValueError('%s: order must be 0, 1 or 3, got %r' % (who, order))
    do, ho, wo = (int(v) for v in out_shape)
    dp, hp, wp = (do, ho, wo) if pad_to is None else (int(v) for v in pad_to)
    if min(do, ho, wo) < 1 or dp < do or hp < ho or wp < wo:
        raise ValueError('%s: out_shape %s must be positive and within pad_to %s' % (who, (do, ho, wo), (dp, hp, wp)))
    return (do, ho, wo), (dp, hp, wp)


def bin_count(bins, most, who):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= most:
        raise ValueError('%s: bins must be an integer in 2..%d, got %r' % (who, most, bins))
    return int(bins)
