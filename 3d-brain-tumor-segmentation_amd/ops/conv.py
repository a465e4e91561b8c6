"""The fp32 convolution engine (csrc/conv_engine.hip, conv_wgrad_engine.hip, conv_pack.hip): packed kernel images, forward, data and weight
gradient."""
import ctypes
import weakref

import torch

from . import _core


def conv_kind_taps(kind):
    return 1 if kind == _core.K1 else 27


def conv_pack(kind, role, w, cin_ref, cout, cin_slab=None, dup_start=0, dup_shift=0):
    """reference-layout kernel -> packed image for the implicit-GEMM kernel"""
    _core._check(w, 'kernel')
    cin_slab = cin_ref if cin_slab is None else cin_slab
    n = _core.lib().query('bts_conv_packed_floats', kind, role, cin_slab, cout)
    wp = torch.empty(n, dtype=torch.float32, device=w.device)
    wc = w.contiguous()
    _core.lib().call('bts_conv_pack', kind, role, _core._p(wc), _core._p(wp), cin_ref, cout, cin_slab, dup_start, dup_shift, _core._stream())
    if wc is not w:      # packed from a temporary copy: the library must not re-pack a form on demand from that address later
        _core.lib()._bts_conv_pack_forget(_core._p(wp))
    else:                # the library keys its record of the image by address: drop it with the tensor
        fin = weakref.finalize(wp, _forget_image, wp.data_ptr())
        fin.atexit = False
    return wp


def _forget_image(ptr):
    try:
        _core.lib()._bts_conv_pack_forget(ctypes.c_void_p(ptr))
    except Exception:      # (interpreter shutdown)
        pass


class PackTable(object):
    """Device-resident descriptor table for bts_conv_pack_batch: entries = [(kind, role, w, wp, cin_ref, cout, cin_slab,
    dup_start, dup_shift)] with torch tensors w (reference layout) / wp (packed image).  Rebuilt only when a pointer or
    the entry list changes."""

    def __init__(self):
        self.key = None
        self.dev = None
        self.host = None
        self.n = 0
        self.blocks = 0

    def run(self, entries):
        if not entries:
            return
        # (+ the library's form-usage generation: images are re-packed in the forms their layers read; a table built before a new form
        # was first read is rebuilt here, once)
        key = (_core.lib().query('bts_conv_pack_generation'),) + tuple((e[0], e[1], e[2].data_ptr(), e[3].data_ptr()) + tuple(e[4:]) for e in entries)
        if key != self.key:
            L = _core.lib()
            nb = L._bts_conv_pack_desc_bytes()
            host = (ctypes.c_char * (nb * len(entries)))()
            first = 0
            for i, (kind, role, w, wp, cin_ref, cout, cin_slab, dup_start, dup_shift) in enumerate(entries):
                _core._check(w, 'kernel')
                _core._check(wp, 'packed image')
                if not w.is_contiguous():
                    raise ValueError('conv_pack_batch: kernels must be contiguous')
                r = L._bts_conv_pack_desc(ctypes.cast(host, ctypes.c_void_p), i, first, kind, role, _core._p(w), _core._p(wp), cin_ref,
                                          cout, cin_slab, dup_start, dup_shift)
                if r <= 0:
                    raise RuntimeError('bts_conv_pack_desc failed: %s' % _core.ERRORS.get(r, r))
                first += r
            dev = entries[0][3].device
            self.dev = torch.frombuffer(bytearray(host), dtype=torch.uint8).to(dev)
            self.host = host      # (kept: the library reads each entry's forms from the host copy of the table it is asked to run)
            self.key, self.n, self.blocks = key, len(entries), first
        _core.lib().call('bts_conv_pack_batch', _core._p(self.dev), ctypes.cast(self.host, ctypes.c_void_p), self.n, self.blocks, _core._stream())


def conv_packed_empty(kind, role, cin_slab, cout, device):
    return torch.empty(_core.lib().query('bts_conv_packed_floats', kind, role, cin_slab, cout), dtype=torch.float32, device=device)


def conv_out_shape(kind, x_shape, cout):
    n, d, h, w, _ = x_shape
    if kind == _core.K3S2:
        return (n, d // 2, h // 2, w // 2, cout)
    if kind == _core.K3S2T:
        return (n, 2 * d, 2 * h, 2 * w, cout)
    return (n, d, h, w, cout)


def conv_fwd(kind, x, wp, bias, cout, out=None, sigmoid=False):
    n, d, h, w, cin = x.shape
    if out is None:
        out = torch.empty(conv_out_shape(kind, x.shape, cout), dtype=torch.float32, device=x.device)
    ws, nb = _core.scratch('bts_conv3d_fwd_workspace', x.device, kind, n, d, h, w, cin, cout, optional=True)
    _core.lib().call('bts_conv3d_fwd', kind, _core._p(x), _core._p(wp), _core._p(bias), _core._p(out), _core._p(ws), nb, n, d, h, w, cin,
                     _core.ld_of(x), cout, _core.ld_of(out), _core.FLAG_SIGMOID if sigmoid else 0, _core._stream())
    return out


def conv_fwd_fused2(x, wp3, bias3, wp1, bias1, cout):
    """(c1, res) = (conv3x3x3(x)+bias3, conv1x1x1(x)+bias1) from one pass over x, or None when the selected tiling cannot
    hold the second accumulator set (the caller then launches the two convolutions separately)"""
    n, d, h, w, cin = x.shape
    if not _core.lib()._bts_conv3d_fwd_can_fuse(n, d, h, w, cin, cout):
        return None
    c1 = torch.empty((n, d, h, w, cout), dtype=torch.float32, device=x.device)
    res = torch.empty_like(c1)
    _core.lib().call('bts_conv3d_fwd_fused2', _core._p(x), _core._p(wp3), _core._p(bias3), _core._p(c1), _core._p(wp1), _core._p(bias1),
                     _core._p(res), n, d, h, w, cin, _core.ld_of(x), cout, cout, cout, _core._stream())
    return c1, res


def conv_fwd_gn(kind, x, wp, bias, cout, groups, eps):
    """(y, mean, rstd): y = conv(x) + bias (dense) and the slab-mode GroupNorm statistics of y, in one pass where the
    tiled kernel can emit them from its epilogue (the library falls back to bts_gn_stats otherwise)"""
    n, d, h, w, cin = x.shape
    y = torch.empty(conv_out_shape(kind, x.shape, cout), dtype=torch.float32, device=x.device)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    ws, nb = _core.scratch('bts_conv3d_fwd_gn_workspace', x.device, kind, n, d, h, w, cin, cout, groups)
    _core.lib().call('bts_conv3d_fwd_gn', kind, _core._p(x), _core._p(wp), _core._p(bias), _core._p(y), _core._p(ws), nb, n, d, h, w, cin,
                     _core.ld_of(x), cout, groups, float(eps), _core._p(mean), _core._p(rstd), _core._stream())
    return y, mean, rstd


def conv_fwd_fused2_gn(x, wp3, bias3, wp1, bias1, cout, groups, eps):
    """conv_fwd_fused2 with the GroupNorm statistics of its 3x3x3 output: (c1, res, mean, rstd) or None"""
    n, d, h, w, cin = x.shape
    if not _core.lib()._bts_conv3d_fwd_can_fuse(n, d, h, w, cin, cout):
        return None
    c1 = torch.empty((n, d, h, w, cout), dtype=torch.float32, device=x.device)
    res = torch.empty_like(c1)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    ws, nb = _core.scratch('bts_conv3d_fwd_gn_workspace', x.device, _core.K3S1, n, d, h, w, cin, cout, groups)
    _core.lib().call('bts_conv3d_fwd_fused2_gn', _core._p(x), _core._p(wp3), _core._p(bias3), _core._p(c1), _core._p(wp1), _core._p(bias1),
                     _core._p(res), _core._p(ws), nb, n, d, h, w, cin, _core.ld_of(x), cout, cout, groups, float(eps), _core._p(mean), _core._p(rstd),
                     _core._stream())
    return c1, res, mean, rstd


def conv_bwd_data(kind, dy, wp_bwd, dx, accumulate):
    """dx: [N,D,H,W,Cin] view of the forward input's gradient"""
    n, d, h, w, cin = dx.shape
    cout = dy.shape[4]
    ws, nb = _core.scratch('bts_conv3d_bwd_data_workspace', dy.device, kind, n, d, h, w, cin, cout, optional=True)
    _core.lib().call('bts_conv3d_bwd_data', kind, _core._p(dy), _core._p(wp_bwd), _core._p(dx), _core._p(ws), nb, n, d, h, w, cin, _core.ld_of(dx),
                     cout, _core.ld_of(dy), _core.FLAG_ACCUM if accumulate else 0, _core._stream())
    return dx


def conv_bwd_data_pair(dy, wp_bwd, dy2, wp2_bwd, dx, accumulate):
    """dx (+)= bwd_data(3x3x3)(dy) + bwd_data(1x1x1)(dy2): both gradient paths into a ResNet block's input in one pass"""
    n, d, h, w, cin = dx.shape
    cout = dy.shape[4]
    ws, nb = _core.scratch('bts_conv3d_bwd_data_pair_workspace', dy.device, n, d, h, w, cin, cout, optional=True)
    _core.lib().call('bts_conv3d_bwd_data_pair', _core._p(dy), _core._p(wp_bwd), _core._p(dy2), _core._p(wp2_bwd), _core._p(dx), _core._p(ws), nb, n,
                     d, h, w, cin, _core.ld_of(dx), cout, _core.ld_of(dy), _core.ld_of(dy2), _core.FLAG_ACCUM if accumulate else 0, _core._stream())
    return dx


def conv_bwd_weight(kind, x, dy, dw, db, dup_start=0, dup_shift=0, accumulate=False):
    n, d, h, w, cin = x.shape
    cout = dy.shape[4]
    ws, nb = _core.scratch('bts_conv3d_bwd_weight_workspace', x.device, kind, n, d, h, w, cin, cout)
    _core.lib().call('bts_conv3d_bwd_weight', kind, _core._p(x), _core._p(dy), _core._p(dw), _core._p(db), _core._p(ws), nb, n, d, h, w, cin,
                     _core.ld_of(x), cout, _core.ld_of(dy), dup_start, dup_shift, 1 if accumulate else 0, _core._stream())


def _conv_bwd_weight_query(name, kind, x, dy):
    n, d, h, w, cin = x.shape
    aligned = (1 if x.data_ptr() % 16 == 0 else 0) | (2 if dy.data_ptr() % 16 == 0 else 0)
    return _core.lib().probe(name, kind, n, d, h, w, cin, _core.ld_of(x), dy.shape[4], _core.ld_of(dy), aligned)


def conv_bwd_weight_form(kind, x, dy):
    """the form conv_bwd_weight takes for these operands (host-only query): 3 Winograd over all axes | 0 every other kernel"""
    return _conv_bwd_weight_query('bts_conv3d_bwd_weight_form', kind, x, dy)


def conv_bwd_weight_kernel(kind, x, dy):
    """the profile symbol of the kernel conv_bwd_weight runs for these operands (host-only query): 100 | 104 | 109 | 110 the direct kernel's
    variants, 24 wgw_kernel, 26 k1w_kernel"""
    return _conv_bwd_weight_query('bts_conv3d_bwd_weight_kernel', kind, x, dy)
