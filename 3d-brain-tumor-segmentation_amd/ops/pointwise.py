"""Element-wise kernels, the dense layer and the 2x samplers of the fp32 step (csrc/pointwise.hip, dense.hip)."""
import torch

from . import _core


def dropout_mask(shape, rate, seed, device):
    m = torch.empty(shape, dtype=torch.uint8, device=device)
    _core.lib().call('bts_dropout_mask', _core._p(m), m.numel(), float(rate), int(seed) & (2 ** 64 - 1), _core._stream())
    return m


def dropout_apply(x, mask, rate):
    y = torch.empty_like(x)
    _core.lib().call('bts_dropout_apply', _core._p(x), _core._p(mask), _core._p(y), x.numel(), float(rate), _core._stream())
    return y


def normal(shape, seed, device):
    out = torch.empty(shape, dtype=torch.float32, device=device)
    _core.lib().call('bts_normal', _core._p(out), out.numel(), int(seed) & (2 ** 64 - 1), _core._stream())
    return out


def vae_sample_fwd(proj, eps):
    n, l2 = proj.shape
    z = torch.empty((n, l2 // 2), dtype=torch.float32, device=proj.device)
    _core.lib().call('bts_vae_sample_fwd', _core._p(proj), _core._p(eps), _core._p(z), n, l2 // 2, _core._stream())
    return z


def vae_sample_bwd(proj, eps, dz, dproj):
    n, l2 = proj.shape
    _core.lib().call('bts_vae_sample_bwd', _core._p(proj), _core._p(eps), _core._p(dz), _core._p(dproj), n, l2 // 2, _core._stream())


def fill(t, v):
    _core.lib().call('bts_fill', _core._p(t), t.numel(), float(v), _core._stream())
    return t


def axpy(y, x, a=1.0):
    _core.lib().call('bts_axpy', _core._p(y), _core._p(x), y.numel(), float(a), _core._stream())


def add_strided(dst, src, accumulate):
    """dst[..., :C] (+)= src[..., :C] for NDHWC channel-slice views"""
    c = src.shape[-1]
    rows = src.numel() // c
    ldd = _core.ld_of(dst) if dst.dim() == 5 else dst.stride(-2)
    lds = _core.ld_of(src) if src.dim() == 5 else src.stride(-2)
    _core.lib().call('bts_add_strided', _core._p(dst), _core._p(src), rows, c, ldd, lds, 1 if accumulate else 0, _core._stream())


def scalar_lincomb(a, b, ca=1.0, cb=1.0):
    out = torch.empty(1, dtype=torch.float32, device=a.device)
    _core.lib().call('bts_scalar_lincomb', _core._p(out), _core._p(a), _core._p(b), float(ca), float(cb), _core._stream())
    return out


def relu_bwd(y, dy):
    dx = torch.empty_like(y)
    _core.lib().call('bts_relu_bwd', _core._p(y), _core._p(dy), _core._p(dx), y.numel(), _core._stream())
    return dx


def sigmoid_bwd(y, dy):
    c = y.shape[-1]
    rows = y.numel() // c
    dx = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    _core.lib().call('bts_sigmoid_bwd', _core._p(y), _core._p(dy), _core._p(dx), rows, c, _core.ld_of(y), _core.ld_of(dy), _core._stream())
    return dx


def dense_fwd(x, w, b, relu):
    n, fin = x.shape
    fout = w.shape[1]
    ws, nb = _core.scratch('bts_dense_workspace', x.device, n, fin, fout)
    y = torch.empty((n, fout), dtype=torch.float32, device=x.device)
    _core.lib().call('bts_dense_fwd', _core._p(x), _core._p(w), _core._p(b), _core._p(y), _core._p(ws), nb, n, fin, fout, 1 if relu else 0,
                     _core._stream())
    return y


def dense_bwd(x, w, g, dx, dw, db, accumulate_dx=False, accumulate_params=False):
    n, fin = x.shape
    fout = w.shape[1]
    _core.lib().call('bts_dense_bwd', _core._p(x), _core._p(w), _core._p(g), _core._p(dx), _core._p(dw), _core._p(db), n, fin, fout,
                     1 if accumulate_dx else 0, 1 if accumulate_params else 0, _core._stream())


# ---- non-default samplers ----
def maxpool2_fwd(x):
    n, d, h, w, c = x.shape
    y = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    idx = torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8, device=x.device)
    _core.lib().call('bts_maxpool2_fwd', _core._p(x), _core._p(y), _core._p(idx), n, d, h, w, c, _core.ld_of(x), c, _core._stream())
    return y, idx


def maxpool2_bwd(dy, idx, dx, accumulate):
    """dx: [N,D,H,W,C] view of the input's gradient (may be a slab slice)"""
    n, d, h, w, c = dx.shape
    _core.lib().call('bts_maxpool2_bwd', _core._p(dy), _core._p(idx), _core._p(dx), n, d, h, w, c, _core.ld_of(dy), _core.ld_of(dx),
                     1 if accumulate else 0, _core._stream())
    return dx


def upsample2_fwd(x, out=None):
    n, d, h, w, c = x.shape
    if out is None:
        out = torch.empty((n, 2 * d, 2 * h, 2 * w, c), dtype=torch.float32, device=x.device)
    _core.lib().call('bts_upsample2_fwd', _core._p(x), _core._p(out), n, d, h, w, c, _core.ld_of(x), _core.ld_of(out), _core._stream())
    return out


def upsample2_bwd(dy, dx=None, accumulate=False):
    n, d2, h2, w2, c = dy.shape
    if dx is None:
        dx = torch.empty((n, d2 // 2, h2 // 2, w2 // 2, c), dtype=torch.float32, device=dy.device)
    _core.lib().call('bts_upsample2_bwd', _core._p(dy), _core._p(dx), n, d2 // 2, h2 // 2, w2 // 2, c, _core.ld_of(dy), _core.ld_of(dx),
                     1 if accumulate else 0, _core._stream())
    return dx
