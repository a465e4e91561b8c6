"""GroupNorm, column sums, the squeeze-excitation gate and the fused block epilogue / backward of the fp32 step (csrc/groupnorm.hip, se.hip,
block_bwd.hip)."""
import torch

from . import _core


def gn_stats(x, groups, mode, eps=1e-5):
    """x dense [N,D,H,W,C] -> (mean, rstd) each (N*G,)"""
    if not x.is_contiguous():
        raise RuntimeError('GroupNormalization statistics need a dense tensor')
    n, v, c = _core.nvc(x)
    ws, nb = _core.scratch('bts_gn_workspace', x.device, n, v, c, groups, mode)
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    _core.lib().call('bts_gn_stats', _core._p(x), _core._p(mean), _core._p(rstd), _core._p(ws), nb, n, v, c, groups, mode, eps, _core._stream())
    return mean, rstd


def gn_apply(x, gamma, beta, mean, rstd, groups, mode, relu, out=None):
    n, v, c = _core.nvc(x)
    if out is None:
        out = torch.empty_like(x)
    _core.lib().call('bts_gn_apply', _core._p(x), _core._p(out), _core._p(gamma), _core._p(beta), _core._p(mean), _core._p(rstd), n, v, c,
                     _core.ld_of(out), groups, mode, 1 if relu else 0, _core._stream())
    return out


def gn_bwd(x, dy, gamma, beta, mean, rstd, dgamma, dbeta, groups, mode, relu, accumulate_params=False):
    n, v, c = _core.nvc(x)
    ws, nb = _core.scratch('bts_gn_bwd_workspace', x.device, n, v, c, groups, mode)
    dx = torch.empty_like(x)
    _core.lib().call('bts_gn_bwd', _core._p(x), _core._p(dy), _core._p(dx), _core._p(gamma), _core._p(beta), _core._p(mean), _core._p(rstd),
                     _core._p(dgamma), _core._p(dbeta), _core._p(ws), nb, n, v, c, _core.ld_of(dy), groups, mode, 1 if relu else 0,
                     1 if accumulate_params else 0, _core._stream())
    return dx


def colsum(x, scale=1.0, sum_over_n=False, out=None, accumulate=False):
    """x [N,...,C] (channel slice allowed) -> [N,C] (or [C]) column sums * scale"""
    n, c = x.shape[0], x.shape[-1]
    rows = x.numel() // (n * c)
    ld = _core.ld_of(x) if x.dim() == 5 else x.stride(-2)
    ws, nb = _core.scratch('bts_colsum_workspace', x.device, n, rows, c)
    if out is None:
        out = torch.empty((c,) if sum_over_n else (n, c), dtype=torch.float32, device=x.device)
    _core.lib().call('bts_colsum', _core._p(x), _core._p(out), _core._p(ws), nb, n, rows, c, ld, float(scale), 1 if sum_over_n else 0,
                     1 if accumulate else 0, _core._stream())
    return out


def se_mlp_fwd(gap, w1, w2):
    n, f = gap.shape
    r = w1.shape[1]
    h = torch.empty((n, r), dtype=torch.float32, device=gap.device)
    ch = torch.empty((n, f), dtype=torch.float32, device=gap.device)
    _core.lib().call('bts_se_mlp_fwd', _core._p(gap), _core._p(w1), _core._p(w2), _core._p(h), _core._p(ch), n, f, r, _core._stream())
    return h, ch


def block_epilogue_fwd(res, c2, out, wsp, ch, gamma, beta, mean, rstd, groups, mode):
    n, v, f = _core.nvc(res)
    sp = torch.empty(n * v, dtype=torch.float32, device=res.device)
    _core.lib().call('bts_block_epilogue_fwd', _core._p(res), _core._p(c2), _core._p(out), _core._p(sp), _core._p(wsp), _core._p(ch), _core._p(gamma),
                     _core._p(beta), _core._p(mean), _core._p(rstd), n, v, f, _core.ld_of(out), groups, mode, _core._stream())
    return sp


def se_bwd(dout, res, sp, gap, h, ch, w1, w2, wsp, dw1, dw2, dwsp, accumulate_params=False):
    n, v, f = _core.nvc(res)
    r = w1.shape[1]
    ws, nb = _core.scratch('bts_se_bwd_workspace', res.device, n, v, f, r)
    dres = torch.empty_like(res)
    ds = torch.empty(n * v, dtype=torch.float32, device=res.device)
    dgap = torch.empty((n, f), dtype=torch.float32, device=res.device)
    _core.lib().call('bts_se_bwd', _core._p(dout), _core._p(res), _core._p(sp), _core._p(gap), _core._p(h), _core._p(ch), _core._p(w1), _core._p(w2),
                     _core._p(wsp), _core._p(dres), _core._p(ds), _core._p(dgap), _core._p(dw1), _core._p(dw2), _core._p(dwsp), _core._p(ws), nb, n,
                     v, f, r, _core.ld_of(dout), 1 if accumulate_params else 0, _core._stream())
    return dres


def block_bwd_takes(res, r, groups, dout, c2):
    """does the fused gate + GroupNorm-2 backward take this block?  Asked BEFORE the grad slots are claimed, so it checks everything
    block_bwd and bts_block_bwd check (tiling, row stride, contiguity, 16-byte alignment of the three streamed tensors): once this
    says yes, block_bwd does not decline."""
    n, v, f = _core.nvc(res)
    return (_core.lib().probe('bts_block_bwd_workspace', n, v, f, r, groups) >= 0 and _core.ld_of(dout) % 4 == 0 and res.is_contiguous()
            and c2.is_contiguous() and all(t.data_ptr() % 16 == 0 for t in (dout, res, c2)))


def block_bwd(dout, res, c2, sp, gap, h, ch, w1, w2, wsp, gamma, beta, mean, rstd, groups, dw1, dw2, dwsp, dgamma, dbeta,
              accumulate_gate_params=False, accumulate_norm_params=False):
    """gate backward + GroupNorm-2 backward (slab mode, ReLU) of a ResnetBlock in one pair of passes -> (dres, dc2), or None where
    the fused kernels do not take the shape (the caller runs se_bwd and gn_bwd)"""
    n, v, f = _core.nvc(res)
    r = w1.shape[1]
    nb = _core.lib().probe('bts_block_bwd_workspace', n, v, f, r, groups)      # (-1: outside the fused kernels' tiling, not an error)
    if not block_bwd_takes(res, r, groups, dout, c2):
        return None
    ws = _core.workspace(nb, res.device)
    dres = torch.empty_like(res)
    dc2 = torch.empty_like(c2)
    ds = torch.empty(n * v, dtype=torch.float32, device=res.device)
    dgap = torch.empty((n, f), dtype=torch.float32, device=res.device)
    _core.lib().call('bts_block_bwd', _core._p(dout), _core.ld_of(dout), _core._p(res), _core._p(c2), _core._p(sp), _core._p(gap), _core._p(h),
                     _core._p(ch), _core._p(w1), _core._p(w2), _core._p(wsp), _core._p(gamma), _core._p(beta), _core._p(mean), _core._p(rstd),
                     _core._p(dres), _core._p(dc2), _core._p(ds), _core._p(dgap), _core._p(dw1), _core._p(dw2), _core._p(dwsp), _core._p(dgamma),
                     _core._p(dbeta), _core._p(ws), nb, n, v, f, r, groups, 1 if accumulate_gate_params else 0, 1 if accumulate_norm_params else 0,
                     _core._stream())
    return dres, dc2
