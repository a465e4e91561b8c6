"""Loss, metric, regulariser and optimiser kernels of the fp32 step (csrc/loss.hip, loss_ce.hip, optim.hip)."""
import ctypes

import torch

from . import _core


def loss_sums(y_pred, y, x, y_vae, proj):
    """-> sums (3C+4,) float64 device tensor (see include/bts_hip.h)"""
    n, v, c = _core.nvc(y_pred)
    sums = torch.empty(3 * c + 4, dtype=torch.float64, device=y_pred.device)
    ws, nb = _core.scratch('bts_loss_workspace', y_pred.device)
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    _core.lib().call('bts_loss_sums', _core._p(y_pred), _core._p(y), _core._p(x), _core._p(y_vae), _core._p(proj), _core._p(sums), _core._p(ws), nb,
                     n, v, c, _core.ld_of(y_pred), _core.ld_of(y), cx, _core.ld_of(x) if has_vae else 0, _core.ld_of(y_vae) if has_vae else 0, lz,
                     _core._stream())
    return sums


def loss_value(sums, c, has_vae=True):
    loss = torch.empty(1, dtype=torch.float32, device=sums.device)
    parts = torch.empty(3, dtype=torch.float32, device=sums.device)
    _core.lib().call('bts_loss_value', _core._p(sums), _core._p(loss), _core._p(parts), c, 1 if has_vae else 0, _core._stream())
    return loss, parts


def loss_bwd(y_pred, y, x, y_vae, proj, sums, gscale, dypred, dyvae, dproj, through_sigmoid=False):
    n, v, c = _core.nvc(y_pred)
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    _core.lib().call('bts_loss_bwd', _core._p(y_pred), _core._p(y), _core._p(x), _core._p(y_vae), _core._p(proj), _core._p(sums), _core._p(gscale),
                     _core._p(dypred), _core._p(dyvae), _core._p(dproj), n, v, c, _core.ld_of(y_pred), _core.ld_of(y), cx,
                     _core.ld_of(x) if has_vae else 0, _core.ld_of(y_vae) if has_vae else 0, lz, 1 if through_sigmoid else 0, _core._stream())


def _seg_loss_dims(y_pred, x, y_vae, proj):
    """(N, V, C of the prediction; C and voxel strides of the VAE pair, latent size) -- zeros without a VAE branch"""
    n, v, c = _core.nvc(y_pred)
    has_vae = x is not None
    cx = x.shape[4] if has_vae else 0
    lz = proj.shape[1] // 2 if proj is not None else 0
    return n, v, c, cx, _core.ld_of(x) if has_vae else 0, _core.ld_of(y_vae) if has_vae else 0, lz


def seg_loss_sums(y_pred, y, x, y_vae, proj, gamma=0.0, w_pos=1.0, w_neg=1.0):
    """the compound loss's raw sums in one pass -> (4C+5,) float64 device tensor: loss_sums' 3C+4, the cross-entropy / focal sums per
    channel, this shard's N*V (see include/bts_hip.h)"""
    n, v, c, cx, ldx, ldv, lz = _seg_loss_dims(y_pred, x, y_vae, proj)
    sums = torch.empty(4 * c + 5, dtype=torch.float64, device=y_pred.device)
    ws, nb = _core.scratch('bts_seg_loss_workspace', y_pred.device)
    _core.lib().call('bts_seg_loss_sums', _core._p(y_pred), _core._p(y), _core._p(x), _core._p(y_vae), _core._p(proj), _core._p(sums), _core._p(ws),
                     nb, n, v, c, _core.ld_of(y_pred), _core.ld_of(y), cx, ldx, ldv, lz, gamma, w_pos, w_neg, _core._stream())
    return sums


def seg_loss_value(sums, c, has_vae=True, w_dice=1.0, w_ce=1.0):
    """-> loss (1,), parts (4,) = dice, l2, kl, cross-entropy"""
    loss = torch.empty(1, dtype=torch.float32, device=sums.device)
    parts = torch.empty(4, dtype=torch.float32, device=sums.device)
    _core.lib().call('bts_seg_loss_value', _core._p(sums), _core._p(loss), _core._p(parts), c, 1 if has_vae else 0, w_dice, w_ce, _core._stream())
    return loss, parts


def seg_loss_bwd(y_pred, y, x, y_vae, proj, sums, gscale, dypred, dyvae, dproj, through_sigmoid=False, w_dice=1.0, w_ce=1.0,
                 gamma=0.0, w_pos=1.0, w_neg=1.0):
    n, v, c, cx, ldx, ldv, lz = _seg_loss_dims(y_pred, x, y_vae, proj)
    _core.lib().call('bts_seg_loss_bwd', _core._p(y_pred), _core._p(y), _core._p(x), _core._p(y_vae), _core._p(proj), _core._p(sums),
                     _core._p(gscale), _core._p(dypred), _core._p(dyvae), _core._p(dproj), n, v, c, _core.ld_of(y_pred), _core.ld_of(y), cx, ldx, ldv,
                     lz, 1 if through_sigmoid else 0, w_dice, w_ce, gamma, w_pos, w_neg, _core._stream())


def dice_metric_sums(y_true, y_pred, channels_last_axes=True, want_labels=True):
    n, d, h, w, c = y_pred.shape
    cells = w if channels_last_axes else 1
    table = torch.empty(cells * c * 3, dtype=torch.float64, device=y_pred.device)
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=y_pred.device) if want_labels else None
    _core.lib().call('bts_dice_metric_sums', _core._p(y_true), _core._p(y_pred), _core._p(labels), _core._p(table), n, d * h * w, w, c,
                     _core.ld_of(y_true), _core.ld_of(y_pred), 1 if channels_last_axes else 0, _core._stream())
    return table, labels


def dice_metric_value(table, w, c, channels_last_axes=True):
    out = torch.empty(2, dtype=torch.float32, device=table.device)
    _core.lib().call('bts_dice_metric_value', _core._p(table), _core._p(out), w, c, 1 if channels_last_axes else 0, _core._stream())
    return out


def _ranges(ranges):
    """[(offset, length, coefficient)] -> the three host arrays and their length (built without _core.carray: up to 128 ranges twice a
    step, already ints and floats, and its per-element conversion would be host time in every training step)"""
    nr, as_p = len(ranges), lambda a: ctypes.cast(a, ctypes.c_void_p)
    return (as_p((ctypes.c_long * max(nr, 1))(*[r[0] for r in ranges])), as_p((ctypes.c_long * max(nr, 1))(*[r[1] for r in ranges])),
            as_p((ctypes.c_float * max(nr, 1))(*[r[2] for r in ranges])), nr)


def l2_reg_fwd(params_flat, ranges):
    """ranges: [(offset, length, coefficient)] (<= 128) into the flat parameter buffer"""
    off, ln, cf, nr = _ranges(ranges)
    out = torch.empty(1, dtype=torch.float32, device=params_flat.device)
    ws, nb = _core.scratch('bts_l2_workspace', params_flat.device)
    _core.lib().call('bts_l2_reg_fwd', _core._p(params_flat), off, ln, cf, nr, _core._p(out), _core._p(ws), nb, _core._stream())
    return out


def l2_reg_bwd(params_flat, grads_flat, ranges, gscale=None):
    off, ln, cf, nr = _ranges(ranges)
    _core.lib().call('bts_l2_reg_bwd', _core._p(params_flat), _core._p(grads_flat), off, ln, cf, nr, _core._p(gscale), _core._stream())


def adam_tf_step(p, g, m, v, lr_t, beta1, beta2, eps, gmul=1.0, skip=None):
    """skip: device int32[1]; the whole update is dropped on the device when it is non-zero (grad_nonfinite below)"""
    if skip is not None:
        _core.lib().call('bts_adam_tf_step_guarded', _core._p(p), _core._p(g), _core._p(m), _core._p(v), p.numel(), float(lr_t), float(beta1),
                         float(beta2), float(eps), float(gmul), _core._p(skip), _core._stream())
        return
    _core.lib().call('bts_adam_tf_step', _core._p(p), _core._p(g), _core._p(m), _core._p(v), p.numel(), float(lr_t), float(beta1), float(beta2),
                     float(eps), float(gmul), _core._stream())


def grad_nonfinite(g, flag):
    """flag[0] (device int32) = 1 iff any element of the flat fp32 gradient is Inf / NaN"""
    _core.lib().call('bts_grad_nonfinite', _core._p(g), g.numel(), _core._p(flag), _core._stream())
