"""The nested BraTS regions WT, TC, ET as training targets and as the decoded prediction (csrc/regions.hip)."""
import torch

from . import _core


REGION_CHANNELS = 3


def _region_channels(c, who):
    if int(c) != REGION_CHANNELS:
        raise ValueError('%s: the BraTS regions (WT, TC, ET) are three channels, got %d' % (who, int(c)))


def region_targets(y, channels_first=False):
    """the label batch an augment launch wrote (one-hot minus the background), IN PLACE (-> y): (l1, l2, l3) -> the nested regions
    (l1 + l2 + l3, l1 + l3, l3) = (WT, TC, ET).  y: dense fp32 (N, ..., 3), or (N, 3, ...) with channels_first; a view into a larger
    buffer is fine"""
    _core.dense(y, torch.float32, 'region_targets: y')
    if y.dim() < (3 if channels_first else 2):
        raise ValueError('region_targets: y must be (N, ..., 3), or (N, 3, ...) with channels_first, got shape %s' % (tuple(y.shape),))
    c = y.shape[1] if channels_first else y.shape[-1]
    _region_channels(c, 'region_targets')
    n = y.shape[0]
    if y.numel() == 0:
        raise ValueError('region_targets: y is empty, shape %s' % (tuple(y.shape),))
    _core.lib().call('bts_region_targets', _core._p(y), n, y.numel() // (n * c), c, 1 if channels_first else 0, _core._stream())
    return y


def region_dice_sums(y_true, y_pred, want_labels=True):
    """y_true, y_pred: (N,D,H,W,3) channel slices of dense NDHWC buffers, channels (WT, TC, ET) -> (table (9,) float64: (I, P, T) per
    region, counted exactly with p > 0.5 and t > 0.5 -- what dice_metric_value(table, w, 3, False) reduces; labels (N,D,H,W) uint8:
    the decode of region_finish with p > 0.5, coded 0, 1, 2, 3 (ET) like dice_metric_sums' map, or None)"""
    if y_true.dim() != 5 or tuple(y_true.shape) != tuple(y_pred.shape):
        raise ValueError('region_dice_sums: y_true and y_pred must be (N,D,H,W,3) tensors of one shape, got %s and %s' %
                         (tuple(y_true.shape), tuple(y_pred.shape)))
    n, d, h, w, c = y_pred.shape
    _region_channels(c, 'region_dice_sums')
    ldt, ldp = _core.ld_of(y_true), _core.ld_of(y_pred)
    table = torch.empty(3 * c, dtype=torch.float64, device=y_pred.device)
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=y_pred.device) if want_labels else None
    _core.lib().call('bts_region_dice_sums', _core._p(y_true), _core._p(y_pred), _core._p(labels), _core._p(table), n * d * h * w, c, ldt, ldp,
                     _core._stream())
    return table, labels


def region_finish(prob, bmask, threshold=0.5, want_probabilities=True, want_labels=True):
    """tta_finish for a network trained on the regions: prob (N,D,H,W,3) = (WT, TC, ET), bmask one float per voxel
    -> (prob * bmask, uint8 label map (N,D,H,W)): 4 where et >= threshold, else 1 where tc >= threshold, else 2 where wt >= threshold,
    else 0 (the masked probabilities; the overwrite rule, not the nested one), 0 where masked out"""
    _core._check(prob, 'prob'), _core._check(bmask, 'bmask')
    if prob.dim() != 5:
        raise ValueError('region_finish: prob must be (N,D,H,W,3), got shape %s' % (tuple(prob.shape),))
    n, d, h, w, c = prob.shape
    _region_channels(c, 'region_finish')
    if bmask.numel() != n * d * h * w:
        raise ValueError('region_finish: bmask holds %d values, prob %d voxels' % (bmask.numel(), n * d * h * w))
    y = torch.empty(tuple(prob.shape), dtype=torch.float32, device=prob.device) if want_probabilities else None
    labels = torch.empty((n, d, h, w), dtype=torch.uint8, device=prob.device) if want_labels else None
    _core.lib().call('bts_region_finish', _core._p(prob.contiguous()), _core._p(bmask.contiguous()), _core._p(y), _core._p(labels), n * d * h * w, c,
                     float(threshold), _core._stream())
    return y, labels
