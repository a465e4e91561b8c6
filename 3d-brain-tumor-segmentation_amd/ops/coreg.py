"""Rigid co-registration by mutual information (csrc/coreg.hip): bin numbers and joint histograms."""
import numpy as np
import torch

from . import _core


def quantize_bins(x, lo, hi, bins=32):
    """dense float32 device tensor -> uint8 tensor of its shape: clamp(floor((double(x) - lo) * bins / (hi - lo)), 0, bins - 1), evaluated
    in float64 (bts_quantize_bins); lo < hi finite, bins in 2..64"""
    bins = _core.bin_count(bins, 64, 'quantize_bins')
    if _core.dense(x, torch.float32, 'quantize_bins: x').numel() < 1:
        raise ValueError('quantize_bins: x must not be empty')
    try:
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError('quantize_bins: lo and hi must be numbers, got %r and %r' % (lo, hi))
    if not (np.isfinite(lo) and np.isfinite(hi) and hi > lo and np.isfinite(hi - lo)):
        raise ValueError('quantize_bins: lo < hi must be finite, got %r and %r' % (lo, hi))
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _core.lib().call('bts_quantize_bins', _core._p(x), _core._p(q), x.numel(), lo, hi, bins, _core._stream())
    return q


def joint_hist_pv(qf, qm, origin, stride, counts, matrices, bins=32):
    """K joint histograms by partial-volume interpolation (bts_joint_hist_pv): qf (Df,Hf,Wf) and qm (Dm,Hm,Wm) dense uint8 device volumes of
    bin numbers below `bins`; the lattice origin + l * stride, 0 <= l < counts, of the fixed grid; matrices (K,3,4) or (K,4,4) float64, fixed
    voxel -> moving voxel, 1 <= K <= 32 -> (K,bins,bins) int64 on the device, [k][fixed bin][moving bin]; every counted lattice point adds
    32768 to its candidate's histogram"""
    who = 'joint_hist_pv'
    bins = _core.bin_count(bins, 64, who)
    for t, name in ((qf, 'qf'), (qm, 'qm')):
        if not 1 <= _core.dense(t, torch.uint8, '%s: %s' % (who, name), rank=3).numel() < 2 ** 31:
            raise ValueError('%s: %s must hold 1 .. 2^31 - 1 voxels' % (who, name))
    if qf.device != qm.device:
        raise ValueError('%s: qf and qm live on different devices' % who)
    o, s, n = _core.int3(origin, 'origin', who), _core.int3(stride, 'stride', who), _core.int3(counts, 'counts', who)
    for a in range(3):
        if o[a] < 0 or s[a] < 1 or n[a] < 1 or o[a] + (n[a] - 1) * s[a] > qf.shape[a] - 1:
            raise ValueError('%s: the lattice origin %s stride %s counts %s does not lie inside the fixed extent %s'
                             % (who, o, s, n, tuple(qf.shape)))
    m12, k = _core.matrix12(matrices, who + ': matrices', most=32)
    hist = torch.empty((k, bins, bins), dtype=torch.int64, device=qf.device)
    _core.lib().call('bts_joint_hist_pv', _core._p(qf), qf.shape[0], qf.shape[1], qf.shape[2], _core._p(qm), qm.shape[0], qm.shape[1], qm.shape[2],
                     o[0], o[1], o[2], s[0], s[1], s[2], n[0], n[1], n[2], m12, k, bins, _core._p(hist), _core._stream())
    return hist
