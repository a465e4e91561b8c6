"""float64 restatement of sliding-window inference with blended windows, written from the definition and independent of the product
(nothing here imports bts_amd): the window plan, the normalised importance tables, and NumPy forms of the gather, the accumulate,
the occupancy count and a whole blended pass over any callable.  Flip bits are 4|2|1 = D|H|W."""
import math

import numpy as np


def axis_starts(S, R, overlap):
    """MONAI's rule: the last window is shifted back to end at the volume's end; a short volume gets one window at 0"""
    interval = max(1, int(R * (1 - overlap)))
    if S <= R:
        return [0]
    count = int(math.ceil((S - R) / float(interval))) + 1
    return [min(i * interval, S - R) for i in range(count)]


def importance(R, mode, sigma_scale=0.125):
    if mode == 'constant':
        return np.ones(R, dtype=np.float64)
    sigma = sigma_scale * R
    return np.array([math.exp(-((r - (R - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for r in range(R)], dtype=np.float64)


def axis_table(S, R, overlap, mode, sigma_scale=0.125):
    """-> (starts, n): n[i][r] = g(r) / sum_j g(start_i + r - start_j) over the windows j that hold the position, 0 beyond S"""
    starts = axis_starts(S, R, overlap)
    g = importance(R, mode, sigma_scale)
    n = np.zeros((len(starts), R), dtype=np.float64)
    for i, si in enumerate(starts):
        for r in range(R):
            p = si + r
            if p >= S:
                continue
            den = 0.0
            for sj in starts:
                if 0 <= p - sj < R:
                    den += g[p - sj]
            n[i, r] = g[r] / den
    return starts, n


def plan(shape, roi, overlap=0.5, mode='gaussian', sigma_scale=0.125):
    axes = [axis_table(S, R, overlap, mode, sigma_scale) for S, R in zip(shape, roi)]
    return [a[0] for a in axes], [a[1] for a in axes]


def axis_coverage(S, starts, R):
    """windows that hold each position of the axis"""
    return np.array([sum(1 for s in starts if 0 <= p - s < R) for p in range(S)])


def flip_axes(flip):
    return tuple(a for a, bit in ((0, 4), (1, 2), (2, 1)) if flip & bit)


def _flip(a, flip):
    ax = flip_axes(flip)
    return np.flip(a, ax) if ax else a


def gather_ref(x, roi, start, flip, mean, std):
    """x (D,H,W,C) -> (R0,R1,R2,C) float64: the window with zeros beyond the volume's end, normalised, then flipped"""
    x = np.asarray(x, dtype=np.float64)
    win = np.zeros(tuple(roi) + (x.shape[-1],), dtype=np.float64)
    n = [min(r, s - o) for r, s, o in zip(roi, x.shape[:3], start)]
    win[:n[0], :n[1], :n[2]] = x[start[0]:start[0] + n[0], start[1]:start[1] + n[1], start[2]:start[2] + n[2]]
    win = (win - np.asarray(mean, dtype=np.float64)) / np.asarray(std, dtype=np.float64)
    return _flip(win, flip)


def accumulate_ref(acc, pred, tables, start, flip, rows, scale):
    """acc (D,H,W,K) float64, IN PLACE += scale nz ny nx unflip(pred) on the part of the window inside the volume"""
    p = _flip(np.asarray(pred, dtype=np.float64), flip)
    roi = p.shape[:3]
    n = [min(r, s - o) for r, s, o in zip(roi, acc.shape[:3], start)]
    w = (np.asarray(tables[0], dtype=np.float64)[rows[0]][:, None, None] * np.asarray(tables[1], dtype=np.float64)[rows[1]][None, :, None]
         * np.asarray(tables[2], dtype=np.float64)[rows[2]][None, None, :])
    acc[start[0]:start[0] + n[0], start[1]:start[1] + n[1], start[2]:start[2] + n[2]] += \
        scale * (w[..., None] * p)[:n[0], :n[1], :n[2]]
    return acc


def occupancy_ref(mask, roi, starts):
    m = np.asarray(mask).reshape(np.asarray(mask).shape[:3]) > 0
    out = np.zeros(tuple(len(s) for s in starts), dtype=np.int64)
    for iz, z in enumerate(starts[0]):
        for iy, y in enumerate(starts[1]):
            for ix, x in enumerate(starts[2]):
                out[iz, iy, ix] = int(m[z:z + roi[0], y:y + roi[1], x:x + roi[2]].sum())
    return out


def sliding_ref(x, mask, predict, roi, flips, mean, std, overlap=0.5, mode='gaussian', sigma_scale=0.125, skip_empty=False):
    """x (D,H,W,C), mask (D,H,W,1); predict: (R0,R1,R2,C) float64 array -> (R0,R1,R2,K) array, called per window and flip
    -> mask * mean over the flips of the blended, un-flipped predictions, float64 (D,H,W,K)"""
    x = np.asarray(x, dtype=np.float64)
    mask = np.asarray(mask, dtype=np.float64)
    starts, tables = plan(x.shape[:3], roi, overlap, mode, sigma_scale)
    occ = occupancy_ref(mask, roi, starts)
    acc = None
    for iz, z in enumerate(starts[0]):
        for iy, y in enumerate(starts[1]):
            for ix, xx in enumerate(starts[2]):
                if skip_empty and occ[iz, iy, ix] == 0:
                    continue
                for flip in flips:
                    p = np.asarray(predict(gather_ref(x, roi, (z, y, xx), flip, mean, std)), dtype=np.float64)
                    if acc is None:
                        acc = np.zeros(x.shape[:3] + (p.shape[-1],), dtype=np.float64)
                    accumulate_ref(acc, p, tables, (z, y, xx), flip, (iz, iy, ix), 1.0 / len(flips))
    return acc * mask
