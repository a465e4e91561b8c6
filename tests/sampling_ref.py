"""numpy restatement of the class-location table (bts_class_locations) and of data.draw_foreground, for the tests of the foreground
oversampling: the formulae of include/bts_hip.h and of draw_foreground's docstring, written independently of both."""
import numpy as np
import torch


def table_entries(n, k):
    """(s_c, m_c) of a class of n voxels in a table of capacity k: the stride max(1, ceil(n / k)) and the ceil(n / s_c) entries held"""
    s = max(1, (n + k - 1) // k)
    return s, (n + s - 1) // s


def class_locations_ref(y, out_ch, k):
    """y: labels of any shape (label c + 1 = class c) -> (counts int64 (out_ch,), loc int32 (out_ch, k)): every s_c-th voxel of each class
    in ascending linear index, padded with -1"""
    flat = np.asarray(y).ravel()
    counts = np.zeros(out_ch, np.int64)
    loc = np.full((out_ch, k), -1, np.int32)
    for c in range(out_ch):
        idx = np.flatnonzero(flat == c + 1)
        counts[c] = idx.size
        sel = idx[::table_entries(idx.size, k)[0]]
        assert sel.size == table_entries(idx.size, k)[1] <= k
        loc[c, :sel.size] = sel
    return counts, loc


def foreground_offsets(u, prob, classes, counts, loc, vol_size, crop_size, offsets):
    """the formulae of the foreground draw on u = [u_on, u_class, u_voxel]; classes: the allowed ones or None for all"""
    allowed = range(len(counts)) if classes is None else sorted(classes)
    present = [c for c in allowed if counts[c] > 0]
    if not (u[0] < prob) or not present:
        return list(offsets)
    c = present[min(int(u[1] * len(present)), len(present) - 1)]
    m = table_entries(int(counts[c]), loc.shape[1])[1]
    p = np.unravel_index(int(loc[c][min(int(u[2] * m), m - 1)]), tuple(vol_size))
    return [int(min(max(int(p[a]) - crop_size[a] // 2, 0), vol_size[a] - crop_size[a])) for a in range(3)]


def draw_foreground_ref(gen, prob, classes, counts, loc, vol_size, crop_size, offsets):
    """takes torch.rand(3, float64) from `gen`, whatever the branch -> the three offsets"""
    u = torch.rand(3, generator=gen, dtype=torch.float64).tolist()
    return foreground_offsets(u, prob, classes, counts, loc, vol_size, crop_size, offsets)
