"""Explicit numpy restatement of what the reference's preprocessing computes (preprocess.py:17-131), written from its semantics; the
oracle of csrc/prepro.hip and bts_amd.preprocess.  tests/test_prepro_host.py proves it equal to results recorded from the reference
itself (tests/golden/prepro_vectors.npz), so the GPU tests need neither the reference nor its dependencies.

A case is a pair (x (S0,S1,S2,C) float32, y (S0,S1,S2) float32); a dataset is a list of cases in visiting order.

  bounds      per axis the first and the last index whose plane holds a non-zero value (numpy truth: NaN yes, -0.0 no) in any channel
              of any case
  crop        [lo:hi] on every axis -- hi is the LAST occupied index, so that plane is dropped and size = hi - lo
  labels      y >= 4 -> 3
  split       with create_val the first len // 11 cases are the validation set, the rest (and only the rest) give the statistics
  norm        mean[c] = sum(x) / #(x > 0), std[c] = sqrt(sum((x - mean)^2) / #(x > 0)), sums over every voxel of the crops
  example     float32((float64(x) - mean) / std)

numpy adds the voxels of a volume one after the other, per channel, in MEMORY order, and the reference's volumes are stacks of
Fortran-ordered files, so its order is axis 2 outermost, axis 0 innermost; `memory_order_sum` restates that.  `norm` has two modes
that differ in the first pass only.  'float64' adds every x in float64.  'float32-sum' mimics the reference: it adds each volume up
in float32 before adding the volumes in float64.  Where the per-volume totals are integers below 2^24 the two modes agree bit for
bit.  The second pass, sum((x - mean)^2), is float64 in the reference and in both modes here.
"""
import numpy as np


def occupancy(x):
    """three boolean vectors: which planes of axis 0, 1, 2 hold an x != 0"""
    nz = np.asarray(x) != 0                                   # NaN != 0 is True, -0.0 != 0 is False
    return [nz.any(axis=tuple(a for a in range(4) if a != ax)) for ax in range(3)]


def bounds(cases):
    """-> (lo, hi): first and LAST occupied index per axis over all cases"""
    lo, hi = [None] * 3, [None] * 3
    for x, _ in cases:
        for ax, o in enumerate(occupancy(x)):
            idx = np.nonzero(o)[0]
            if idx.size == 0:
                raise ValueError('a case without a non-zero voxel')
            lo[ax] = int(idx[0]) if lo[ax] is None else min(lo[ax], int(idx[0]))
            hi[ax] = int(idx[-1]) if hi[ax] is None else max(hi[ax], int(idx[-1]))
    return tuple(lo), tuple(hi)


def crop(v, lo, hi):
    return v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


def labels(y):
    y = np.array(y, dtype=np.float32, copy=True)
    y[y >= 4] = 3
    return y


def split(n, create_val):
    """-> (indices of the validation cases, indices of the training cases)"""
    k = n // 11 if create_val else 0
    return list(range(k)), list(range(k, n))


def pairwise_sum(a):
    """numpy's summation of one contiguous run: below 8 terms one after the other, up to 128 terms eight interleaved partial sums
    combined as a balanced tree plus the remainder one by one, above that the two halves (the first a multiple of 8) recursively"""
    n = len(a)
    if n < 8:
        t = a.dtype.type(0)
        for v in a:
            t = t + v
        return t
    if n <= 128:
        r = [a[k] for k in range(8)]
        i = 8
        while i < n - (n % 8):
            r = [r[k] + a[i + k] for k in range(8)]
            i += 8
        t = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[i:]:
            t = t + v
        return t
    half = n // 2
    half -= half % 8
    return pairwise_sum(a[:half]) + pairwise_sum(a[half:])


def memory_order_sum(v, compact=False):
    """per-channel sum of a (h,w,d,C) array in its own dtype, in memory order: axis 2 outermost, axis 0 innermost.  With C > 1 the
    voxels are added one after the other.  With C = 1 the terms of a channel are adjacent in memory and numpy sums each contiguous
    run pairwise: the whole volume where it is `compact` (a freshly computed array such as (x - mean)^2), else each run along
    axis 0 (a crop is a strided view), the runs added one after the other."""
    flat = np.ascontiguousarray(v.transpose(2, 1, 0, 3))
    if v.shape[-1] == 1:
        if compact:
            return np.array([pairwise_sum(flat.reshape(-1))])
        t = v.dtype.type(0)
        for run in flat.reshape(-1, v.shape[0]):
            t = t + pairwise_sum(run)
        return np.array([t])
    acc = np.zeros(v.shape[-1], v.dtype)
    for row in flat.reshape(-1, v.shape[-1]):
        acc = acc + row
    return acc


def volume_sum(x, mode):
    """per-channel sum of one cropped volume as a float64 vector"""
    if mode == 'float64':
        return memory_order_sum(x.astype(np.float64))
    if mode == 'float32-sum':
        return memory_order_sum(x).astype(np.float64)
    raise ValueError(mode)


def norm(xs, mode='float64'):
    """cropped training volumes -> (mean, std, count, sum_x, sum_sq), each a float64 vector of C values"""
    c = xs[0].shape[-1]
    s, n = np.zeros(c), np.zeros(c)
    for x in xs:
        s += volume_sum(x, mode)
        n += (x > 0).reshape(-1, c).sum(axis=0)
    mean = s / n
    q = np.zeros(c)
    for x in xs:
        d = x.astype(np.float64) - mean
        q += memory_order_sum(d * d, compact=True)
    std = np.sqrt(q / n)
    return mean, std, n, s, q


def normalize(x, mean, std):
    return ((x.astype(np.float64) - mean) / std).astype(np.float32)


def run(cases, create_val=False, mode='float64'):
    """the whole of the reference's main on a list of cases -> dict(lo, hi, size, val, train, mean, std, count, sum_x, sum_sq,
    x (normalised float32 per case), y (remapped, (h,w,d,1) per case))"""
    lo, hi = bounds(cases)
    c = cases[0][0].shape[-1]
    xs = [crop(x, lo, hi) for x, _ in cases]
    ys = [crop(labels(y), lo, hi)[..., None] for _, y in cases]
    val, train = split(len(cases), create_val)
    mean, std, n, s, q = norm([xs[i] for i in train], mode)
    return {'lo': lo, 'hi': hi, 'size': {'h': hi[0] - lo[0], 'w': hi[1] - lo[1], 'd': hi[2] - lo[2], 'c': c},
            'val': val, 'train': train, 'mean': mean, 'std': std, 'count': n, 'sum_x': s, 'sum_sq': q,
            'x': [normalize(x, mean, std) for x in xs], 'y': ys}
