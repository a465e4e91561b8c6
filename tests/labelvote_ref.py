"""numpy float64 restatement of moving a label map through a general affine by vote (helper module, not collected): csrc/conform.hip's
bts_label_resample3d, built on the pieces of tests/conform_ref.py that tests/test_conform_host.py pins to SciPy.

  coordinate, field of view    conform_ref.coordinates, conform_ref.inside: s = M (o0, o1, o2, 1) in float64, 0 outside [-0.5, n - 0.5]
  taps                         conform_ref._taps(order=1): floor(s) and floor(s) + 1 per axis, reflected; weight (wd * wh) * ww, row-major
  vote                         a value's weight is the sum, in tap order, of the weights of the taps that hold it
  result                       the value of the largest weight; of exactly equal weights the smallest value
  margin                       the winner's weight minus the largest weight of another value (the winner's own weight where all 8 taps
                               agree): a voxel with a margin of rounding size is one where the last bit decides
"""
import numpy as np

import conform_ref

VALUES = (0.0, 1.0, 2.0, 4.0)


def taps(y, matrix, out_shape):
    """-> (values (8,) + out_shape, weights (8,) + out_shape) in row-major tap order, float64"""
    a = np.asarray(y, dtype=np.float64)
    a = a[..., 0] if a.ndim == 4 else a
    s = conform_ref.coordinates(matrix, out_shape)
    (idd, wd), (ih, wh), (iw, ww) = [conform_ref._taps(s[b], a.shape[b], 1, np.float64) for b in range(3)]
    val, wt = [], []
    for i in range(2):
        for j in range(2):
            for k in range(2):
                val.append(a[idd[..., i], ih[..., j], iw[..., k]])
                wt.append((wd[..., i] * wh[..., j]) * ww[..., k])
    return np.stack(val), np.stack(wt)


def label_vote(y, matrix, out_shape):
    """y (D,H,W) or (D,H,W,1) -> (labels out_shape float32, margin out_shape float64)"""
    y = np.asarray(y)
    src = y.shape[:3]
    val, wt = taps(y, matrix, out_shape)
    total = np.zeros_like(wt)
    for t in range(8):
        for u in range(8):                                             # in tap order, a tap of another value adds nothing
            total[t] += np.where(val[u] == val[t], wt[u], 0.0)
    best_w = np.full(tuple(out_shape), -1.0)
    best_v = np.zeros(tuple(out_shape))
    for t in range(8):
        take = (total[t] > best_w) | ((total[t] == best_w) & (val[t] < best_v))
        best_w = np.where(take, total[t], best_w)
        best_v = np.where(take, val[t], best_v)
    other = np.zeros(tuple(out_shape))
    for t in range(8):
        other = np.maximum(other, np.where(val[t] != best_v, total[t], 0.0))
    fov = conform_ref.inside(matrix, out_shape, src)
    return np.where(fov, best_v, 0.0).astype(np.float32), np.where(fov, best_w - other, np.inf)


def label_volume(shape, seed, values=VALUES):
    """nested ellipsoids of values[2] > values[1] > values[3] on values[0] (2 around 1 around 4 on 0), and 3 % random speckle drawn from
    the four values, so that many voxels see 3 or 4 different values among their taps -> float32"""
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    cx = rng.uniform(-0.15, 0.15, 3)
    r2 = sum(((g[k] - cx[k]) / (0.8, 0.75, 0.85)[k]) ** 2 for k in range(3))
    out = np.full(shape, values[0], dtype=np.float32)
    out[r2 < 1.0] = values[2]
    out[r2 < 0.45] = values[1]
    out[r2 < 0.15] = values[3]
    speckle = rng.random(shape) < 0.03
    out[speckle] = np.asarray(values, dtype=np.float32)[rng.integers(0, 4, size=shape)][speckle]
    return out


def shift_matrix(shift):
    """the identity plus a translation: with 0.5 every weight is exactly 0.5 (one axis) or 0.125 (three), and ties are exact"""
    m = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1)
    m[:, 3] = shift
    return m


TIE_SHIFTS = {'w': (0.0, 0.0, 0.5), 'dhw': (0.5, 0.5, 0.5)}


def tied(y, matrix, out_shape):
    """voxels inside the field of view whose two best values have exactly equal weights"""
    _, margin = label_vote(y, matrix, out_shape)
    return margin == 0.0
