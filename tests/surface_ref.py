"""NumPy restatement of the distance side of the per-case score (csrc/surface.hip, bts_amd.infer.surface_scores), for
tests/test_surface_host.py and tests/test_surface_gpu.py (helper module, not collected).

  region      boolean mask of the classes min(label, K-1) named by a bit mask
  surface     a voxel of the mask with a face neighbour outside the mask or outside the volume, by padded neighbour tests
  edt_sq      the separable float64 transform with the kernel's operations in the kernel's order: along W, then H, then D,
              out[i] = min_j (g[j] + (s*(i-j))**2), every product and sum one IEEE operation
  edt_sq_brute  minimum over all feature voxels of the squared distance in mm^2, for tiny volumes
  hd95        np.percentile of the pooled directed surface distances (medpy's hd95), with the empty-mask rules
"""
import numpy as np

BRATS = {'wt': 0b1110, 'tc': 0b1010, 'et': 0b1000}


def widened(spacing):
    """float32 pixdim values widened to float64, as the command hands them on"""
    return tuple(float(np.float32(s)) for s in spacing)


def region(lab, k, class_mask):
    c = np.minimum(np.asarray(lab).astype(np.int64), k - 1)
    return ((class_mask >> c) & 1).astype(bool)


def surface(mask):
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1, mode='constant', constant_values=False)
    inner = (p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:])
    return m & ~inner


def _pass(g, axis, s):
    """out[i] = min_j (g[j] + (s*(i-j))**2) along `axis`"""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    idx = np.arange(n, dtype=np.float64)
    t = np.float64(s) * (idx[:, None] - idx[None, :])              # [i, j], one rounding
    cost = t * t                                                   # one rounding
    out = np.empty_like(g)
    for i in range(n):
        out[..., i] = np.min(g + cost[i], axis=-1)                 # one rounding per sum; the minimum is exact
    return np.moveaxis(out, -1, axis)


def edt_sq(feat, spacing):
    """squared distance in mm^2 to the nearest voxel with feat != 0; +inf everywhere when there is none"""
    sd, sh, sw = spacing
    g = np.where(np.asarray(feat) != 0, 0.0, np.inf).astype(np.float64)
    return _pass(_pass(_pass(g, 2, sw), 1, sh), 0, sd)


def edt_sq_brute(feat, spacing):
    feat = np.asarray(feat) != 0
    pts = np.argwhere(feat).astype(np.float64)
    out = np.full(feat.shape, np.inf)
    if len(pts) == 0:
        return out
    s = np.asarray(spacing, dtype=np.float64)
    for v in np.ndindex(*feat.shape):
        d = (np.asarray(v, dtype=np.float64) - pts) * s
        out[v] = np.min((d * d).sum(axis=1))
    return out


def directed_sq(t_mask, p_mask, spacing):
    """-> (d2(P->T), d2(T->P)): squared distances from the surface voxels of one mask to the nearest surface voxel of the other, each
    in the flat order of its volume"""
    st, sp = surface(t_mask), surface(p_mask)
    return edt_sq(st, spacing)[sp], edt_sq(sp, spacing)[st]


def hd95(t_mask, p_mask, spacing, percentile=95.0):
    """-> {'hd95', 'hd', 'hd95_directed': (P->T, T->P), 'surface_voxels': (|T|, |P|)}; nan when both masks are empty, inf when one is"""
    t_mask, p_mask = np.asarray(t_mask, dtype=bool), np.asarray(p_mask, dtype=bool)
    nt, npr = int(surface(t_mask).sum()), int(surface(p_mask).sum())
    if nt == 0 or npr == 0:
        v = float('nan') if nt == npr else float('inf')
        return {'hd95': v, 'hd': v, 'hd95_directed': (v, v), 'surface_voxels': (nt, npr)}
    pt, tp = (np.sqrt(d) for d in directed_sq(t_mask, p_mask, spacing))
    pooled = np.concatenate([pt, tp])
    return {'hd95': float(np.percentile(pooled, percentile)), 'hd': float(pooled.max()),
            'hd95_directed': (float(np.percentile(pt, percentile)), float(np.percentile(tp, percentile))),
            'surface_voxels': (nt, npr)}


def rates_onehot(truth, pred, class_mask, k=4):
    """sensitivity and specificity of a region from boolean arithmetic on the two maps; nan where undefined"""
    t, p = region(truth, k, class_mask).reshape(-1), region(pred, k, class_mask).reshape(-1)
    tp, fn, tn, fp = int((t & p).sum()), int((t & ~p).sum()), int((~t & ~p).sum()), int((~t & p).sum())
    return (tp / (tp + fn) if tp + fn else float('nan')), (tn / (tn + fp) if tn + fp else float('nan'))
