"""numpy float64 restatement of the per-case normalisation (the contract of bts_case_norm), shared by tests/test_casenorm_host.py
and tests/test_casenorm_gpu.py, imported the way prepro_ref and norm_ref are.

x (T0,T1,T2,C) float32; mask (T0,T1,T2) non-zero = inside, None = any channel > 0; clip None or (p_lo, p_hi).
  n        voxels inside, the same for every channel
  bound    s = the inside values of a channel in ascending order; h = (n-1) p / 100, k = floor(h), f = h - k;
           s[k] + f (s[min(k+1,n-1)] - s[k]) in float64; -inf / +inf without clipping
  v        clamp(float64(x), lo_c, hi_c)        (numpy's maximum, then minimum)
  mean_c   sum v / n;  std_c = sqrt(sum (v - mean_c)^2 / n), two passes
  out      float32((v - mean_c) / std_c) inside, +0.0 outside; +0.0 throughout a channel with std_c == 0 and everywhere when n == 0
  stats    [n, (mean, std, lo, hi) per channel], all 0 when n == 0
"""
import numpy as np


def inside_mask(x, mask=None):
    if mask is None:
        return (x > 0).any(axis=-1)
    return np.asarray(mask).reshape(x.shape[:3]) != 0


def percentile_bound(s, p):
    """s: ascending float64, at least one value"""
    n = s.size
    h = np.float64(n - 1) * np.float64(p) / np.float64(100.0)
    k = int(np.floor(h))
    f = h - np.float64(k)
    k1 = min(k + 1, n - 1)
    return s[k] + f * (s[k1] - s[k])


def clamp(x64, lo, hi):
    return np.minimum(np.maximum(x64, lo), hi)


def apply_stats(x, inside, stats):
    """the output the contract defines for given statistics: float32((clamp(x) - mean) / std) in float64, rounded once"""
    c = x.shape[-1]
    out = np.zeros(x.shape, dtype=np.float32)
    n = stats[0]
    for ch in range(c):
        mean, std, lo, hi = stats[1 + 4 * ch:5 + 4 * ch]
        if n == 0 or std == 0:
            continue
        v = clamp(x[..., ch].astype(np.float64), lo, hi)
        with np.errstate(all='ignore'):
            r = ((v - mean) / std).astype(np.float32)
        out[..., ch] = np.where(inside, r, np.float32(0.0))
    return out


def case_norm(x, mask=None, clip=None):
    """-> (out float32, stats float64 (1 + 4C,), sums: per channel (sum v, sum (v - mean)^2, sum |v|, sum (v - mean)^2 terms' bound))"""
    x = np.asarray(x, dtype=np.float32)
    c = x.shape[-1]
    inside = inside_mask(x, mask)
    n = int(inside.sum())
    stats = np.zeros(1 + 4 * c, dtype=np.float64)
    sums = np.zeros((c, 3), dtype=np.float64)
    stats[0] = n
    if n == 0:
        return np.zeros(x.shape, dtype=np.float32), stats, sums
    for ch in range(c):
        vals = x[..., ch][inside].astype(np.float64)
        lo, hi = -np.inf, np.inf
        if clip is not None:
            s = np.sort(vals)
            lo, hi = percentile_bound(s, clip[0]), percentile_bound(s, clip[1])
        v = clamp(vals, lo, hi)
        total = v.sum()
        mean = total / n
        d = v - mean
        sq = (d * d).sum()
        std = np.sqrt(sq / n)
        stats[1 + 4 * ch:5 + 4 * ch] = (mean, std, lo, hi)
        sums[ch] = (total, sq, np.abs(v).sum())
    return apply_stats(x, inside, stats), stats, sums
