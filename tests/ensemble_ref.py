"""numpy restatement of csrc/ensemble.hip and of infer.uncertainty_scores (shared by tests/test_ensemble_*.py; imported the way
regions_ref and segment_ref are): Welford's recurrence in float32 and in float64, the two level formulas in float64, the
(channel, level, pair) table by brute force and the score reduction by its definition, threshold by threshold."""
import numpy as np

LEVELS = 101
BRATS_REGIONS = (('wt', (1, 2, 3)), ('tc', (1, 3)), ('et', (3,)))


def welford(members, dtype):
    """members: a list of equal-shaped arrays -> (mean, m2) after d = p - mean; mean += d / k; m2 += d * (p - mean), every operation in
    `dtype` and rounded on its own (numpy never contracts); member 1 writes mean = p, m2 = 0"""
    mean = m2 = None
    for k, p in enumerate(members, 1):
        p = np.asarray(p, dtype=dtype)
        if k == 1:
            mean, m2 = p.copy(), np.zeros_like(p)
            continue
        d = p - mean
        mean = mean + d / dtype(k)
        m2 = m2 + d * (p - mean)
    return mean, m2


def exact_moments(members):
    """float64 mean and sum of squared deviations, two passes"""
    a = np.stack([np.asarray(p, dtype=np.float64) for p in members])
    mean = a.mean(axis=0)
    return mean, ((a - mean) ** 2).sum(axis=0)


def entropy_scaled(mean):
    """100 h of p = clamp(mean, 0, 1) in float64, h = -(p log2 p + (1 - p) log2(1 - p)), 0 at p in {0, 1}"""
    p = np.clip(np.asarray(mean, dtype=np.float64), 0.0, 1.0)
    q = 1.0 - p
    with np.errstate(divide='ignore', invalid='ignore'):
        h = -(np.where(p > 0, p * np.log2(np.where(p > 0, p, 1.0)), 0.0) + np.where(q > 0, q * np.log2(np.where(q > 0, q, 1.0)), 0.0))
    return 100.0 * h


def std_scaled(spread, scale):
    """200 sqrt(max(spread, 0) * scale) in float64"""
    return 200.0 * np.sqrt(np.maximum(np.asarray(spread, dtype=np.float64), 0.0) * float(scale))


def levels(scaled, mask):
    """min(100, floor(scaled + 0.5)) as uint8, 0 where mask (one value per voxel, broadcast over the channels) == 0"""
    lv = np.minimum(100.0, np.floor(scaled + 0.5)).astype(np.uint8)
    return np.where(np.asarray(mask).reshape(lv.shape[:-1] + (1,)) != 0, lv, 0).astype(np.uint8)


def near_half(scaled, band=1e-3):
    """where the exact scaled value lies within `band` of a half-integer: there, and only there, a float32 evaluation may round the other
    way"""
    return np.abs(scaled - np.floor(scaled) - 0.5) <= band


def table(truth, pred, unc, class_masks, mask=None, K=4):
    """(C, 101, 4) int64 by brute force: per voxel with mask != 0 and channel c, cell [c][min(unc, 100)][2 t + pr]"""
    t = np.minimum(np.asarray(truth).reshape(-1).astype(np.int64), K - 1)
    p = np.minimum(np.asarray(pred).reshape(-1).astype(np.int64), K - 1)
    u = np.minimum(np.asarray(unc).reshape(t.size, len(class_masks)).astype(np.int64), 100)
    keep = np.ones(t.size, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0
    out = np.zeros((len(class_masks), LEVELS, 4), dtype=np.int64)
    for c, cm in enumerate(class_masks):
        tt, pp = (int(cm) >> t) & 1, (int(cm) >> p) & 1
        np.add.at(out[c], (u[keep, c], (2 * tt + pp)[keep]), 1)
    return out


def scores(counts):
    """(101, 4) counts [level, (TN, FP, FN, TP)] -> (score, dice_auc, ftp_auc, ftn_auc) by the definition, one threshold at a time"""
    counts = np.asarray(counts, dtype=np.int64)
    tn100, tp100 = int(counts[:, 0].sum()), int(counts[:, 3].sum())
    dice, ftp, ftn = [], [], []
    for tau in range(LEVELS):
        tn, fp, fn, tp = (int(v) for v in counts[:tau + 1].sum(axis=0))
        den = 2 * tp + fp + fn
        dice.append(2.0 * tp / den if den else 1.0)
        ftp.append((tp100 - tp) / tp100 if tp100 else 0.0)
        ftn.append((tn100 - tn) / tn100 if tn100 else 0.0)

    def auc(v):
        return sum((v[i] + v[i + 1]) / 2.0 for i in range(LEVELS - 1)) / 100.0
    a, b, c = auc(dice), auc(ftp), auc(ftn)
    return (a + (1.0 - b) + (1.0 - c)) / 3.0, a, b, c


def class_masks(targets='labels', K=4):
    sets = [sel for _, sel in BRATS_REGIONS] if targets == 'regions' else [(c,) for c in range(1, K)]
    return [sum(1 << c for c in sel) for sel in sets]


def member_sets(shape, seed):
    """the three kinds of members the kernels are held to -> {'random', 'saturated', 'near_half'}: lists of 5 float32 arrays"""
    rng = np.random.default_rng(seed)
    return {'random': [rng.random(shape, dtype=np.float32) for _ in range(5)],
            'saturated': [(rng.random(shape) > 0.5).astype(np.float32) for _ in range(5)],
            'near_half': [(0.5 + (rng.random(shape) * 2.0 - 1.0) * 5e-4).astype(np.float32) for _ in range(5)]}
