"""The nested BraTS regions in numpy, float64 or integer, written from their definition (include/bts_hip.h): the
reference tests/test_regions_host.py and tests/test_regions_gpu.py hold csrc/regions.hip to.  Channels are (WT, TC, ET) = labels
{1,2,4}, {1,4}, {4}; a label map holds 0, 1, 2, 4."""
import numpy as np

LABELS = (1, 2, 4)


def onehot(lab):
    """label map over {0,1,2,4} -> (..., 3) float64 one-hot without the background, as the augment kernels write it"""
    lab = np.asarray(lab)
    return np.stack([(lab == v) for v in LABELS], axis=-1).astype(np.float64)


def encode(onehot_labels):
    """(..., 3) one-hot (l1, l2, l3) -> (..., 3) regions (l1 + l2 + l3, l1 + l3, l3), float64"""
    o = np.asarray(onehot_labels, dtype=np.float64)
    l1, l2, l3 = o[..., 0], o[..., 1], o[..., 2]
    return np.stack([l1 + l2 + l3, l1 + l3, l3], axis=-1)


def decode(prob, mask=None, threshold=0.5, strict=False):
    """(..., 3) region probabilities -> int64 label map over {0,1,2,4} by the OVERWRITE rule on prob * mask: 4 where et passes, else 1
    where tc passes, else 2 where wt passes, else 0, and 0 where mask == 0.  A value passes when it is >= threshold, or with `strict`
    when it is > threshold.  mask: (...) or (..., 1), None = ones.  The product is taken in the dtype of `prob` (a float32 input is
    masked in float32, as the device does; a mask of zeros and ones changes no value)."""
    p = np.asarray(prob)
    if mask is None:
        m = np.ones(p.shape[:-1], dtype=p.dtype)
    else:
        m = np.asarray(mask).reshape(p.shape[:-1]).astype(p.dtype)
    pm = p * m[..., None]
    on = (pm > threshold) if strict else (pm >= threshold)
    lab = np.zeros(p.shape[:-1], dtype=np.int64)
    lab[on[..., 0]] = 2
    lab[on[..., 1]] = 1
    lab[on[..., 2]] = 4
    lab[m == 0] = 0
    return lab


def decode_nested(prob, threshold=0.5):
    """the rule this project does NOT use: ET only inside TC inside WT"""
    on = np.asarray(prob) >= threshold
    wt, tc, et = on[..., 0], on[..., 0] & on[..., 1], on[..., 0] & on[..., 1] & on[..., 2]
    lab = np.zeros(on.shape[:-1], dtype=np.int64)
    lab[wt] = 2
    lab[tc] = 1
    lab[et] = 4
    return lab


def dice_counts(y_true, y_pred):
    """(..., 3) targets and probabilities -> int64 (9,): (I_r, P_r, T_r) per region with P_r = #(p_r > 0.5), T_r = #(t_r > 0.5), I_r = #
    of voxels where both hold"""
    t = np.asarray(y_true).reshape(-1, 3) > 0.5
    p = np.asarray(y_pred).reshape(-1, 3) > 0.5
    out = np.zeros(9, dtype=np.int64)
    for r in range(3):
        out[3 * r:3 * r + 3] = (int((t[:, r] & p[:, r]).sum()), int(p[:, r].sum()), int(t[:, r].sum()))
    return out


def dice_value(table):
    """(9,) counts -> (macro, micro) in float64: mean_r (2 I_r + 1) / (P_r + T_r + 1) and sum I / (sum P + sum T)"""
    c = np.asarray(table, dtype=np.float64).reshape(3, 3)
    inter, pred, true = c[:, 0], c[:, 1], c[:, 2]
    macro = float(np.mean((2.0 * inter + 1.0) / (pred + true + 1.0)))
    den = pred.sum() + true.sum()
    return macro, (float(inter.sum() / den) if den else float('nan'))
