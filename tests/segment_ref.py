"""Restatement of the two-stage chain and of the per-case score for the tests of bts_amd.infer.segment_case / label_scores and
csrc/segment.hip (helper module, not collected).

  two-stage chain  test.py:235-264 with the skull stage (:238-248), from the oracle's pad_to_spatial_res / tta_predict / tta_labels
                   and zoom_ref's float64 resampling; each stage is a function of the previous stage's output, so a test can feed it
                   the engine's own intermediate tensors
  confusion        np.bincount over min(t, K-1) * K + min(p, K-1)
  scores           one-hot arithmetic with the sums of util.py:50-55 (oracle.torch_ref.dice_coefficient's), NOT through the confusion
                   matrix: labels -> classes min(label, K-1), one-hot with the background dropped (train.py:39-41)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import zoom_ref  # noqa: E402
from oracle import torch_ref as R  # noqa: E402


def padded(shape, res):
    """pad_to_spatial_res's extent: a full extra block where the size is already a multiple (test.py:164-178)"""
    return tuple(int(s) + res - (int(s) % res) for s in shape)


def scan_like(vol, seed, hole=0.3):
    """a (D,H,W,2) float32 volume with smooth positive texture and an ellipsoidal zero region (background for the brain mask)"""
    g = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in vol], indexing='ij')
    rng = np.random.default_rng(seed)
    tex = 0.65 + 0.35 * np.sin(5.0 * g[0] + 1.0) * np.cos(4.0 * g[1] + 2.0) * np.sin(6.0 * g[2] + 0.5) + 0.02 * rng.standard_normal(vol)
    chans = []
    for c, a in enumerate((160.0, 190.0)):
        r2 = ((g[0] - 0.05 * c) / hole) ** 2 + (g[1] / (hole - 0.05)) ** 2 + (g[2] / (hole + 0.05)) ** 2
        chans.append(np.where(r2 < 1.0, 0.0, tex * a))
    return np.stack(chans, axis=-1).astype(np.float32)


def randomised_params(cfg, crop, seed):
    """oracle ParamSet with every gamma / beta / bias randomised, fp32-representable (as tests/test_infer_gpu.py::randomised_params)"""
    P = R.build_params(cfg, crop, seed=seed)
    g = torch.Generator().manual_seed(seed + 1)
    for k in P:
        if k.endswith('_b'):
            P[k] = torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.1
        if k.endswith('_g'):
            P[k] = 1.0 + torch.randn(P[k].shape, generator=g, dtype=torch.float64) * 0.3
    for k in P:
        P[k] = P[k].float().double()
    return P


# ---- the chain, stage by stage (numpy in, numpy out; float64 inside the oracle) --------------------------------------------------
def resample(image, pixdim, order, pad_res):
    """test.py:45-56 + pad_to_spatial_res -> (x padded float64, mask padded float32, shape on the 1 mm^3 grid)"""
    unit = all(float(f) == 1.0 for f in pixdim)
    shape = tuple(image.shape[:3]) if unit else zoom_ref.zoom_output_shape(image.shape[:3], pixdim)
    y = np.asarray(image, dtype=np.float64) if unit else zoom_ref.zoom(image, shape, order, np.float64)
    m = zoom_ref.brain_mask(y)
    xp, mp, _ = R.pad_to_spatial_res(pad_res, torch.from_numpy(y), torch.from_numpy(m))
    return xp.numpy(), mp.numpy(), shape


def stage_prob(xp, mp, P, cfg, mean, std):
    """TestTimeAugmentor.__call__ (test.py:105-161): masked mean probability on the padded grid, float64"""
    as64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    return R.tta_predict(as64(xp), as64(mp), P, cfg, as64(mean), as64(std)).numpy()


def strip(x, p, m, orig, pad_to):
    """test.py:244-254 in numpy float32: x * (1 - p), slice to `orig`, pad to `pad_to`; the mask sliced and padded alike"""
    x, p, m = (np.asarray(a, dtype=np.float32) for a in (x, p, m))
    d, h, w = orig
    xo = np.zeros(tuple(pad_to) + (x.shape[-1],), dtype=np.float32)
    mo = np.zeros(tuple(pad_to) + (1,), dtype=np.float32)
    xo[:d, :h, :w] = (x * (np.float32(1) - p))[:d, :h, :w]
    mo[:d, :h, :w] = m[:d, :h, :w]
    return xo, mo


def reverse(prob, mask, native, pixdim, order):
    """Interpolator.reverse as bts_amd.infer states it: probabilities (configured order) and mask (order 0) back to the scan's
    extent, masked -> (probabilities float64, mask float64)"""
    if all(float(f) == 1.0 for f in pixdim):
        return np.asarray(prob, dtype=np.float64) * mask, np.asarray(mask, dtype=np.float64)
    back = zoom_ref.zoom(np.asarray(prob, dtype=np.float64), native, order, np.float64)
    mback = zoom_ref.zoom(np.asarray(mask, dtype=np.float64), native, 0, np.float64)
    return back * mback, mback


def labels(prob, mask, threshold=0.5):
    return R.tta_labels(torch.from_numpy(np.asarray(prob, dtype=np.float64)), torch.from_numpy(np.asarray(mask, dtype=np.float64)),
                        threshold).numpy()


def ambiguous(prob, threshold=0.5, eps=1e-4):
    """the voxels tests/test_infer_gpu.py leaves out of the label comparison: best class within eps of the threshold or of a tie"""
    srt = np.sort(np.asarray(prob, dtype=np.float64), axis=-1)[..., ::-1]
    amb = np.abs(srt[..., 0] - threshold) < eps
    if srt.shape[-1] > 1:
        amb |= (srt[..., 0] - srt[..., 1]) < eps
    return amb


def two_stage(image, pixdim, skull, tumor, order=3, threshold=0.5):
    """the whole chain by the oracle alone; skull / tumor: dicts with P, cfg, mean, std, res -> dict of every stage's output"""
    xp, mp, shape = resample(image, pixdim, order, skull['res'])
    p = stage_prob(xp, mp, skull['P'], skull['cfg'], skull['mean'], skull['std'])
    xo, mo = strip(xp, p, mp, shape, padded(shape, tumor['res']))
    y = stage_prob(xo, mo, tumor['P'], tumor['cfg'], tumor['mean'], tumor['std'])[:shape[0], :shape[1], :shape[2]]
    yb, mb = reverse(y, mp[:shape[0], :shape[1], :shape[2]], tuple(image.shape[:3]), pixdim, order)
    return {'x1mm': xp, 'mask': mp, 'skull_prob': p, 'x_stripped': xo, 'mask_repadded': mo, 'prob_1mm': y, 'prob': yb, 'mask_native': mb,
            'labels': labels(yb, mb, threshold)}


# ---- the score ----------------------------------------------------------------------------------------------------------------
def confusion(truth, pred, k):
    t = np.minimum(np.asarray(truth).reshape(-1).astype(np.int64), k - 1)
    p = np.minimum(np.asarray(pred).reshape(-1).astype(np.int64), k - 1)
    return np.bincount(t * k + p, minlength=k * k).reshape(k, k).astype(np.int64)


def _onehot(lab, k):
    """classes min(label, k-1), one-hot, background channel dropped -> (nvox, k-1) float64"""
    c = np.minimum(np.asarray(lab).reshape(-1).astype(np.int64), k - 1)
    return np.eye(k, dtype=np.float64)[c][:, 1:]


def _binary_dice(a, b):
    den = float(a.sum() + b.sum())
    return 2.0 * float((a & b).sum()) / den if den else float('nan')


def scores_onehot(truth, pred, k=4):
    yt, yp = _onehot(truth, k), _onehot(pred, k)
    inter, p, t = (yp * yt).sum(axis=0), yp.sum(axis=0), yt.sum(axis=0)                   # util.py:50-52
    den = yp.sum() + yt.sum()
    out = {'macro': float(np.mean((2.0 * inter + 1.0) / (p + t + 1.0))),                    # util.py:54
           'micro': float((yp * yt).sum() / den) if den else float('nan'),                  # util.py:55
           'dice': [float(2.0 * inter[c] / (p[c] + t[c])) if p[c] + t[c] else float('nan') for c in range(k - 1)]}
    if k == 4:
        tr, pr = np.asarray(truth).reshape(-1), np.asarray(pred).reshape(-1)
        out['wt'] = _binary_dice(tr >= 1, pr >= 1)                                          # labels {1,2,4}
        out['tc'] = _binary_dice((tr == 1) | (tr >= 3), (pr == 1) | (pr >= 3))              # labels {1,4}
        out['et'] = _binary_dice(tr >= 3, pr >= 3)                                          # label {4}
    return out
