"""Full-volume inference wrapper (reference test.py:78-178,259-261).

`pad_to_spatial_res` and `TestTimeAugmentor` keep the reference's names, argument order and arithmetic:
  * padding (test.py:164-178) appends `res - (size % res)` zero voxels per axis -- a FULL extra block when the size is
    already a multiple (reference quirk, kept: the channels_last GroupNorm statistics depend on the padded extent);
  * spatial TTA (test.py:95-103) runs the 8 subsets of {D,H,W} flips, un-flips each prediction, averages them and
    multiplies by the brain mask (:139-155).
Where the script is not functional (README.md:70 says so) the evident intent is implemented instead of the bug:
  * channel TTA (test.py:144-151) perturbs and re-feeds the *prediction*; here the normalised *input* is shifted/scaled
    by per-channel sigma as the training augmentation does (train.py:14-22), off by default;
  * the argmax is commented out (test.py:157-158) and `+1` / `>=3 -> 4` are applied to probabilities (:259-261);
    `labels()` applies them to the argmax, with 0 for masked-out voxels and voxels whose best class is below `threshold`.
  * `Interpolator` (test.py:15-72) uses pixdim[0] (qfac) as a zoom factor and adds [1.0] element-wise (test.py:46); here the
    spatial factors are (dx,dy,dz) = pixdim[1:4] and every channel is resampled on its own (scipy's 4-D call mixes the channels
    by up to 9e-6 relative at C=4 through its approximate boundary initialisation on short axes, a library artefact);
  * `Interpolator.reverse` (test.py:58-66,259-264) zooms the label VALUES with a cubic spline, which gives fractional labels, and
    to round(n * 1/pixdim), which need not be the scan's extent; here the probabilities (configured order) and the brain mask
    (order 0) are resampled to the scan's recorded native shape and the labels are taken there with bts_tta_finish.
  * the skull-stripping hand-over (test.py:238-258) is `segment_case`: the skull model's masked mean probability, inverted, multiplies
    the scan, which is cropped and padded again to the tumour model's resolution in the same pass (bts_skull_strip);
  * the score (test.py:226-232,266-270) hands a 1-channel raw label volume and a spline-zoomed label volume to DiceCoefficient, which
    expects one-hot truth and probabilities; `label_scores` gives the per-class Dice the call evidently intends, between the truth and
    the predicted label map on the scan's own grid, from a confusion matrix counted on the device (bts_label_confusion).
  * overlap alone is what the reference's score (test.py:266-270) can report; `surface_scores` adds the distance side BraTS tables
    carry, the 95th-percentile Hausdorff distance per class and region (bts_region_surface, bts_edt3d_sq, bts_masked_select), and
    `region_rates_from_confusion` sensitivity and specificity of the regions.
  * the reference writes and scores the raw arg-max; `remove_components` and `postprocess_labels` add the cleaning every practical
    pipeline applies first (small connected components removed, a tiny enhancing region relabelled, the brain mask reduced to its
    largest piece), off by default.
  * `lesionwise_scores` adds the lesion-wise Dice and HD95 BraTS has ranked by since 2023: every truth lesion scored on its own, a missed
    lesion 0, a predicted component on no lesion a false positive.  Its docstring is the definition; where published code differs in a
    detail, that definition holds: the HD95 of a lesion is `surface_scores`' (pooled directed distances, np.percentile, face-neighbour
    surfaces), a component reaching a lesion's dilated halo alone matches it, a component on a lesion ignored for its size is no
    false positive, two empty maps score (1, 0), and a region in which nothing is left to score gives nan.
  * the reference runs the network over the whole padded volume (test.py:128-134), an extent no training step produced; with a
    `WindowSpec` the `TestTimeAugmentor` predicts windows of the training crop instead and blends them with a Gaussian importance map,
    as nnU-Net and MONAI's sliding_window_inference do (`window_plan`; bts_window_gather, bts_window_accumulate, bts_window_occupancy),
    off by default.
  * the reference trains its per-channel sigmoids on disjoint one-hot labels and decodes an arg-max (train.py:38-41, test.py:259-261),
    although its model is the paper's, whose three channels are the nested regions; with `targets='regions'` (a network trained by
    `python -m bts_amd.train --targets regions`) the channels are read as WT, TC, ET and decoded by the overwrite rule of the usual
    BraTS conversions, 4 where et >= threshold, else 1 where tc >= threshold, else 2 where wt >= threshold (bts_region_finish), to the
    same {0,1,2,4} map everything downstream takes; 'labels', the default, is the arg-max as before.
  * the reference normalises every scan with one mean and deviation per channel of the training set (test.py:107), background included,
    although the paper it implements normalises each scan on its own brain voxels; with a `norm` of mode 'case' (a prepro.npy written by
    `python -m bts_amd.preprocess --norm case`, read by preprocess.load_norm) the `TestTimeAugmentor` does the latter, optionally after
    clamping to robust percentiles (bts_case_norm), so that a scan of another intensity scale gives the same labels; off by default.
  * the reference stacks its modalities voxel for voxel and scales along the array axes (test.py:21-46), whatever the headers say about
    orientation, spacing per modality or the grids of the modalities against each other: right for BraTS (all LPS, 1 mm, one grid), noise
    for anything else, since the network is not flip- or permutation-invariant.  A `Conformer` brings every modality onto one grid of
    a stated orientation and spacing by the affines (nifti.best_affine) -- an exact reorientation copy where the map is a signed
    permutation, a spline resample with a general matrix otherwise (bts_reorient3d, bts_affine_resample3d) -- and the prediction back;
    `segment_case(geometry=...)` uses it in place of the Interpolator, off by default.
  * the reference runs one tumour checkpoint (test.py:185-221) and says of a voxel its label and nothing else, although the paper it
    implements won BraTS 2018 with an ensemble of ten models.  A `StageEnsemble` stands wherever the tumour `StageSpec` does: every
    member runs its own TestTimeAugmentor on the same input and the unmasked means are averaged on the device by Welford's recurrence
    (bts_ensemble_update), which also keeps the members' spread; with `uncertainty` = 'entropy' or 'std' `segment_case` adds a map of
    levels 0..100 per voxel and channel on the scan's own grid (bts_uncertainty_finish), and `uncertainty_scores` gives the
    uncertainty-filtered Dice and the filtered true positives and negatives of the BraTS uncertainty task from one table counted on the
    device (bts_uncertainty_confusion); off by default.
All tensor work is on the device through the C ABI (bts_flip_affine, bts_tta_finish, bts_region_finish, bts_spline_prefilter3d, bts_zoom3d,
bts_skull_strip, bts_label_confusion, bts_region_surface, bts_edt3d_sq, bts_masked_select, bts_components3d, bts_component_sizes,
bts_component_largest, bts_components_apply, bts_region_relabel, bts_dilate3d, bts_lesion_pairs, bts_component_boxes, bts_lesion_crop,
bts_reorient3d, bts_affine_resample3d, bts_ensemble_update, bts_uncertainty_finish, bts_uncertainty_confusion, the model forward).
"""
import glob
import os

import numpy as np
import torch

from . import ops
from .data import TARGETS      # ('labels', 'regions'): disjoint labels decoded by an arg-max | the nested regions WT, TC, ET
from .tape import Tensor


def pad_to_spatial_res(res, x, mask):
    """x: (D,H,W,C), mask: (D,H,W,1) channels_last tensors -> (x_padded, mask_padded, orig_shape)  [test.py:164-178]"""
    shape = list(x.shape[:-1])
    pad = [res - (s % res) for s in shape]
    xp = torch.zeros((shape[0] + pad[0], shape[1] + pad[1], shape[2] + pad[2], x.shape[-1]), dtype=x.dtype, device=x.device)
    mp = torch.zeros((shape[0] + pad[0], shape[1] + pad[1], shape[2] + pad[2], mask.shape[-1]), dtype=mask.dtype,
                     device=mask.device)
    xp[:shape[0], :shape[1], :shape[2]] = x
    mp[:shape[0], :shape[1], :shape[2]] = mask
    return xp, mp, shape


def augment_axes(spatial_tta=True):
    """the reference's flip list in its order (test.py:95-103), as D/H/W bit masks 4/2/1"""
    if not spatial_tta:
        return [0]
    bit = {1: 4, 2: 2, 3: 1}          # channels_last spatial axes 1,2,3 = D,H,W
    axes = [1, 2, 3]
    out = [7, 0]
    for a in axes:
        pairs = [b for b in axes if b != a]
        out.append(bit[a])
        out.append(bit[pairs[0]] | bit[pairs[1]])
    return out


WINDOW_MODES = ('gaussian', 'constant')


def _finish_of(targets, model=None):
    """the probabilities -> (masked probabilities, label map) call of a target encoding: ops.tta_finish | ops.region_finish"""
    if targets not in TARGETS:
        raise ValueError('unknown targets %r: one of %s' % (targets, TARGETS))
    if targets == 'labels':
        return ops.tta_finish
    if model is not None:
        out_ch = getattr(getattr(model, 'decoder', None), 'out_ch', None)
        if out_ch != 3:
            raise ValueError("targets='regions' reads the output channels as the three BraTS regions WT, TC, ET; the model has "
                             'out_ch = %r' % (out_ch,))
    return ops.region_finish


def _window_axis(extent, window, overlap, mode, sigma_scale):
    """one axis of `window_plan` -> (starts, float64 table (windows, window))"""
    s, r = int(extent), int(window)
    interval = max(1, int(r * (1 - overlap)))
    count = 1 if s <= r else -(-(s - r) // interval) + 1
    starts = [min(i * interval, max(s - r, 0)) for i in range(count)]
    pos = np.arange(r, dtype=np.float64)
    if mode == 'gaussian':
        g = np.exp(-(pos - (r - 1) / 2.0) ** 2 / (2.0 * (float(sigma_scale) * r) ** 2))
    else:
        g = np.ones(r, dtype=np.float64)
    total = np.zeros(max(s, r), dtype=np.float64)         # S_a(p): the importance of every window that covers p
    for st in starts:
        total[st:st + r] += g
    table = np.zeros((count, r), dtype=np.float64)
    for i, st in enumerate(starts):
        inside = min(r, s - st)                           # beyond the volume's end the weight is 0
        table[i, :inside] = g[:inside] / total[st:st + inside]
    return starts, table


def window_plan(shape, roi, overlap=0.5, mode='gaussian', sigma_scale=0.125):
    """the windows of a sliding-window pass over a volume of spatial extent `shape` with windows of extent `roi`
    -> (starts, tables): per axis the list of window starts and a float64 table n[i][r], one row per window, one entry per position.
    Starts (MONAI's rule), with S the extent and R the window: interval = max(1, int(R (1 - overlap))), 1 window when S <= R and
    ceil((S - R) / interval) + 1 otherwise, start_i = min(i interval, max(S - R, 0)): the last window is shifted back to end at the
    volume's end, and a volume shorter than the window gets one window at 0 that hangs over.  Importance: g(r) =
    exp(-(r - (R-1)/2)^2 / (2 (sigma_scale R)^2)) for 'gaussian', 1 for 'constant'; a voxel's weight in a window is gz gy gx.  The windows
    are the Cartesian product of the per-axis starts, so the sum of all windows' weights at a voxel is Sz(z) Sy(y) Sx(x) with S_a(p) =
    sum_i g(p - start_i), and n[i][r] = g(r) / S_a(start_i + r) inside the volume, 0 beyond its end: the weights nz ny nx of all windows
    at any voxel sum to 1.  No weight volume, no division on the device."""
    try:
        roi = tuple(int(r) for r in roi)
    except TypeError:
        roi = ()
    if len(roi) != 3 or min(roi) < 1:
        raise ValueError('window_plan: roi must have three positive entries, got %r' % (roi,))
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError('window_plan: shape must have three positive entries, got %r' % (shape,))
    if not 0 <= overlap < 1:
        raise ValueError('window_plan: overlap must lie in [0, 1), got %r' % (overlap,))
    if mode not in WINDOW_MODES:
        raise ValueError('window_plan: mode must be one of %s, got %r' % (WINDOW_MODES, mode))
    if not sigma_scale > 0:
        raise ValueError('window_plan: sigma_scale must be positive, got %r' % (sigma_scale,))
    axes = [_window_axis(s, r, overlap, mode, sigma_scale) for s, r in zip(shape, roi)]
    return [a[0] for a in axes], [a[1] for a in axes]


class WindowSpec(object):
    """how a TestTimeAugmentor windows a volume: roi (the window, a multiple of the model's spatial resolution per axis), overlap, mode,
    sigma_scale as in `window_plan`; batch: jobs (windows x augmented copies) per forward, None = the augmentor's tta_batch;
    skip_empty: windows without a brain-mask voxel are not run (tta_finish zeroes those voxels anyway)"""

    def __init__(self, roi, overlap=0.5, mode='gaussian', sigma_scale=0.125, batch=None, skip_empty=True):
        window_plan(roi, roi, overlap, mode, sigma_scale)                 # the checks, on a one-window volume
        if batch is not None and int(batch) < 1:
            raise ValueError('WindowSpec: batch must be positive, got %r' % (batch,))
        self.roi = tuple(int(r) for r in roi)
        self.overlap, self.mode, self.sigma_scale = float(overlap), mode, float(sigma_scale)
        self.batch = None if batch is None else int(batch)
        self.skip_empty = bool(skip_empty)

    def check_resolution(self, spatial_res):
        """the network halves every axis `depth` times: a window must be a multiple of the model's spatial resolution"""
        if any(r % int(spatial_res) for r in self.roi):
            raise ValueError('window roi %s must be a multiple of the model\'s spatial resolution %d on every axis' % (self.roi, spatial_res))

    def __repr__(self):
        return 'WindowSpec(roi=%r, overlap=%r, mode=%r, sigma_scale=%r, batch=%r, skip_empty=%r)' % (
            self.roi, self.overlap, self.mode, self.sigma_scale, self.batch, self.skip_empty)


def check_norm(norm):
    """None, or an object with .mode in ('dataset', 'case') and .clip (preprocess.NormSpec)"""
    if norm is not None and getattr(norm, 'mode', None) not in ('dataset', 'case'):
        raise ValueError("norm must be None or a NormSpec with mode 'dataset' or 'case', got %r" % (norm,))


class TestTimeAugmentor(object):
    __test__ = False  # not a pytest class

    def __init__(self, mean, std, model, model_data_format='channels_last', spatial_tta=True, channel_tta=0, threshold=0.5,
                 seed=0, compute_dtype='float32', tta_batch=None, window=None, targets='labels', norm=None):
        """compute_dtype: 'float32' (the engine's parity path) | 'float16' | 'bfloat16' -- 16-bit STORAGE of activations and
        weight images with fp32 sums (bts_amd.lowp; BASELINE configs[4] runs the forwards in fp16)
        targets: 'labels' | 'regions' -- how the mean probabilities are decoded (`_finish_of`); the probabilities do not depend on it
        norm: None | a preprocess.NormSpec (anything with .mode and .clip).  None or mode 'dataset': (x - mean) / std with the statistics
        given here, as the reference.  mode 'case': the volume is normalised on its own voxels inside `bmask` first (ops.case_norm, into
        a new tensor: the caller's x is left as it is) and everything after runs with mean 0 and std 1; `mean` and `std` are not read"""
        check_norm(norm)
        self.norm = norm
        self._finish = _finish_of(targets, model)
        self.targets = targets
        if model_data_format not in ('channels_last', 'channels_first'):
            raise ValueError('unknown data_format %r' % (model_data_format,))
        self.model = model
        cf = model_data_format == 'channels_first'
        if compute_dtype in ('float32', 'fp32', 'f32'):
            # like the reference (test.py:109-117) the volume always ARRIVES channels_last; a channels_first model is fed the
            # transposed view (the engine's memory is NDHWC either way, so the view costs nothing) and answers in its layout
            self._forward = lambda aug: self.model(aug.permute(0, 4, 1, 2, 3) if cf else aug, training=False, inference=True)[0]
        else:
            from .lowp import LowPrecisionForward
            self._forward = LowPrecisionForward(model, compute_dtype)
        self.mean, self.std = mean, std
        self.model_data_format = model_data_format
        self.channel_tta = int(channel_tta)
        self.threshold = float(threshold)
        self.flips = augment_axes(spatial_tta)
        self._gen = torch.Generator().manual_seed(seed)
        # The augmented copies are independent forwards (test.py:128-134 runs them one by one): `tta_batch` of them go through the
        # network as one batch.  16-bit storage, 160x192x160: 150.6 volumes/s at batch 1, 164.9 at 2, 180.2 at 4, 185.1 at 8 (the
        # deep levels of a single volume leave part of the chip idle); default 4 there, 1 for the fp32 parity path
        if tta_batch is None:
            tta_batch = 1 if compute_dtype in ('float32', 'fp32', 'f32') else 4
        self.tta_batch = max(1, int(tta_batch))
        # window: a WindowSpec -> the volume is predicted in windows of that extent, blended by their importance (`_call_windowed`);
        # None: the whole volume per forward, as the reference does.  After a windowed call `window_counts` = (run, skipped).
        self.window = window
        self.window_counts = None
        self._lowp = compute_dtype not in ('float32', 'fp32', 'f32')

    def _dev(self, t, like):
        return torch.as_tensor(t, dtype=torch.float32).reshape(-1).to(like.device).contiguous()

    def _normalised(self, x, bmask):
        """-> (x, mean, std) the rest of a call works with: in case mode the case-normalised volume and the identity"""
        if self.norm is None or self.norm.mode != 'case':
            return x, self.mean, self.std
        c = x.shape[-1]
        xn, _ = ops.case_norm(x.to(torch.float32), bmask.to(torch.float32), self.norm.clip)
        return xn, np.zeros(c), np.ones(c)

    def __call__(self, x, bmask):
        """x: (D,H,W,C) raw intensities, bmask: (D,H,W,1) -> masked mean probability map (D,H,W,out_ch)"""
        if self.window is not None:
            return self._call_windowed(x, bmask)
        x, mean, std = self._normalised(x, bmask)
        xs = x.unsqueeze(0).contiguous()
        mean, std = self._dev(mean, xs), self._dev(std, xs)
        acc = None
        count = len(self.flips) * (1 + self.channel_tta)
        sig = None
        if self.channel_tta:
            xn = ops.flip_affine(xs, 0, mean, std)
            _, var = ops.channel_moments(xn[0])                                     # tf.nn.moments over the spatial axes
            sig = torch.sqrt(var)
        jobs = []                       # (flip, shift, scale) of every augmented copy, in the reference's order
        for flip in self.flips:
            jobs.append((flip, None, None))
            for _ in range(self.channel_tta):
                c = xs.shape[-1]
                shift = (torch.rand(c, generator=self._gen) * 0.2 - 0.1).to(xs.device) * sig
                scale = (torch.rand(c, generator=self._gen) * 0.2 + 0.9).to(xs.device)
                jobs.append((flip, shift, scale))
        for j0 in range(0, len(jobs), self.tta_batch):
            chunk = jobs[j0:j0 + self.tta_batch]
            aug = torch.empty((len(chunk),) + tuple(xs.shape[1:]), dtype=torch.float32, device=xs.device)
            for i, (flip, shift, scale) in enumerate(chunk):
                if shift is None:
                    ops.flip_affine(xs, flip, mean, std, out=aug[i:i + 1])          # normalise + tf.reverse in one pass
                else:  # (x_norm + shift*sigma)*scale == (x - (mean - shift*sigma*std)) / (std / scale)
                    ops.flip_affine(xs, flip, (mean - shift * std).contiguous(), (std / scale).contiguous(), out=aug[i:i + 1])
            y = self._forward(aug)
            yt = (y.t if isinstance(y, Tensor) else y).contiguous()
            for i, (flip, _, _) in enumerate(chunk):
                if acc is None:
                    acc = ops.flip_affine(yt[i:i + 1], flip, scale=1.0 / count)     # un-flip, start the mean
                else:
                    ops.flip_affine(yt[i:i + 1], flip, scale=1.0 / count, out=acc, accumulate=True)
        self._prob = acc
        self._mask = bmask.unsqueeze(0).to(torch.float32).contiguous()
        y, _ = self._finish(acc, self._mask, self.threshold, want_probabilities=True, want_labels=False)
        return y[0].permute(3, 0, 1, 2) if self.model_data_format == 'channels_first' else y[0]   # (test.py:112-114: the model's layout)

    def _call_windowed(self, x, bmask):
        """__call__ with a WindowSpec: every augmented copy of every window is a job; jobs go through the network `batch` at a time
        (gather -> forward -> accumulate), weighted by the normalised importance tables, so `acc` ends as the blended mean"""
        spec = self.window
        x, mean, std = self._normalised(x, bmask)
        xv = x.to(torch.float32).contiguous()
        mask = bmask.to(torch.float32).contiguous()
        dev, c = xv.device, xv.shape[-1]
        roi = spec.roi
        starts, tables = window_plan(tuple(xv.shape[:3]), roi, spec.overlap, spec.mode, spec.sigma_scale)
        tables = [torch.from_numpy(t.astype(np.float32)).to(dev) for t in tables]
        wins = [(iz, iy, ix) for iz in range(len(starts[0])) for iy in range(len(starts[1])) for ix in range(len(starts[2]))]
        run = wins
        if spec.skip_empty:
            occ = ops.window_occupancy(mask, roi, starts).cpu().numpy()              # the one read of the counts
            run = [w for w in wins if occ[w] > 0]
        self.window_counts = (len(run), len(wins) - len(run))
        mean = torch.as_tensor(mean, dtype=torch.float32).reshape(-1).cpu()        # the job table is built on the host
        std = torch.as_tensor(std, dtype=torch.float32).reshape(-1).cpu()
        sig = None
        if self.channel_tta:                          # the deviation of the WHOLE normalised volume, read once; one draw per copy
            xn = ops.flip_affine(xv.unsqueeze(0), 0, mean.to(dev).contiguous(), std.to(dev).contiguous())
            sig = torch.sqrt(ops.channel_moments(xn[0])[1]).cpu()
        copies = []                                   # (flip, mean, std) of every augmented copy, in the reference's order
        for flip in self.flips:
            copies.append((flip, mean.tolist(), std.tolist()))
            for _ in range(self.channel_tta):
                shift = (torch.rand(c, generator=self._gen) * 0.2 - 0.1) * sig
                scale = torch.rand(c, generator=self._gen) * 0.2 + 0.9
                copies.append((flip, (mean - shift * std).tolist(), (std / scale).tolist()))
        count = len(copies)
        jobs = [(w, cp) for w in run for cp in copies]
        batch = min(self.tta_batch if spec.batch is None else spec.batch, ops.window_batch_max())
        cf = self.model_data_format == 'channels_first'
        aug = torch.empty((min(batch, len(jobs)),) + roi + (c,), dtype=torch.float32, device=dev) if jobs else None
        acc = None
        for j0 in range(0, len(jobs), batch):
            chunk = jobs[j0:j0 + batch]
            at = [tuple(starts[a][w[a]] for a in range(3)) for w, _ in chunk]
            flips = [cp[0] for _, cp in chunk]
            ops.window_gather(xv, roi, at, flips, [cp[1] for _, cp in chunk], [cp[2] for _, cp in chunk], out=aug[:len(chunk)])
            if self._lowp:
                y = self._forward(aug[:len(chunk)].permute(0, 4, 1, 2, 3) if cf else aug[:len(chunk)])
                y = y.permute(0, 2, 3, 4, 1) if cf else y
            else:
                y = self._forward(aug[:len(chunk)])
            yt = (y.t if isinstance(y, Tensor) else y).contiguous()
            if acc is None:
                acc = torch.zeros(tuple(xv.shape[:3]) + (yt.shape[-1],), dtype=torch.float32, device=dev)
            ops.window_accumulate(yt, acc, tables, at, flips, [w for w, _ in chunk], scale=1.0 / count)
        if acc is None:                               # every window empty: the mask is zero everywhere, and so is the result
            out_ch = getattr(getattr(self.model, 'decoder', None), 'out_ch', None)
            acc = torch.zeros(tuple(xv.shape[:3]) + (int(out_ch),), dtype=torch.float32, device=dev)
        acc = acc.unsqueeze(0)
        self._prob = acc
        self._mask = mask.unsqueeze(0)
        y, _ = self._finish(acc, self._mask, self.threshold, want_probabilities=True, want_labels=False)
        return y[0].permute(3, 0, 1, 2) if self.model_data_format == 'channels_first' else y[0]

    def labels(self):
        """uint8 label map (D,H,W) of the last call: argmax+1, >=3 -> 4, 0 = background / masked / below threshold; with
        targets='regions' 4 where et >= threshold, else 1 where tc, else 2 where wt, else 0"""
        _, lab = self._finish(self._prob, self._mask, self.threshold, want_probabilities=False, want_labels=True)
        return lab[0]


def segment_volume(model, x, mask, mean, std, spatial_res, spatial_tta=True, threshold=0.5, compute_dtype='float32', tta_batch=None,
                   window=None, targets='labels', norm=None):
    """test.py:246-261 for one volume: pad to the model's spatial resolution, TTA inference, crop back.
    x (D,H,W,C), mask (D,H,W,1) channels_last (test.py:109) -> (probabilities, uint8 labels (D,H,W)); the probabilities are
    (D,H,W,out_ch), or (out_ch,D,H,W) for a model built with data_format='channels_first'.  window: a WindowSpec -> the padded volume
    is predicted in blended windows of that extent; targets: 'labels' | 'regions', the decode of the label map (TestTimeAugmentor);
    norm: None | a NormSpec, how the volume is normalised (TestTimeAugmentor); in case mode over the voxels of `mask`.
    model may be a StageEnsemble: its members carry their own statistics and settings, so of the other arguments only x, mask, window
    and norm are read, and the probabilities are the members' mean, channels last"""
    ensemble = isinstance(model, StageEnsemble)
    if ensemble:
        spatial_res = model.spatial_res
    if window is not None:
        window.check_resolution(spatial_res)
    xp, mp, orig = pad_to_spatial_res(spatial_res, x, mask)
    df = getattr(model, 'data_format', 'channels_last')
    tta = model.augmentor(window, norm) if ensemble else TestTimeAugmentor(
        mean, std, model, df, spatial_tta=spatial_tta, threshold=threshold, compute_dtype=compute_dtype, tta_batch=tta_batch, window=window,
        targets=targets, norm=norm)
    y = tta(xp, mp)
    lab = tta.labels()
    y = y[:, :orig[0], :orig[1], :orig[2]] if df == 'channels_first' else y[:orig[0], :orig[1], :orig[2]]
    return y, lab[:orig[0], :orig[1], :orig[2]]


def zoom_output_shape(shape, factors):
    """spatial extent scipy.ndimage.zoom gives: int(round(n * factor)) per axis, Python's round (ties to even)"""
    return tuple(int(round(int(n) * float(f))) for n, f in zip(shape, factors))


class Interpolator(object):
    """test.py:15-72 on the device: resample a scan to 1 mm^3 (cubic spline, reflect boundary), build the brain mask, and bring
    the prediction back to the scan's own grid"""

    def __init__(self, modalities, order=3, mode='reflect'):
        if mode != 'reflect':
            raise ValueError("Interpolator: mode %r is not supported; the only supported boundary mode is 'reflect'" % (mode,))
        if order not in (0, 1, 3):
            raise ValueError('Interpolator: order %r is not supported; supported spline orders are 0, 1 and 3' % (order,))
        self.modalities = modalities
        self.order = order
        self.mode = mode
        self.pixdim = None          # after __call__: mean of pixdim[0:4] over the modalities (test.py:41)
        self.affine = None          # after __call__: mean 4x4 affine of the srows (test.py:42)
        self.factors = None         # (dx,dy,dz) of the last resample
        self.native_shape = None    # spatial extent of the last resampled scan
        self.mask = None            # unpadded brain mask of the last resample, on the 1 mm^3 grid

    @staticmethod
    def _device_volume(image):
        if isinstance(image, np.ndarray):
            if not torch.cuda.is_available():
                raise RuntimeError('Interpolator: resampling runs on the GPU (no CPU fallback exists for the product path)')
            image = torch.from_numpy(np.ascontiguousarray(image, dtype=np.float32)).cuda()
        if image.dim() != 4:
            raise ValueError('Interpolator: image must be (D,H,W,C), got shape %s' % (tuple(image.shape),))
        return image.to(torch.float32).contiguous()

    def _zoom(self, x, out_shape, order, pad_to=None, want_mask=False):
        coef = ops.spline_prefilter3d(x) if order == 3 else x
        return ops.zoom3d(coef, out_shape, order=order, pad_to=pad_to, want_mask=want_mask)

    def resample(self, image, pixdim, pad_res=None):
        """image (D,H,W,C) numpy or device tensor, pixdim (dx,dy,dz) -> (image_1mm, mask (.., 1)) on the device; with pad_res
        -> (image_padded, mask_padded, orig_shape) by the reference's padding rule (pad_to_spatial_res: a full extra block when
        the extent is already a multiple).  All-ones pixdim skips the resample (test.py:45): mask and padding only."""
        x = self._device_volume(image)
        factors = tuple(float(v) for v in pixdim)
        if len(factors) != 3:
            raise ValueError('Interpolator: pixdim must be (dx,dy,dz), got %r' % (pixdim,))
        self.factors = factors
        self.native_shape = tuple(x.shape[:3])
        unit = all(f == 1.0 for f in factors)
        shape = self.native_shape if unit else zoom_output_shape(self.native_shape, factors)
        pad_to = None if pad_res is None else tuple(s + pad_res - (s % pad_res) for s in shape)
        y, m = self._zoom(x, shape, 0 if unit else self.order, pad_to=pad_to, want_mask=True)   # order 0 onto the same grid: a copy
        self.mask = m if pad_to is None else m[:shape[0], :shape[1], :shape[2]]
        if pad_res is None:
            return y, m
        return y, m, list(shape)

    def __call__(self, path, pad_res=None):
        """test.py:21-56: load *name*.nii* per modality, average pixdim / affine over the modalities, resample"""
        from . import nifti
        image, pixdim, affine = [], [], []
        for name in self.modalities:
            cards = sorted(glob.glob(os.path.join(path, '*' + name + '*' + '.nii' + '*')))
            if not cards:
                raise FileNotFoundError('Interpolator: no *%s*.nii* under %s' % (name, path))
            data, header = nifti.load(cards[0])
            image.append(np.asarray(data).astype(np.float32))
            pixdim.append(header['pixdim'][:4])
            affine.append(header['affine'])
        self.pixdim = np.mean(pixdim, axis=0, dtype=np.float32)
        self.affine = np.mean(affine, axis=0, dtype=np.float32)
        return self.resample(np.stack(image, axis=-1), self.pixdim[1:4], pad_res=pad_res)

    def reverse(self, prob, mask=None, path=None, threshold=0.5, targets='labels', extra=None, native=False):
        """prob (D1,H1,W1,K): cropped probability map on the 1 mm^3 grid, mask (D1,H1,W1,1) (default: the last resample's)
        -> (probabilities (D,H,W,K), uint8 labels (D,H,W)) on the scan's native grid; with `path`, writes mask.nii there
        (test.py:69-70) with the affine averaged in __call__ (identity if the scan came through resample()).  targets: 'labels' (the
        arg-max of bts_tta_finish) | 'regions' (K == 3, the decode of bts_region_finish), taken on the native grid either way.
        extra: one more (D1,H1,W1,J) volume that rides the same way back at order 1 (a variance: linear interpolation keeps it inside
        its range); with it, or with native=True, a third value is returned: (the probabilities before the mask multiplies them, the
        mask (D,H,W,1), extra or None), all on the native grid"""
        finish = _finish_of(targets)
        if self.native_shape is None:
            raise RuntimeError('Interpolator.reverse: no scan has been resampled yet')
        mask = self.mask if mask is None else mask
        p = prob.to(torch.float32).contiguous()
        m = mask.to(torch.float32).contiguous()
        e = None if extra is None else extra.to(torch.float32).contiguous()
        if not all(f == 1.0 for f in self.factors):
            p = self._zoom(p, self.native_shape, self.order)
            m = self._zoom(m, self.native_shape, 0)
            e = None if e is None else self._zoom(e, self.native_shape, 1)
        y, lab = finish(p.unsqueeze(0), m.unsqueeze(0), threshold)
        y, lab = y[0], lab[0]
        if path is not None:
            from . import nifti
            nifti.save(os.path.join(path, 'mask.nii'), lab.cpu().numpy(), np.eye(4) if self.affine is None else self.affine)
        return (y, lab, (p, m, e)) if native or extra is not None else (y, lab)


def _grid_corners(shape):
    """the 8 corner voxels of a grid, homogeneous: (4, 8) float64"""
    n = [float(int(v) - 1) for v in shape]
    return np.array([[a, b, c, 1.0] for a in (0.0, n[0]) for b in (0.0, n[1]) for c in (0.0, n[2])], dtype=np.float64).T


def _corner_shift(m_a, m_b, shape):
    """the largest displacement, in source voxels along any axis, between two 3x4 voxel maps over the corners of a grid"""
    c = _grid_corners(shape)
    return float(np.abs(np.asarray(m_a)[:3] @ c - np.asarray(m_b)[:3] @ c).max())


IDENTITY_REORIENTATION = ((0, 1, 2), (False, False, False))


def signed_permutation(matrix, src_shape, out_shape, entry_tol=1e-6, corner_tol=1e-3):
    """is the 3x4 voxel map output grid -> source grid an exact reorientation of the whole source array?  Every row of the 3x3 part one
    entry within entry_tol of +-1 and the others within it of 0, the extents matching, and the map within corner_tol voxel of the
    reorientation's own (translation 0, or n - 1 on a reversed axis) at the corners of the output grid -> (perm, flip) as
    ops.reorient3d takes them, else None"""
    m = np.asarray(matrix, dtype=np.float64)[:3]
    lin = m[:, :3]
    perm, flip, exact = [None] * 3, [False] * 3, np.zeros((3, 4), dtype=np.float64)
    for b in range(3):                                   # source axis b is fed by output axis a
        a = int(np.argmax(np.abs(lin[b])))
        rest = [k for k in range(3) if k != a]
        if abs(abs(lin[b, a]) - 1.0) > entry_tol or np.abs(lin[b, rest]).max() > entry_tol or perm[a] is not None:
            return None
        perm[a], flip[a] = b, bool(lin[b, a] < 0)
        exact[b, a] = -1.0 if flip[a] else 1.0
        exact[b, 3] = float(int(src_shape[b]) - 1) if flip[a] else 0.0
    if any(int(out_shape[a]) != int(src_shape[perm[a]]) for a in range(3)):
        return None
    if _corner_shift(m, exact, out_shape) > corner_tol:
        return None
    return tuple(perm), tuple(flip)


class Conformer(object):
    """brings the modalities of a scan onto ONE grid of a stated orientation and spacing by their affines, on the device, and the
    prediction back onto the first modality's own grid.

    The reference grid is the first modality's.  The target keeps that scan's own axes -- permuted and reversed to the closest
    `orientation` (nifti.orientation / nifti.reorientation), each rescaled to `spacing` -- and is not rotated to the scanner's axes, so an
    oblique scan is not resliced through its field of view.  Extent per axis int(round(n * src_spacing / spacing)) (zoom_output_shape);
    the outer faces of the two volumes coincide: source coordinate s = (o + 0.5) * (spacing / src_spacing) - 0.5.  Every modality c is
    read through M_c = inv(A_c) @ target_affine, so modalities on other grids land where their affines say; what lies outside a
    modality's field of view is 0."""

    def __init__(self, orientation='LPS', spacing=(1.0, 1.0, 1.0), order=3):
        from . import nifti
        nifti.reorientation(orientation, orientation)                         # refuses a code that is none
        if order not in (0, 1, 3):
            raise ValueError('Conformer: order %r is not supported; supported spline orders are 0, 1 and 3' % (order,))
        spacing = tuple(float(v) for v in spacing)
        if len(spacing) != 3 or not all(np.isfinite(v) and v > 0 for v in spacing):
            raise ValueError('Conformer: spacing must be three positive numbers, got %r' % (spacing,))
        self.orientation, self.spacing, self.order = str(orientation), spacing, int(order)
        self.last = None            # after forward: the plan of the last scan
        self.affine = None          # the reference modality's affine (mask.nii is written with it)
        self.native_shape = None    # the reference modality's extent
        self.mask = None            # unpadded brain mask of the last forward, on the target grid

    def plan(self, shapes, affines):
        """host only, float64.  shapes: the (D,H,W) of every modality's array, affines: their 4x4 voxel -> world matrices
        -> {'shape': the target extent, 'target_affine' (4,4), 'voxel_map' (4,4): target voxel -> reference voxel, 'matrices': one 3x4
        target voxel -> source voxel map per modality, 'groups': lists of modality indices that share a map (within 1e-3 voxel at the
        corners of the target grid) and a source extent, 'reorient': per group (perm, flip) where the map is an exact reorientation
        (`signed_permutation`), else None, 'code': the reference's own orientation code, 'native_spacing': its voxel size per axis,
        'shapes': the extents as given}"""
        from . import nifti
        shapes = [tuple(int(v) for v in sh) for sh in shapes]
        affines = [np.asarray(a, dtype=np.float64) for a in affines]
        if not shapes or len(shapes) != len(affines) or any(len(sh) != 3 or min(sh) < 1 for sh in shapes) \
                or any(a.shape != (4, 4) for a in affines):
            raise ValueError('Conformer.plan: one (D,H,W) extent and one 4x4 affine per modality, got %r and %r'
                             % (shapes, [a.shape for a in affines]))
        a0, n0 = affines[0], shapes[0]
        code = nifti.orientation(a0)
        perm, flip = nifti.reorientation(code, self.orientation)
        native = np.sqrt((a0[:3, :3] ** 2).sum(axis=0))
        shape = zoom_output_shape([n0[perm[a]] for a in range(3)], [native[perm[a]] / self.spacing[a] for a in range(3)])
        if min(shape) < 1:
            raise ValueError('Conformer.plan: extent %s at spacing %s leaves the empty target %s' % (n0, tuple(native), shape))
        vmap = np.zeros((4, 4), dtype=np.float64)
        vmap[3, 3] = 1.0
        for a in range(3):
            k = self.spacing[a] / native[perm[a]]
            if abs(k - 1.0) <= 1e-6:          # the column norm of float32 srows: the same spacing, and then an exactly integer map
                k = 1.0
            start = 0.5 * k - 0.5
            vmap[perm[a], a] = -k if flip[a] else k
            vmap[perm[a], 3] = (n0[perm[a]] - 1) - start if flip[a] else start
        target = a0 @ vmap
        mats = [vmap[:3].copy() if c == 0 or np.array_equal(a, a0) else (np.linalg.inv(a) @ target)[:3] for c, a in enumerate(affines)]
        groups = []
        for c, m in enumerate(mats):
            for g in groups:
                if shapes[g[0]] == shapes[c] and _corner_shift(mats[g[0]], m, shape) <= 1e-3:
                    g.append(c)
                    break
            else:
                groups.append([c])
        return {'shape': tuple(shape), 'target_affine': target, 'voxel_map': vmap, 'matrices': mats, 'groups': groups,
                'reorient': [signed_permutation(mats[g[0]], shapes[g[0]], shape) for g in groups], 'code': code,
                'native_spacing': tuple(float(v) for v in native), 'shapes': shapes}

    @staticmethod
    def _runs(group):
        """a group's channels as runs of consecutive indices of at most 8 (one launch each)"""
        runs = []
        for c in group:
            if runs and runs[-1][-1] == c - 1 and len(runs[-1]) < 8:
                runs[-1].append(c)
            else:
                runs.append([c])
        return runs

    @staticmethod
    def _device_stack(vols, run):
        """the volumes `run` names, channels last, dense float32 on the device"""
        out = []
        for c in run:
            v = vols[c]
            if isinstance(v, np.ndarray):
                if not torch.cuda.is_available():
                    raise RuntimeError('Conformer: conforming runs on the GPU (no CPU fallback exists for the product path)')
                v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).cuda()
            if v.dim() != 3:
                raise ValueError('Conformer: every modality must be a (D,H,W) volume, got shape %s' % (tuple(v.shape),))
            out.append(v.to(torch.float32))
        return torch.stack(out, dim=-1).contiguous()

    def _gather(self, x, matrix, shape, order, **kw):
        coef = ops.spline_prefilter3d(x) if order == 3 else x
        return ops.affine_resample3d(coef, matrix, shape, order=order, **kw)

    def forward(self, vols, affines, pad_res=None):
        """vols: one (D,H,W) volume per modality (numpy or device tensors, each on its own grid), affines: their 4x4 matrices
        -> (x (D,H,W,C), mask (D,H,W,1), orig_shape) on the device, on the target grid; with pad_res padded by the reference's rule
        (pad_to_spatial_res, as Interpolator.resample) with orig_shape the unpadded extent.  A group whose map is an exact
        reorientation goes through ops.reorient3d, any other through the prefilter (order 3) and ops.affine_resample3d; mask and padding
        come from the resampling launch where one launch writes every channel, else from one more pass over the finished volume."""
        plan = self.plan([tuple(v.shape) for v in vols], affines)
        self.last, self.affine, self.native_shape = plan, np.asarray(affines[0], dtype=np.float64), plan['shapes'][0]
        shape, nch = plan['shape'], len(vols)
        pad_to = None if pad_res is None else tuple(s + pad_res - (s % pad_res) for s in shape)
        launches = [(run, plan['matrices'][g[0]], ro) for g, ro in zip(plan['groups'], plan['reorient']) for run in self._runs(g)]
        whole = None
        if len(launches) == 1:
            run, matrix, ro = launches[0]
            src = self._device_stack(vols, run)
            if ro is None:
                x, m = self._gather(src, matrix, shape, self.order, pad_to=pad_to, want_mask=True)
            else:
                whole = src if ro == IDENTITY_REORIENTATION else ops.reorient3d(src, *ro)
        else:
            for run, matrix, ro in launches:
                src = self._device_stack(vols, run)
                if whole is None:
                    whole = torch.empty(tuple(shape) + (nch,), dtype=torch.float32, device=src.device)
                if ro is None:
                    self._gather(src, matrix, shape, self.order, out=whole, channel=run[0])
                else:
                    whole[..., run[0]:run[0] + len(run)].copy_(src if ro == IDENTITY_REORIENTATION else ops.reorient3d(src, *ro))
        if whole is not None:
            x, m = ops.zoom3d(whole, shape, order=0, pad_to=pad_to, want_mask=True)        # order 0 onto the same grid: copy, mask, padding
        self.mask = m if pad_to is None else m[:shape[0], :shape[1], :shape[2]]
        return x, m, list(shape)

    @property
    def identity(self):
        """did the reference modality of the last scan already lie on the target grid, array axes included?"""
        return self.last is not None and self.last['reorient'][0] == IDENTITY_REORIENTATION

    def reverse(self, prob, mask=None, path=None, threshold=0.5, targets='labels', extra=None, native=False):
        """prob (D1,H1,W1,K): cropped probability map on the target grid, mask (D1,H1,W1,1) (default: the last forward's)
        -> (probabilities (D,H,W,K), uint8 labels (D,H,W)) on the reference modality's own grid, as Interpolator.reverse: the
        probabilities at the configured order and the mask at order 0 through the inverse map (the exact copy where the forward was a
        reorientation), the labels taken there ('labels' | 'regions'); with `path`, writes mask.nii there with the reference modality's
        own affine.  extra, native: as Interpolator.reverse -- one more volume through the inverse map at order 1 (the exact copy where
        the forward was a reorientation), and the third value (unmasked probabilities, mask, extra or None) on the native grid"""
        finish = _finish_of(targets)
        if self.last is None:
            raise RuntimeError('Conformer.reverse: no scan has been conformed yet')
        mask = self.mask if mask is None else mask
        p = prob.to(torch.float32).contiguous()
        m = mask.to(torch.float32).contiguous()
        e = None if extra is None else extra.to(torch.float32).contiguous()
        ro = self.last['reorient'][0]
        if ro is None:
            inv = np.linalg.inv(self.last['voxel_map'])[:3]
            p = self._gather(p, inv, self.native_shape, self.order)
            m = self._gather(m, inv, self.native_shape, 0)
            e = None if e is None else self._gather(e, inv, self.native_shape, 1)
        elif ro != IDENTITY_REORIENTATION:
            perm, flip = ro
            back = tuple(perm.index(b) for b in range(3))                     # native axis b is the target's axis back[b]
            p = ops.reorient3d(p, back, tuple(flip[a] for a in back))
            m = ops.reorient3d(m, back, tuple(flip[a] for a in back))
            e = None if e is None else ops.reorient3d(e, back, tuple(flip[a] for a in back))
        y, lab = finish(p.unsqueeze(0), m.unsqueeze(0), threshold)
        y, lab = y[0], lab[0]
        if path is not None:
            from . import nifti
            nifti.save(os.path.join(path, 'mask.nii'), lab.cpu().numpy(), self.affine)
        return (y, lab, (p, m, e)) if native or extra is not None else (y, lab)


def _conformed(geometry, pad_res):
    """segment_scan / segment_case with `geometry` = (Conformer, volumes, affines): the forward in place of Interpolator.resample"""
    try:
        conf, vols, affines = geometry
    except (TypeError, ValueError):
        conf = None
    if not isinstance(conf, Conformer):
        raise ValueError('geometry must be (Conformer, one (D,H,W) volume per modality, one 4x4 affine per modality), got %r' % (geometry,))
    return (conf,) + tuple(conf.forward(vols, affines, pad_res=pad_res))


def segment_scan(model, image, pixdim, mean, std, spatial_res, spatial_tta=True, threshold=0.5, compute_dtype='float32', tta_batch=None,
                 order=3, window=None, targets='labels', norm=None, geometry=None):
    """test.py:235-264 for one scan: resample to 1 mm^3 with mask and padding in one pass, TTA inference, crop, resample back.
    image (D,H,W,C) on the scan's grid, pixdim (dx,dy,dz) -> (probabilities, uint8 labels (D,H,W)) on that grid; the probabilities
    are (D,H,W,out_ch), or (out_ch,D,H,W) for a model built with data_format='channels_first'.  With pixdim (1,1,1) this is
    segment_volume with the reference's mask, bit for bit.  window: a WindowSpec, targets: 'labels' | 'regions', norm: None | a NormSpec, as
    in segment_volume (in case mode the voxels of the resampled brain mask).
    geometry: (Conformer, one (D,H,W) volume per modality, their 4x4 affines) -> the Conformer takes the Interpolator's place, forward and
    back; `image`, `pixdim` and `order` are not read, and the result lies on the first modality's own grid.
    model may be a StageEnsemble, as in segment_volume: mean, std, spatial_res and the TTA arguments are then its members' own."""
    ensemble = isinstance(model, StageEnsemble)
    if ensemble:
        spatial_res, threshold, targets = model.spatial_res, model.threshold, model.targets
    if window is not None:
        window.check_resolution(spatial_res)
    if geometry is None:
        interp = Interpolator(None, order=order)
        xp, mp, orig = interp.resample(image, pixdim, pad_res=spatial_res)
        same_grid = all(f == 1.0 for f in interp.factors)
    else:
        interp, xp, mp, orig = _conformed(geometry, spatial_res)
        same_grid = interp.identity
    df = getattr(model, 'data_format', 'channels_last')
    tta = model.augmentor(window, norm) if ensemble else TestTimeAugmentor(
        mean, std, model, df, spatial_tta=spatial_tta, threshold=threshold, compute_dtype=compute_dtype, tta_batch=tta_batch, window=window,
        targets=targets, norm=norm)
    y = tta(xp, mp)
    if same_grid:
        lab = tta.labels()
        y = y[:, :orig[0], :orig[1], :orig[2]] if df == 'channels_first' else y[:orig[0], :orig[1], :orig[2]]
        return y, lab[:orig[0], :orig[1], :orig[2]]
    if df == 'channels_first':
        y = y.permute(1, 2, 3, 0)
    y, lab = interp.reverse(y[:orig[0], :orig[1], :orig[2]], threshold=threshold, targets=targets)
    return (y.permute(3, 0, 1, 2) if df == 'channels_first' else y), lab


class StageSpec(object):
    """one model of the two-stage pipeline with everything its TestTimeAugmentor takes (test.py:185-221).  The augmentor is built
    once and kept: the 16-bit engine packs its weight images on the first forward"""

    def __init__(self, model, mean, std, spatial_res, spatial_tta=True, channel_tta=0, threshold=0.5, compute_dtype='float32',
                 tta_batch=None, largest_component=False, window=None, targets='labels', norm=None):
        """largest_component: for a skull-stripping stage, keep only the largest connected piece of the brain it finds (segment_case);
        window: a WindowSpec -> this stage predicts blended windows of that extent (a multiple of spatial_res per axis);
        targets: 'labels' | 'regions' -- what the tumour model was trained on (train_args.pkl's `targets`), i.e. how segment_case
        decodes its label map; a skull-stripping stage (out_ch == 1) is always 'labels';
        norm: None | a NormSpec (preprocess.load_norm of the stage's prepro.npy) -- how the stage's training examples were normalised, and
        so its input here: None or mode 'dataset' with mean / std, mode 'case' on the scan's own voxels inside the mask the stage is
        handed (TestTimeAugmentor)"""
        check_norm(norm)
        self.norm = norm
        _finish_of(targets, model)
        self.targets = targets
        if window is not None:
            window.check_resolution(spatial_res)
        self.window = window
        self.model, self.mean, self.std = model, mean, std
        self.largest_component = bool(largest_component)
        self.spatial_res = int(spatial_res)
        self.spatial_tta, self.channel_tta, self.threshold = bool(spatial_tta), int(channel_tta), float(threshold)
        self.compute_dtype, self.tta_batch = compute_dtype, tta_batch
        self._tta = None

    @property
    def data_format(self):
        return getattr(self.model, 'data_format', 'channels_last')

    @property
    def window_counts(self):
        """(windows run, windows skipped as empty) of the stage's last windowed call, None before one"""
        return None if self._tta is None else self._tta.window_counts

    def augmentor(self, window=None, norm=None):
        """the stage's TestTimeAugmentor, with the channel-TTA generator back at its seed: every case draws what a fresh augmentor
        would (segment_scan builds one per call).  window: a WindowSpec, norm: a NormSpec for this call in place of the stage's own"""
        check_norm(norm)
        if window is not None:
            window.check_resolution(self.spatial_res)
        if self._tta is not None:
            self._tta._gen.manual_seed(0)
        if self._tta is None:
            self._tta = TestTimeAugmentor(self.mean, self.std, self.model, self.data_format, spatial_tta=self.spatial_tta,
                                          channel_tta=self.channel_tta, threshold=self.threshold, compute_dtype=self.compute_dtype,
                                          tta_batch=self.tta_batch, targets=self.targets)
        self._tta.window = self.window if window is None else window
        self._tta.norm = self.norm if norm is None else norm
        return self._tta


UNCERTAINTY_MODES = ops.UNCERTAINTY_MODES        # ('entropy', 'std')


class EnsembleAugmentor(object):
    """what `StageEnsemble.augmentor` hands out: a TestTimeAugmentor's call and `labels()` over the mean of the members.  After a call
    `_prob` is the unmasked mean probability (1,D,H,W,C) of the members, channels last, `_mask` the brain mask it was called with and,
    in 'std' mode, `_m2` the sum of the members' squared deviations from that mean (ops.ensemble_update)"""

    def __init__(self, ensemble, window=None, norm=None):
        self.ensemble, self.window, self.norm = ensemble, window, norm
        self._finish = _finish_of(ensemble.targets)
        self.threshold, self.targets = ensemble.threshold, ensemble.targets
        self._prob = self._mask = self._m2 = None

    def __call__(self, x, bmask):
        """x: (D,H,W,C) raw intensities, bmask: (D,H,W,1) -> masked mean probability map (D,H,W,out_ch) of the members, channels last.
        Every member runs its own augmentor (its own statistics, NormSpec and window) on the same input; its unmasked mean over the
        augmented copies is folded into the running mean, so one member's volume is held at a time"""
        ens = self.ensemble
        mean = m2 = None
        for k, member in enumerate(ens.members, 1):
            tta = member.augmentor(self.window, self.norm)
            tta(x, bmask)
            p = tta._prob.contiguous()
            if k == 1:
                mean = torch.empty_like(p)
                m2 = torch.empty_like(p) if ens.uncertainty == 'std' else None
            elif tuple(p.shape) != tuple(mean.shape):
                raise ValueError('StageEnsemble: member %d gives probabilities of shape %s, the members before it %s' %
                                 (k - 1, tuple(p.shape), tuple(mean.shape)))
            ops.ensemble_update(p, mean, m2, k)
            self._mask = tta._mask
        self._prob, self._m2 = mean, m2
        y, _ = self._finish(mean, self._mask, self.threshold, want_probabilities=True, want_labels=False)
        return y[0]

    def labels(self):
        """uint8 label map (D,H,W) of the last call, decoded from the members' mean as TestTimeAugmentor.labels decodes one model's"""
        _, lab = self._finish(self._prob, self._mask, self.threshold, want_probabilities=False, want_labels=True)
        return lab[0]

    def uncertainty(self, mean, mask, spread=None):
        """the ensemble's map from a mean (and, in 'std' mode, a VARIANCE) volume and a mask on one grid -> uint8 (D,H,W,C)"""
        if self.ensemble.uncertainty == 'std':
            return ops.uncertainty_finish(mean, mask, 'std', spread=spread, scale=1.0)
        return ops.uncertainty_finish(mean, mask, 'entropy')


class StageEnsemble(object):
    """several tumour models in the place of one StageSpec: the probabilities `segment_case` decodes, resamples and hands back are the
    mean over the members of each member's mean over its augmented copies.  members: a non-empty list of StageSpec that agree in
    spatial_res, decoder out_ch, targets, threshold and compute_dtype (anything else -- statistics, NormSpec, window, data format, TTA
    settings -- is each member's own); uncertainty: None | 'entropy' | 'std', the voxel-wise map `segment_case(return_stages=True)` adds
    as stages['uncertainty']: the binary entropy of the mean per channel, or the population deviation of the members' probabilities
    (two members at least), as levels 0..100 (ops.uncertainty_finish).  The ensemble hands over channels last whatever the members are."""

    data_format = 'channels_last'

    def __init__(self, members, uncertainty=None):
        members = list(members) if isinstance(members, (list, tuple)) else None
        if not members or not all(isinstance(m, StageSpec) for m in members):
            raise ValueError('StageEnsemble: members must be a non-empty list of StageSpec')
        if uncertainty is not None and uncertainty not in UNCERTAINTY_MODES:
            raise ValueError('StageEnsemble: uncertainty must be None or one of %s, got %r' % (UNCERTAINTY_MODES, uncertainty))
        if uncertainty == 'std' and len(members) < 2:
            raise ValueError("StageEnsemble: uncertainty 'std' is the spread between members and needs two at least, got %d" % len(members))

        def facts(m):
            return (('spatial_res', m.spatial_res), ('out_ch', getattr(getattr(m.model, 'decoder', None), 'out_ch', None)),
                    ('targets', m.targets), ('threshold', m.threshold), ('compute_dtype', m.compute_dtype))
        first = facts(members[0])
        for i, m in enumerate(members[1:], 1):
            for (what, a), (_, b) in zip(first, facts(m)):
                if a != b:
                    raise ValueError('StageEnsemble: member %d has %s = %r, member 0 has %r' % (i, what, b, a))
        self.members, self.uncertainty = members, uncertainty
        self.spatial_res, self.out_ch, self.targets, self.threshold, self.compute_dtype = (v for _, v in first)
        self._tta = None

    @property
    def window_counts(self):
        """(windows run, windows skipped as empty) summed over the members' last windowed calls, None where none was windowed"""
        counts = [m.window_counts for m in self.members if m.window_counts is not None]
        return (sum(c[0] for c in counts), sum(c[1] for c in counts)) if counts else None

    def augmentor(self, window=None, norm=None):
        """the ensemble's EnsembleAugmentor; window, norm: for this call in place of every member's own, as StageSpec.augmentor"""
        check_norm(norm)
        if window is not None:
            window.check_resolution(self.spatial_res)
        self._tta = EnsembleAugmentor(self, window, norm)
        return self._tta


def remove_components(lab, class_mask, K=4, connectivity=26, min_voxels=0, largest_only=False, fill=0):
    """clean one region of a dense uint8 label map (D,H,W) on the GPU, IN PLACE: the region (classes min(label, K-1) whose bit is set in
    class_mask) is split into its connected components (6 | 18 | 26 neighbours), and every voxel of a component of fewer than
    `min_voxels` voxels, or with `largest_only` of any component but the largest (the one that starts first among equals), becomes `fill`
    -> {'components': found, 'removed_components', 'removed_voxels'}.  On the device: bts_components3d, bts_component_sizes,
    bts_component_largest, bts_components_apply; one host read at the end."""
    comp = ops.components3d(lab, class_mask, K, connectivity)
    size, count = ops.component_sizes(comp)
    key = ops.component_largest(size) if largest_only else None
    removed = ops.components_apply(lab, comp, size, key, min_voxels, largest_only, fill)
    found, vox, gone = torch.cat([count, removed]).cpu().tolist()                    # the one read
    return {'components': int(found), 'removed_components': int(gone), 'removed_voxels': int(vox)}


BRATS_WT_MASK, BRATS_ET_MASK = 0b1110, 0b1000       # class masks over min(label, 3)


def postprocess_labels(lab, min_component_voxels=0, et_min_voxels=0, connectivity=26):
    """the usual cleaning of a BraTS label map (values 0, 1, 2, 4; dense uint8 (D,H,W) on the GPU), IN PLACE:
    (a) with min_component_voxels > 0, connected components of the whole tumour (labels 1, 2, 4 together) of fewer voxels become 0;
    (b) then, with et_min_voxels > 0, an enhancing tumour (label 4) of 1 .. et_min_voxels - 1 voxels in all becomes label 1 (necrotic
        core), so that a case without enhancing tumour is not scored on a few stray voxels.
    -> {'components', 'removed_components', 'removed_voxels', 'et_relabelled'}; with both parameters 0 nothing is launched."""
    if min_component_voxels < 0 or et_min_voxels < 0:
        raise ValueError('postprocess_labels: the voxel counts must not be negative, got %r and %r' % (min_component_voxels, et_min_voxels))
    out = {'components': 0, 'removed_components': 0, 'removed_voxels': 0, 'et_relabelled': 0}
    if min_component_voxels > 0:
        out.update(remove_components(lab, BRATS_WT_MASK, 4, connectivity, min_voxels=min_component_voxels))
    if et_min_voxels > 0:
        out['et_relabelled'] = int(ops.region_relabel(lab, BRATS_ET_MASK, 1, et_min_voxels, K=4).item())
    return out


def segment_case(tumor, image, pixdim, skull=None, order=3, return_stages=False, postprocess=None, window=None, norm=None, geometry=None):
    """test.py:235-264 for one scan, with the optional skull-stripping stage (test.py:238-248): resample to 1 mm^3 padded to the first
    model's resolution, [skull model with TTA, x * (1 - p) cropped and padded again to the tumour model's resolution,] tumour model
    with TTA, crop, resample back.  tumor, skull: StageSpec; image (D,H,W,C) on the scan's grid, pixdim (dx,dy,dz)
    -> (probabilities, uint8 labels (D,H,W)) on that grid, as segment_scan gives them; without `skull` this IS segment_scan.
    return_stages: also a dict of the device tensors each stage handed to the next -- 'x1mm', 'mask' (padded to the first model's
    resolution), 'skull_prob' (masked mean probability, same extent), 'x_stripped', 'mask_repadded' (padded to the tumour model's
    resolution), 'prob_1mm' (the tumour model's cropped probabilities on the 1 mm^3 grid, channels last); None where a stage did not run.
    A skull stage with `largest_component` set: the candidate brain, (mask > 0) & (p < threshold) on the padded 1 mm^3 grid, is reduced
    to its largest 26-connected component (eye sockets, neck fragments go), and p is set to 1 at the candidates outside it before the
    hand-over; 'brain_kept' is that uint8 map, 'brain_counts' remove_components' counts; 'skull_prob' stays the stage's own output.
    postprocess: keyword arguments of `postprocess_labels`, applied to the labels on the scan's own grid (the returned probabilities
    are unchanged); 'postprocess' holds its counts.  These three keys exist only where their option is on (`stages.get(key)` is None
    otherwise): with the options off the dict is the one callers have always got, every value of a two-stage call a tensor.
    window: each stage predicts in windows when its StageSpec carries a WindowSpec; a WindowSpec given here takes the place of both
    stages' own for this call (checked against each stage's resolution).  After the call `stage.window_counts` is (windows run,
    windows skipped as empty) of that stage.
    norm: each stage normalises its input as its StageSpec's NormSpec says; a NormSpec given here takes the place of both stages' own for
    this call.  In case mode a stage normalises into a tensor of its own over the mask it is handed ('mask' for the first stage,
    'mask_repadded' for the tumour stage after skull stripping): 'x1mm' and 'x_stripped' stay the raw intensities, which is what
    ops.skull_strip multiplies.
    geometry: (Conformer, one (D,H,W) volume per modality, their 4x4 affines) -> the Conformer takes the Interpolator's place for the forward
    and the reverse: `image`, `pixdim` and `order` are not read, 'x1mm' is the conformed scan, and probabilities and labels lie on the
    first modality's own grid.  None: as before.
    tumor may be a StageEnsemble: its members' mean probabilities take the place of one model's, everything after is the same.  One built
    with `uncertainty` adds two keys: 'uncertainty', uint8 (D,H,W,C) levels 0..100 on the scan's own grid, channels last, 0 outside the
    brain mask, and 'uncertainty_mask', that mask (D,H,W,1) float32.  Where the scan was resampled the mean goes back at the configured
    order and the mask at order 0, as for the labels, in 'std' mode the members' variance m2 / M rides the same inverse map at order 1, and
    ops.uncertainty_finish runs on the native grid.  Post-processing changes the labels only, never the map."""
    if window is not None:
        for stage in (tumor, skull):
            if stage is not None:
                window.check_resolution(stage.spatial_res)
    if skull is not None:
        out_ch = getattr(getattr(skull.model, 'decoder', None), 'out_ch', None)
        if out_ch != 1:
            raise ValueError('segment_case: the skull-stripping model must have out_ch == 1 (its probability multiplies every channel '
                             'of the scan, test.py:245), got out_ch = %r' % (out_ch,))
    first = tumor if skull is None else skull
    if geometry is None:
        interp = Interpolator(None, order=order)
        xp, mp, orig = interp.resample(image, pixdim, pad_res=first.spatial_res)
        same_grid = all(f == 1.0 for f in interp.factors)
    else:
        interp, xp, mp, orig = _conformed(geometry, first.spatial_res)
        same_grid = interp.identity
    stages = {'x1mm': xp, 'mask': mp, 'skull_prob': None, 'x_stripped': None, 'mask_repadded': None, 'prob_1mm': None}
    if skull is not None:
        p = skull.augmentor(window, norm)(xp, mp)
        if skull.data_format == 'channels_first':
            p = p.permute(1, 2, 3, 0)
        p = p.contiguous()
        stages['skull_prob'] = p
        if skull.largest_component:
            cand = ((mp > 0) & (p < skull.threshold)).to(torch.uint8).reshape(tuple(p.shape[:3]))
            kept = cand.clone()
            stages['brain_counts'] = remove_components(kept, 2, K=2, connectivity=26, largest_only=True, fill=0)
            stages['brain_kept'] = kept
            p = torch.where((cand != kept).unsqueeze(-1), torch.ones_like(p), p).contiguous()
        res = tumor.spatial_res
        xp, mp = ops.skull_strip(xp, p, mp, orig, tuple(s + res - (s % res) for s in orig))
        stages.update(x_stripped=xp, mask_repadded=mp)
    df = tumor.data_format
    tta = tumor.augmentor(window, norm)
    y = tta(xp, mp)
    if df == 'channels_first':
        y = y.permute(1, 2, 3, 0)
    y = y[:orig[0], :orig[1], :orig[2]]
    stages['prob_1mm'] = y
    mode = getattr(tumor, 'uncertainty', None)                       # a StageEnsemble that was asked for its map
    if mode is None:
        if same_grid:
            lab = tta.labels()[:orig[0], :orig[1], :orig[2]]
        else:
            y, lab = interp.reverse(y, threshold=tumor.threshold, targets=tumor.targets)
    else:
        var = None
        if mode == 'std':                                            # the population variance of the members, on the 1 mm^3 grid
            var = (tta._m2[0, :orig[0], :orig[1], :orig[2]] * (1.0 / len(tumor.members))).contiguous()
        if same_grid:
            lab = tta.labels()[:orig[0], :orig[1], :orig[2]]
            mean = tta._prob[0, :orig[0], :orig[1], :orig[2]].contiguous()
            mask = tta._mask[0, :orig[0], :orig[1], :orig[2]].contiguous()
        else:                                                        # the map is taken where the labels are: on the scan's own grid
            y, lab, (mean, mask, var) = interp.reverse(y, threshold=tumor.threshold, targets=tumor.targets, extra=var, native=True)
        stages['uncertainty'] = tta.uncertainty(mean, mask, var)
        stages['uncertainty_mask'] = mask
    if postprocess is not None:
        lab = lab.contiguous()
        stages['postprocess'] = postprocess_labels(lab, **postprocess)
    if df == 'channels_first':
        y = y.permute(3, 0, 1, 2)
    return (y, lab, stages) if return_stages else (y, lab)


def scores_from_confusion(confusion):
    """K x K counts [truth class, predicted class] -> the scores of `label_scores`, float64 arithmetic on the host"""
    m = np.asarray(confusion)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2:
        raise ValueError('confusion must be K x K with K >= 2, got shape %s' % (m.shape,))
    m = m.astype(np.int64)
    k = m.shape[0]

    def dice(sel):                   # 2 I / (P + T) of the union of the classes `sel`; nan when truth and prediction are both empty
        inter, t, p = int(m[np.ix_(sel, sel)].sum()), int(m[sel, :].sum()), int(m[:, sel].sum())
        return 2.0 * inter / (p + t) if p + t else float('nan')

    inter = np.diag(m)[1:].astype(np.float64)
    true, pred = m.sum(axis=1)[1:].astype(np.float64), m.sum(axis=0)[1:].astype(np.float64)
    out = {'confusion': m,
           'macro': float(np.mean((2.0 * inter + 1.0) / (pred + true + 1.0))),                       # util.py:54
           'micro': float(inter.sum() / (pred.sum() + true.sum())) if pred.sum() + true.sum() else float('nan'),   # util.py:55
           'dice': [dice([c]) for c in range(1, k)]}
    if k == 4:                       # BraTS regions over labels {1,2,4} = classes {1,2,3}
        out.update(wt=dice([1, 2, 3]), tc=dice([1, 3]), et=dice([3]))
    return out


def label_scores(truth, pred, n_classes=4):
    """per-class Dice between two uint8 label maps of equal shape (device tensors or numpy) -> {'confusion' (K,K) int64 numpy,
    'macro', 'micro', 'dice' [class 1..K-1], and for n_classes == 4 'wt', 'tc', 'et'}.  Labels >= K-1 count as class K-1 (BraTS 4 -> 3,
    preprocess.py:36).  macro = mean_c (2 I_c + 1) / (P_c + T_c + 1) and micro = sum I / (sum P + sum T) over classes 1..K-1 are
    util.py:54-55 on the one-hot of the two maps with the background dropped (train.py:39-41), the missing factor 2 of micro included;
    dice[c] = 2 I / (P + T), nan when both are empty; wt / tc / et: the same over labels {1,2,4} / {1,4} / {4}."""
    if tuple(truth.shape) != tuple(pred.shape):
        raise ValueError('label_scores: truth has shape %s, the prediction %s' % (tuple(truth.shape), tuple(pred.shape)))
    maps = []
    for t in (truth, pred):
        if isinstance(t, np.ndarray):
            if t.dtype != np.uint8:
                raise ValueError('label_scores: label maps must be uint8, got %s' % t.dtype)
            if not torch.cuda.is_available():
                raise RuntimeError('label_scores: the confusion matrix is counted on the GPU (no CPU fallback exists for the product path)')
            t = torch.from_numpy(np.ascontiguousarray(t)).cuda()
        maps.append(t.contiguous())
    counts = ops.label_confusion(maps[0], maps[1], n_classes)
    return scores_from_confusion(counts.cpu().numpy())


BRATS_REGIONS = (('wt', (1, 2, 3)), ('tc', (1, 3)), ('et', (3,)))      # over classes min(label, 3): labels {1,2,4} / {1,4} / {4}


def region_rates_from_confusion(confusion):
    """4 x 4 counts [truth class, predicted class] -> {'sens_wt', 'sens_tc', 'sens_et', 'spec_wt', 'spec_tc', 'spec_et'}: sensitivity
    TP / (TP + FN) and specificity TN / (TN + FP) of the BraTS regions, float64 on the host, nan where the denominator is zero"""
    m = np.asarray(confusion)
    if m.shape != (4, 4):
        raise ValueError('confusion must be 4 x 4 (the BraTS regions are sets of classes 1..3), got shape %s' % (m.shape,))
    m = m.astype(np.int64)
    total = int(m.sum())
    out = {}
    for name, sel in BRATS_REGIONS:
        sel = list(sel)
        tp, t, p = int(m[np.ix_(sel, sel)].sum()), int(m[sel, :].sum()), int(m[:, sel].sum())
        tn, neg = total - t - p + tp, total - t
        out['sens_' + name] = tp / t if t else float('nan')
        out['spec_' + name] = tn / neg if neg else float('nan')
    return out


UNCERTAINTY_SCORE_KEYS = ('qu_score', 'qu_dice_auc', 'qu_ftp_auc', 'qu_ftn_auc')


def uncertainty_channels(targets='labels', n_classes=4):
    """-> ((name, classes), ...) of an uncertainty map's channels over min(label, K-1): BRATS_REGIONS for 'regions', the single classes
    ('class_1', (1,)), ... for 'labels'"""
    if targets not in TARGETS:
        raise ValueError('unknown targets %r: one of %s' % (targets, TARGETS))
    return BRATS_REGIONS if targets == 'regions' else tuple(('class_%d' % c, (c,)) for c in range(1, int(n_classes)))


def uncertainty_scores_from_counts(table):
    """(101, 4) counts [level, (TN, FP, FN, TP)] of one channel -> (score, dice_auc, ftp_auc, ftn_auc), float64 on the host.  See
    `uncertainty_scores` for the definition"""
    t = np.asarray(table)
    if t.shape != (101, 4):
        raise ValueError('table must be (101, 4): one row per level, cells TN, FP, FN, TP; got shape %s' % (t.shape,))
    kept = np.cumsum(t.astype(np.int64), axis=0).astype(np.float64)          # at threshold tau: the voxels with level <= tau
    tn, fp, fn, tp = kept[:, 0], kept[:, 1], kept[:, 2], kept[:, 3]
    den = 2.0 * tp + fp + fn
    dice = np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 1.0)
    ftp = (tp[100] - tp) / tp[100] if tp[100] > 0 else np.zeros(101)
    ftn = (tn[100] - tn) / tn[100] if tn[100] > 0 else np.zeros(101)

    def auc(v):                                                              # the trapezoid over tau = 0..100, divided by 100
        return float((v[0] / 2.0 + v[1:100].sum() + v[100] / 2.0) / 100.0)
    a_dice, a_ftp, a_ftn = auc(dice), auc(ftp), auc(ftn)
    return (a_dice + (1.0 - a_ftp) + (1.0 - a_ftn)) / 3.0, a_dice, a_ftp, a_ftn


def uncertainty_scores(truth, pred, unc, mask=None, targets='labels', n_classes=4):
    """the uncertainty-filtered scores of the BraTS uncertainty task (QU-BraTS, Mehta et al. 2022) of a map `unc`, uint8 (D,H,W,C) levels
    0..100 channels last, for the label maps truth and pred, uint8 (D,H,W) (device tensors or numpy); mask: uint8 (D,H,W) or None, only
    voxels with mask != 0 count.  Channels: wt, tc, et with the class sets BRATS_REGIONS for targets 'regions', class_1.. with single
    classes for 'labels' (`uncertainty_channels`); labels >= K-1 count as class K-1.
    -> {'qu_score_<name>', 'qu_dice_auc_<name>', 'qu_ftp_auc_<name>', 'qu_ftn_auc_<name>'} per channel.  Per channel, with thresholds
    tau = 0, 1, ..., 100 and the voxels of level <= tau KEPT at tau:
      Dice(tau) = 2 TP / (2 TP + FP + FN) over the kept voxels, 1 where the denominator is 0;
      FTP(tau) = (TP_100 - TP_tau) / TP_100, the true positives filtered out, and FTN(tau) likewise of the true negatives, each 0 where
      its denominator is 0;
      AUC = the trapezoid over tau, divided by 100;
      score = (AUC_Dice + (1 - AUC_FTP) + (1 - AUC_FTN)) / 3.
    Where published code differs in a detail, this definition holds.  The device counts the table (ops.uncertainty_confusion: one pass,
    integer counts), the host reduces it in float64 (`uncertainty_scores_from_counts`)."""
    chans = uncertainty_channels(targets, n_classes)
    tmap, pmap = _label_maps(truth, pred, 'uncertainty_scores')
    if tuple(unc.shape) != tuple(tmap.shape) + (len(chans),):
        raise ValueError('uncertainty_scores: the map must have shape %s, got %s' % (tuple(tmap.shape) + (len(chans),), tuple(unc.shape)))
    maps = []
    for t in (unc, mask):
        if isinstance(t, np.ndarray):
            if t.dtype != np.uint8:
                raise ValueError('uncertainty_scores: the map and the mask must be uint8, got %s' % t.dtype)
            t = torch.from_numpy(np.ascontiguousarray(t)).to(tmap.device)
        maps.append(None if t is None else t.contiguous())
    if maps[1] is not None and tuple(maps[1].shape) != tuple(tmap.shape):
        raise ValueError('uncertainty_scores: the mask must have shape %s, got %s' % (tuple(tmap.shape), tuple(maps[1].shape)))
    table = ops.uncertainty_confusion(tmap, pmap, maps[0], [sum(1 << int(c) for c in set(sel)) for _, sel in chans], mask=maps[1],
                                      n_classes=int(n_classes)).cpu().numpy()                 # the one read
    out = {}
    for (name, _), counts in zip(chans, table):
        for key, v in zip(UNCERTAINTY_SCORE_KEYS, uncertainty_scores_from_counts(counts)):
            out['%s_%s' % (key, name)] = v
    return out


def _percentile_ranks(q, m):
    """the 0-based order statistics np.percentile(values, 100 q) of m values interpolates between, and the last one"""
    pos = q * (m - 1)
    return [int(np.floor(pos)), int(np.ceil(pos)), m - 1]


def _percentile_value(q, lo, hi, m):
    """np.percentile's linear interpolation between the two order statistics of `_percentile_ranks`, float64 on the host"""
    pos = q * (m - 1)
    return float(lo + (hi - lo) * (pos - np.floor(pos)))


def _label_maps(truth, pred, who):
    """surface_scores' checks and upload of its two maps, for lesionwise_scores -> (truth, pred) dense uint8 (D,H,W) on the GPU"""
    if tuple(truth.shape) != tuple(pred.shape):
        raise ValueError('%s: truth has shape %s, the prediction %s' % (who, tuple(truth.shape), tuple(pred.shape)))
    if len(truth.shape) != 3:
        raise ValueError('%s: label maps must have shape (D,H,W), got %s' % (who, tuple(truth.shape)))
    maps = []
    for t in (truth, pred):
        if isinstance(t, np.ndarray):
            if t.dtype != np.uint8:
                raise ValueError('%s: label maps must be uint8, got %s' % (who, t.dtype))
            if not torch.cuda.is_available():
                raise RuntimeError('%s: the distances are computed on the GPU (no CPU fallback exists for the product path)' % who)
            t = torch.from_numpy(np.ascontiguousarray(t)).cuda()
        maps.append(t.contiguous())
    return maps


def surface_scores(truth, pred, spacing, n_classes=4, percentile=95.0):
    """Hausdorff distances in mm between the surfaces of two uint8 label maps (D,H,W) of equal shape (device tensors or numpy) on a
    grid of voxel spacing `spacing` = (sd,sh,sw) -> {'hd95', 'hd', 'hd95_directed', 'surface_voxels': one entry per class 1..K-1, and for
    n_classes == 4 'hd95_wt/tc/et', 'hd_wt/tc/et'}.  Labels >= K-1 count as class K-1.  Per region, with T / P the surface voxels (a
    face neighbour outside the region or the volume) of truth / prediction: d(P->T) = the distances from every voxel of P to the
    nearest voxel of T, d(T->P) likewise; hd95 = np.percentile of the two sets pooled (medpy's hd95), hd = their maximum,
    hd95_directed = (percentile of d(P->T), of d(T->P)) (its maximum is MONAI's convention), surface_voxels = (|T|, |P|).  nan when
    both regions are empty, inf when one is.  On the device: bts_region_surface, bts_edt3d_sq (exact, float64, mm^2),
    bts_masked_select (exact order statistics); on the host the ranks, the square roots and the interpolation, in float64."""
    if tuple(truth.shape) != tuple(pred.shape):
        raise ValueError('surface_scores: truth has shape %s, the prediction %s' % (tuple(truth.shape), tuple(pred.shape)))
    if len(truth.shape) != 3:
        raise ValueError('surface_scores: label maps must have shape (D,H,W), got %s' % (tuple(truth.shape),))
    q = float(percentile) / 100.0
    if not 0.0 <= q <= 1.0:
        raise ValueError('surface_scores: percentile must lie in [0, 100], got %r' % (percentile,))
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3:
        raise ValueError('surface_scores: spacing must be (sd,sh,sw), got %r' % (spacing,))
    k = int(n_classes)
    maps = []
    for t in (truth, pred):
        if isinstance(t, np.ndarray):
            if t.dtype != np.uint8:
                raise ValueError('surface_scores: label maps must be uint8, got %s' % t.dtype)
            if not torch.cuda.is_available():
                raise RuntimeError('surface_scores: the distances are computed on the GPU (no CPU fallback exists for the product path)')
            t = torch.from_numpy(np.ascontiguousarray(t)).cuda()
        maps.append(t.contiguous())
    tmap, pmap = maps
    dev, shape, n = tmap.device, tuple(tmap.shape), tmap.numel()
    names = ['class_%d' % c for c in range(1, k)]
    masks = [1 << c for c in range(1, k)]
    if k == 4:
        for name, sel in BRATS_REGIONS:
            names.append(name)
            masks.append(sum(1 << c for c in sel))
    uniq = sorted(set(masks))
    # one set of buffers for every region: mask = [surface of P | surface of T], values = [dist2 to T's surface | dist2 to P's surface]
    surf = torch.empty(2 * n, dtype=torch.uint8, device=dev)
    dist = torch.empty(2 * n, dtype=torch.float64, device=dev)
    sp, st = surf[:n].view(shape), surf[n:].view(shape)
    counts = torch.zeros((len(uniq), 2), dtype=torch.int64, device=dev)
    for i, cm in enumerate(uniq):
        ops.region_surface(tmap, k, cm, out=st, count=counts[i, 0:1])
        ops.region_surface(pmap, k, cm, out=sp, count=counts[i, 1:2])
    counts = counts.cpu().numpy()                                  # the one read of the surface counts

    def ranks(m):
        return _percentile_ranks(q, m)

    picked = torch.zeros((len(uniq), 3, 3), dtype=torch.float64, device=dev)
    live = []
    for i, cm in enumerate(uniq):
        nt, npr = int(counts[i, 0]), int(counts[i, 1])
        if nt == 0 or npr == 0:
            continue
        live.append(i)
        ops.region_surface(tmap, k, cm, out=st, count=torch.zeros(1, dtype=torch.int64, device=dev))
        ops.region_surface(pmap, k, cm, out=sp, count=torch.zeros(1, dtype=torch.int64, device=dev))
        ops.edt3d_sq(st, spacing, out=dist[:n])
        ops.edt3d_sq(sp, spacing, out=dist[n:])
        ops.masked_select(dist, surf, ranks(nt + npr), out=picked[i, 0])
        ops.masked_select(dist[:n], surf[:n], ranks(npr), out=picked[i, 1])
        ops.masked_select(dist[n:], surf[n:], ranks(nt), out=picked[i, 2])
    picked = np.sqrt(picked.cpu().numpy()) if live else None

    def interpolate(lo, hi, m):
        return _percentile_value(q, lo, hi, m)

    res = {}
    for i, cm in enumerate(uniq):
        nt, npr = int(counts[i, 0]), int(counts[i, 1])
        if nt == 0 or npr == 0:
            v = float('nan') if nt == npr else float('inf')
            res[cm] = (v, v, (v, v), (nt, npr))
            continue
        a = picked[i]
        res[cm] = (interpolate(a[0, 0], a[0, 1], nt + npr), float(a[0, 2]),
                   (interpolate(a[1, 0], a[1, 1], npr), interpolate(a[2, 0], a[2, 1], nt)), (nt, npr))
    per = [res[cm] for cm in masks[:k - 1]]
    out = {'hd95': [r[0] for r in per], 'hd': [r[1] for r in per], 'hd95_directed': [r[2] for r in per],
           'surface_voxels': [r[3] for r in per]}
    for name, cm in zip(names[k - 1:], masks[k - 1:]):
        out['hd95_' + name], out['hd_' + name] = res[cm][0], res[cm][1]
    return out


def _lesionwise_region(tmap, pmap, spacing, k, class_mask, q, dilation, dilation_connectivity, connectivity, min_lesion_voxels, penalty_mm):
    """steps 1-7 of `lesionwise_scores` for one region -> (lw_dice, lw_hd95, counts, lesions)"""
    dev, n = tmap.device, tmap.numel()
    counts = {'lesions': 0, 'false_negatives': 0, 'false_positives': 0, 'ignored': 0}
    td = ops.dilate3d(tmap, class_mask, k, dilation_connectivity, dilation)
    tdc = ops.components3d(td, 2, 2, connectivity)
    pc = ops.components3d(pmap, class_mask, k, connectivity)
    found = torch.zeros(2, dtype=torch.int64, device=dev)
    size_p = torch.empty(n, dtype=torch.int32, device=dev)
    ops.component_sizes(tdc, out=size_p, count=found[0:1])
    ops.component_sizes(pc, out=size_p, count=found[1:2])
    n_td, n_p = (int(v) for v in found.cpu().tolist())                               # read: the two component counts
    if n_td == 0 and n_p == 0:
        return 1.0, 0.0, counts, []
    lesions, live = [], []
    matched_all = []
    if n_td:
        rows, lvox = ops.lesion_pairs(tdc, tmap, pc, class_mask, k, counts=(n_td, n_p))     # read: the pairs
        td_roots = torch.nonzero(lvox).view(-1)                                      # ascending = lesion order (a sync of its own)
        matched_all = sorted(set(int(r) for r in rows[:, 1]))
        mr = torch.tensor(matched_all, dtype=torch.int64, device=dev)
        tb = ops.component_boxes(tdc, td_roots.to(torch.int32))
        pb = ops.component_boxes(pc, mr.to(torch.int32))
        host = torch.cat([td_roots, lvox[td_roots].long(), tb.view(-1).long(), pb.view(-1).long(), size_p[mr].long()]).cpu().numpy()
        nl, nm = td_roots.numel(), len(matched_all)                                  # read: roots, sizes and boxes
        if nl != n_td:
            raise RuntimeError('lesionwise_scores: %d dilated components, %d of them hold truth voxels' % (n_td, nl))
        roots, lv = host[:nl], host[nl:2 * nl]
        tbox = host[2 * nl:8 * nl].reshape(nl, 6)
        pbox = host[8 * nl:8 * nl + 6 * nm].reshape(nm, 6)
        psize = dict(zip(matched_all, host[8 * nl + 6 * nm:].tolist()))
        pidx = {r: i for i, r in enumerate(matched_all)}
        for i in range(nl):
            root, vox = int(roots[i]), int(lv[i])
            if vox < min_lesion_voxels:
                counts['ignored'] += 1
                continue
            mine = rows[rows[:, 0] == root]
            comps = [int(c) for c in mine[:, 1]]
            les = {'voxels': vox, 'matched_components': len(comps), 'matched_voxels': sum(psize[c] for c in comps),
                   'overlap': int(mine[:, 3].sum()), 'dice': 0.0, 'hd95': float(penalty_mm)}
            lesions.append(les)
            if not comps:
                counts['false_negatives'] += 1
                continue
            les['dice'] = 2.0 * les['overlap'] / (les['voxels'] + les['matched_voxels'])
            boxes = np.concatenate([tbox[i:i + 1], pbox[[pidx[c] for c in comps]]])
            box = tuple(int(v) for v in boxes[:, :3].min(axis=0)) + tuple(int(v) for v in boxes[:, 3:].max(axis=0))
            live.append((les, root, comps, box))
    counts['lesions'] = len(lesions)
    counts['false_positives'] = n_p - len(matched_all)
    if live:
        # per lesion, the buffers of surface_scores on the box alone: mask = [surface of M | surface of L], values = [dist2 to L's | to M's]
        nsurf = torch.zeros((len(live), 2), dtype=torch.int64, device=dev)
        surfs = []
        for j, (les, root, comps, box) in enumerate(live):
            g, m = ops.lesion_crop(tdc, tmap, pc, class_mask, box, root, comps, K=k)
            nb = g.numel()
            surf = torch.empty(2 * nb, dtype=torch.uint8, device=dev)
            ops.region_surface(g, 2, 2, out=surf[nb:], count=nsurf[j, 0:1])
            ops.region_surface(m, 2, 2, out=surf[:nb], count=nsurf[j, 1:2])
            surfs.append((surf, tuple(g.shape)))
        nsurf = nsurf.cpu().numpy()                                                  # read: the surface counts of every lesion
        picked = torch.zeros((len(live), 2), dtype=torch.float64, device=dev)
        for j, (surf, ext) in enumerate(surfs):
            nb = surf.numel() // 2
            dist = torch.empty(2 * nb, dtype=torch.float64, device=dev)
            ops.edt3d_sq(surf[nb:].view(ext), spacing, out=dist[:nb])
            ops.edt3d_sq(surf[:nb].view(ext), spacing, out=dist[nb:])
            ops.masked_select(dist, surf, _percentile_ranks(q, int(nsurf[j].sum()))[:2], out=picked[j])
        picked = np.sqrt(picked.cpu().numpy())                                       # read: the order statistics of every lesion
        for j, (les, _, _, _) in enumerate(live):
            les['hd95'] = _percentile_value(q, picked[j, 0], picked[j, 1], int(nsurf[j].sum()))
    total = len(lesions) + counts['false_positives']
    if total == 0:
        return float('nan'), float('nan'), counts, lesions
    sum_dice = sum_hd = 0.0
    for les in lesions:                                                              # float64, in lesion order
        sum_dice += les['dice']
        sum_hd += les['hd95']
    return sum_dice / total, (sum_hd + float(penalty_mm) * counts['false_positives']) / total, counts, lesions


def lesionwise_scores(truth, pred, spacing, n_classes=4, regions=None, dilation=3, dilation_connectivity=18, connectivity=26,
                      min_lesion_voxels=50, penalty_mm=374.0, percentile=95.0):
    """lesion-wise Dice and HD95 (the BraTS 2023 ranking) between two uint8 label maps (D,H,W) of equal shape (device tensors or numpy)
    on a grid of voxel spacing `spacing` = (sd,sh,sw) mm.  regions: ((name, classes), ...) over min(label, K-1), BRATS_REGIONS for
    n_classes == 4 and the single classes ('class_1', ...) otherwise.  Per region, with T / P its binary maps in truth / prediction:
      1. T and P both empty: Dice 1, HD95 0, all counts 0;
      2. T dilated `dilation` times (dilation_connectivity, clipped at the volume's border) and labelled (connectivity); a LESION is the
         set of T's voxels inside one component of the dilated map, lesions in the order of their components' first voxels;
      3. P labelled (connectivity) into predicted components;
      4. a component MATCHES a lesion when a voxel of it lies inside the lesion's dilated component (the halo alone is enough), may match
         several lesions, and is a FALSE POSITIVE when it matches none, lesions ignored in 5 included;
      5. a lesion of fewer than min_lesion_voxels voxels is IGNORED: no row, no count;
      6. per remaining lesion L with M the union of its matched components: M empty is a FALSE NEGATIVE (dice 0, hd95 penalty_mm),
         otherwise dice = 2 |L & M| / (|L| + |M|) and hd95 = surface_scores' HD95 of L against M;
      7. lw_dice = sum dice / n, lw_hd95 = (sum hd95 + penalty_mm * false positives) / n with n = scored lesions + false positives,
         float64 sums in lesion order; nan when n == 0.
    -> {'lw_dice_<name>', 'lw_hd95_<name>', 'lw_counts_<name>': {'lesions', 'false_negatives', 'false_positives', 'ignored'},
        'lw_lesions_<name>': [{'voxels', 'matched_components', 'matched_voxels', 'overlap', 'dice', 'hd95'} per scored lesion]}.
    On the device: bts_dilate3d, bts_components3d, bts_component_sizes, bts_lesion_pairs, bts_component_boxes, bts_lesion_crop, and per
    lesion on its bounding box bts_region_surface, bts_edt3d_sq, bts_masked_select; no label map travels to the host, which reads
    counts, the pair table, roots with sizes and boxes, surface counts and order statistics, once each per region."""
    tmap, pmap = _label_maps(truth, pred, 'lesionwise_scores')
    q = float(percentile) / 100.0
    if not 0.0 <= q <= 1.0:
        raise ValueError('lesionwise_scores: percentile must lie in [0, 100], got %r' % (percentile,))
    spacing = tuple(float(s) for s in spacing)
    if len(spacing) != 3:
        raise ValueError('lesionwise_scores: spacing must be (sd,sh,sw), got %r' % (spacing,))
    if dilation < 0 or min_lesion_voxels < 0 or not penalty_mm >= 0:
        raise ValueError('lesionwise_scores: dilation, min_lesion_voxels and penalty_mm must not be negative, got %r, %r and %r' %
                         (dilation, min_lesion_voxels, penalty_mm))
    k = int(n_classes)
    if regions is None:
        regions = BRATS_REGIONS if k == 4 else tuple(('class_%d' % c, (c,)) for c in range(1, k))
    out, done = {}, {}
    for name, sel in regions:
        cm = sum(1 << int(c) for c in set(sel))
        if cm not in done:
            done[cm] = _lesionwise_region(tmap, pmap, spacing, k, cm, q, int(dilation), int(dilation_connectivity), int(connectivity),
                                          int(min_lesion_voxels), float(penalty_mm))
        dice, hd, counts, lesions = done[cm]
        out['lw_dice_' + name], out['lw_hd95_' + name] = dice, hd
        out['lw_counts_' + name], out['lw_lesions_' + name] = dict(counts), [dict(les) for les in lesions]
    return out
