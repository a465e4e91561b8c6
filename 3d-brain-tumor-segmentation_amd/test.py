"""Segment folders of scans end to end: the reference's test.py main() (test.py:181-270) on the device.

    python -m bts_amd.test --in_locs a,b --modalities t1ce,flair --tumor_model DIR[,DIR...] --tumor_prepro DIR/prepro.npy[,FILE...]
                           [--uncertainty entropy|std]
                           [--skull_model DIR --skull_prepro FILE] [--truth seg] [--out_loc DIR] [--dtype float16]
                           [--min_component_voxels N] [--et_min_voxels N] [--component_connectivity 26] [--skull_largest_component]
                           [--lesionwise] [--lesion_dilation 3] [--lesion_min_voxels 50] [--lesion_penalty_mm 374]
                           [--window D,H,W|crop] [--window_overlap 0.5] [--window_mode gaussian] [--window_batch N]
                           [--conform [CODE]] [--coregister] [--coregister_max_mm 30] [--coregister_max_deg 20] [--coregister_bins 32]
                           [--bias_correct [--bias_shrink 4] [--bias_levels 4] [--bias_iters 50] [--bias_threshold 0.001] [--bias_fwhm 0.15]]

This module is named after the reference's script and is NOT a pytest module: pytest's `test_*.py` pattern does not match `test.py`
and `testpaths` points at tests/, so it is never collected.

Every sub-folder of every folder of --in_locs is a case.  Per case: the modalities (and, with --truth, the label) are decoded by host
threads while the device works on the previous case; `infer.segment_case` resamples to 1 mm^3, runs the optional skull-stripping
model and the tumour model with test-time augmentation and brings the labels back to the scan's grid; `mask.nii` is written with
the affine averaged over the modalities into the case folder (test.py:69-70), or into DIR/<case>/ with --out_loc; a labelled case
prints the reference's line (test.py:269) from `infer.label_scores`.  With --out_loc a `scores.csv` holds one row per labelled case
and a last row computed from the summed confusion matrix.  With --surface_metrics each labelled case also gets the 95th-percentile Hausdorff
distance (mm, on the scan's own grid with its pixdim) and the sensitivity and specificity of the regions WT, TC and ET
(`infer.surface_scores`, `infer.region_rates_from_confusion`): nine more columns after the existing ones; the `total` row holds the mean
of the finite distances and the rates of the summed confusion matrix.

Post-processing of the label map, off by default (`infer.postprocess_labels`, connected components on the device): with
--min_component_voxels N connected pieces of the whole tumour (labels 1, 2 and 4 together; 6, 18 or 26 neighbours by
--component_connectivity) of fewer than N voxels become background, and with --et_min_voxels N an enhancing tumour (label 4) of fewer
than N voxels in all becomes label 1; --skull_largest_component reduces the brain the skull-stripping model finds to its largest
connected piece before the tumour model sees the scan.  `mask.nii` and every score are of the post-processed map, and one more line per
case prints what was removed.  The columns of scores.csv do not change.

With --lesionwise each labelled case also gets the lesion-wise Dice and HD95 of WT, TC and ET (`infer.lesionwise_scores`, the BraTS 2023
ranking: every truth lesion scored on its own, a missed lesion 0 and --lesion_penalty_mm, a predicted component on no lesion a false
positive; --lesion_dilation iterations join truth pieces into one lesion, lesions below --lesion_min_voxels are ignored), taken on the
mask as written: fifteen more columns at the end of the row (after those of --surface_metrics), lw_dice_*, lw_hd95_*, and the counts
lw_lesions_*, lw_fn_*, lw_fp_*; the `total` row holds the mean of the finite scores and the sums of the counts; one more line per case.

With --window D,H,W both models predict windows of that extent in place of the whole padded volume and blend them where they overlap
(`infer.WindowSpec`, `infer.window_plan`: --window_overlap is the fraction two neighbouring windows share, --window_mode the importance
map, `gaussian` or `constant`, --window_batch the windows and augmented copies per forward); --window crop takes each model's recorded
crop size.  A window must be a multiple of each model's spatial resolution.  Windows without a brain-mask voxel are not run, and one
more line per case prints the windows run and skipped per stage.  Without --window nothing changes.

With --conform [CODE] (default LPS, the orientation of the BraTS arrays) the headers decide where the voxels are: every modality keeps its
own shape and its best affine (`nifti.best_affine`: the sform, else the qform; a header with neither is refused), and an
`infer.Conformer` brings them all onto one 1 mm grid of that orientation -- the first modality's axes, permuted, reversed and rescaled;
an exact copy where that is a pure reorientation, a spline resample of --order otherwise -- and the prediction back onto the first
modality's grid.  A RAS scan, a sagittal acquisition, or modalities exported on different grids then segment as the same scan in BraTS
layout does.  The truth volume must lie on the first modality's grid (same shape, affine within 1e-3 voxel at the corners), else the case
is reported and skipped.  Scores act on that native grid, with its own voxel size for the distances; `mask.nii` carries the first
modality's affine, not a mean; one more line per case prints the native orientation code, the voxel size and the path taken.  Without
--conform nothing changes.

With --conform --coregister every modality after the first is first registered to the first one: `coreg.coregister_case` estimates one
rigid motion per modality by normalised mutual information on the device (at most --coregister_max_mm and --coregister_max_deg per
parameter, --coregister_bins intensity bins) and corrects that modality's affine, so the Conformer reads it where the anatomy is, not where
the header says; one more line per case and modality prints the six parameters, the score before and after and the candidates evaluated.
`mask.nii`, the truth check and every score are as with --conform alone: they belong to the first modality, which is not moved.  Without
--conform the modalities are stacked voxel for voxel and there is no affine to correct: --coregister is then refused.

Recorded geometry: where the tumour stage's prepro.npy records a `geometry` (`python -m bts_amd.preprocess --conform` wrote it: the examples
the model was trained on were conformed by their headers), every scan is conformed to the recorded orientation code without any flag
here, and co-registered first with the recorded bounds where it records them (`geometry_rule`, `preprocess.load_geometry`); one line at
the start says so.  --conform CODE and --coregister with its bounds win over the record, a code other than the recorded one gets one
warning line, and the dumps of an ensemble must record the same geometry (a refusal names the member).  The truth rule of --conform is
the same either way.  A prepro.npy without the entry changes nothing.

Bias-field correction: where the tumour stage's prepro.npy records a `bias` spec (`python -m bts_amd.preprocess --bias_correct` wrote it),
or with --bias_correct, every modality of every case is corrected once by N4 on its own positive voxels right after upload
(`n4.correct`, csrc/n4.hip), before --coregister, --conform, the Interpolator and both model stages.  --bias_shrink, --bias_levels,
--bias_iters, --bias_threshold and --bias_fwhm need --bias_correct and replace the recorded fields.  One line at the start says which
rule applies, one more line per case prints the sweeps per level and the final cv per modality.  Without either nothing changes.

Ensembles and uncertainty: --tumor_model A,B,C runs every checkpoint folder of the list as a member of one `infer.StageEnsemble` (its own
statistics, normalisation and crop size each; --tumor_prepro takes one dump for all of them or one per member) and decodes the mean of
their probabilities; the members must agree in resolution, output channels, `targets` and the flags here make them agree in the rest,
and a refusal names the member.  With --uncertainty entropy|std each case also gets `unc_<name>.nii` beside `mask.nii`, uint8 levels
0..100 with the same affine, one file per channel of the tumour stage (wt, tc, et for a stage trained on regions, else 1, 2, 4): the
binary entropy of the mean probability, or (two models at least) the deviation between the members.  A labelled case prints one more line
and gets twelve more columns at the end of its scores.csv row, the scores of `infer.uncertainty_scores` (qu_score_*, qu_dice_auc_*,
qu_ftp_auc_*, qu_ftn_auc_*: uncertainty-filtered Dice and the filtered true positives and negatives of the BraTS uncertainty task),
counted inside the brain mask on the scan's grid; the `total` row holds the mean of the finite values.  Post-processing changes the
labels, never the map.  One line at the start lists the members and what each decodes.  One model and no --uncertainty is the code path
there has always been.

The flags and defaults are the reference's TestArgParser (args.py:199-235), its two checks included (args.py:243-246).  --gpu is
accepted and implied: there is no CPU path.  Added: --uncertainty, the comma lists of --tumor_model and --tumor_prepro, --dtype, --tta_batch, --workers, --out_loc, --surface_metrics,
--min_component_voxels, --et_min_voxels, --component_connectivity, --skull_largest_component, --lesionwise, --lesion_dilation,
--lesion_min_voxels, --lesion_penalty_mm, --window, --window_overlap, --window_mode, --window_batch, --conform, --coregister,
--coregister_max_mm, --coregister_max_deg, --coregister_bins, --bias_correct, --bias_shrink, --bias_levels, --bias_iters,
--bias_threshold, --bias_fwhm.

Deviations:
  * cases are visited in sorted order of their paths (the reference: the file system's order);
  * each model is built at the crop size recorded in its train_args.pkl, as test.py:186-188 does, so that the checkpoint's
    VAE variables (tied to that extent, vae.py:101-111) load; a train_args.pkl without one builds at the first case's padded shape;
  * a case with a missing modality is reported by name and skipped (the reference's glob(...)[0] ends the run with an IndexError);
  * the score is `infer.label_scores` (see bts_amd.infer on why the reference's call is not functional);
  * a model trained with `python -m bts_amd.train --targets regions` (its train_args.pkl says so; there is no flag here) is decoded
    as the nested regions WT, TC, ET (`infer.StageSpec(targets='regions')`, bts_region_finish) to the same {0,1,2,4} label map that
    post-processing, `mask.nii` and every score take; any other model by the arg-max, as before.
  * a stage whose prepro.npy was written by `python -m bts_amd.preprocess --norm case` (the file says so; there is no flag here)
    normalises every scan on its own brain voxels, with the recorded percentile clipping (`preprocess.load_norm`,
    `infer.StageSpec(norm=...)`, bts_case_norm); any other file means the dataset's mean and deviation, as before.
"""
import argparse
import glob
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import coreg, n4, nifti
from .infer import (BRATS_REGIONS, UNCERTAINTY_MODES, UNCERTAINTY_SCORE_KEYS, WINDOW_MODES, Conformer, Interpolator, StageEnsemble, StageSpec, WindowSpec,
                    label_scores, lesionwise_scores, region_rates_from_confusion, scores_from_confusion, segment_case, surface_scores,
                    uncertainty_channels, uncertainty_scores, zoom_output_shape)
from .preprocess import (COREGISTER_DEFAULTS, add_bias_flags, add_geometry_flags, bias_spec, check_geometry_flags,      # noqa: F401
                         code_arg as _code_arg, coregister_kwargs, load_bias, load_geometry, load_norm, truth_grid_shift)
from .train import load_checkpoint, load_train_args

N_CLASSES = 4        # background + the three BraTS labels 1, 2, 4 (4 counts as class 3, preprocess.py:36)
HD95_KEYS = ('hd95_wt', 'hd95_tc', 'hd95_et')
RATE_KEYS = ('sens_wt', 'sens_tc', 'sens_et', 'spec_wt', 'spec_tc', 'spec_et')
SURFACE_KEYS = HD95_KEYS + RATE_KEYS      # the columns --surface_metrics appends to scores.csv
LESION_SCORE_KEYS = tuple('lw_%s_%s' % (what, name) for what in ('dice', 'hd95') for name, _ in BRATS_REGIONS)
LESION_COUNT_KEYS = tuple('lw_%s_%s' % (what, name) for what in ('lesions', 'fn', 'fp') for name, _ in BRATS_REGIONS)
LESION_KEYS = LESION_SCORE_KEYS + LESION_COUNT_KEYS      # the columns --lesionwise appends to scores.csv, after the others
LESION_DEFAULTS = {'lesion_dilation': 3, 'lesion_min_voxels': 50, 'lesion_penalty_mm': 374.0}
WINDOW_DEFAULTS = {'window_overlap': 0.5, 'window_mode': 'gaussian', 'window_batch': None}


UNCERTAINTY_FILE_NAMES = {'regions': ('wt', 'tc', 'et'), 'labels': ('1', '2', '4')}      # unc_<name>.nii per channel of the map


def tumor_models(args):
    """--tumor_model A,B,C -> the checkpoint folders of the ensemble's members, one for a single model"""
    return [m for m in args.tumor_model.split(',') if m]


def tumor_prepros(args):
    """--tumor_prepro: one dump for every member, or one per member -> one per member"""
    files, n = [f for f in args.tumor_prepro.split(',') if f], len(tumor_models(args))
    return files * n if len(files) == 1 else files


def uncertainty_keys(targets):
    """the columns --uncertainty appends to scores.csv for a tumour stage that decodes `targets`"""
    return tuple('%s_%s' % (key, name) for key in UNCERTAINTY_SCORE_KEYS for name, _ in uncertainty_channels(targets, N_CLASSES))


def _window_arg(text):
    """--window: 'crop' or three positive integers D,H,W"""
    if text == 'crop':
        return text
    try:
        roi = tuple(int(v) for v in text.split(','))
    except ValueError:
        roi = ()
    if len(roi) != 3 or min(roi) < 1:
        raise argparse.ArgumentTypeError("expected D,H,W (three positive integers) or 'crop', got %r" % (text,))
    return roi


def arg_parser():
    """the flags of the reference's TestArgParser (args.py:199-235) and ours"""
    p = argparse.ArgumentParser(prog='python -m bts_amd.test', description=__doc__.split('\n')[0])
    p.add_argument('--in_locs', type=str, required=True, help='Comma-separated paths of test data.')
    p.add_argument('--modalities', type=str, required=True, help='Comma-separated modalities to be used as input')
    p.add_argument('--truth', type=str, default='', help='Truth label pattern to use (optional).')
    p.add_argument('--tumor_prepro', type=str, required=True, help='Path to Numpy preprocessing dump for tumor segmentation.')
    p.add_argument('--skull_prepro', type=str, default='', help='Path to Numpy preprocessing dump for skull segmentation.')
    p.add_argument('--tumor_model', type=str, required=True, help='Path to checkpoint folder for tumor segmentation.')
    p.add_argument('--skull_model', type=str, default='', help='Path to checkpoint folder for skull-stripping segmentation.')
    p.add_argument('--order', type=int, default=3, help='Order of interpolation function to be used in voxel resizing.')
    p.add_argument('--mode', type=str, default='reflect', help='Method of handling image edges in interpolation.')
    p.add_argument('--spatial_tta', action='store_true', default=True, help='Whether to apply spatial augmentation on all spatial axes.')
    p.add_argument('--channel_tta', type=int, default=0, help='Additional intensity shifting samples to take.')
    p.add_argument('--threshold', type=float, default=0.5, help='Threshold at which to create mask from probabilities.')
    p.add_argument('--gpu', action='store_true', default=False, help='Accepted for the reference\'s command line; the GPU is always used.')
    p.add_argument('--dtype', type=str, default='float32', choices=('float32', 'float16', 'bfloat16'),
                   help='Storage type of activations and weight images in both stages.')
    p.add_argument('--tta_batch', type=int, default=None, help='Augmented copies per forward (default: 1 in float32, 4 in 16 bits).')
    p.add_argument('--workers', type=int, default=8, help='Host threads that decode the next cases; 0 decodes in line.')
    p.add_argument('--out_loc', type=str, default='', help='Write DIR/<case>/mask.nii and DIR/scores.csv instead of into the case folders.')
    p.add_argument('--surface_metrics', action='store_true', default=False,
                   help='Also score each labelled case with the 95th-percentile Hausdorff distance, sensitivity and specificity of WT, TC, ET.')
    p.add_argument('--min_component_voxels', type=int, default=0,
                   help='Remove connected components of the whole tumour of fewer voxels than this (0: keep all).')
    p.add_argument('--et_min_voxels', type=int, default=0,
                   help='Relabel an enhancing tumour of fewer voxels than this in all as label 1 (0: never).')
    p.add_argument('--component_connectivity', type=int, default=26, choices=(6, 18, 26),
                   help='Neighbours that connect two voxels of a component: by face, edge or corner.')
    p.add_argument('--skull_largest_component', action='store_true', default=False,
                   help='Keep only the largest connected piece of the brain found by the skull-stripping model.')
    # the lesion-wise flags exist in the namespace only where the command line gives them (tests/test_components_host.py pins the
    # attributes a plain command line parses to); `lesion_kwargs` supplies LESION_DEFAULTS
    p.add_argument('--lesionwise', action='store_true', default=argparse.SUPPRESS,
                   help='Also score each labelled case with the lesion-wise Dice and HD95 of WT, TC, ET (the BraTS 2023 ranking).')
    p.add_argument('--lesion_dilation', type=int, default=argparse.SUPPRESS,
                   help='Dilation iterations that join truth pieces into one lesion (default: %d).' % LESION_DEFAULTS['lesion_dilation'])
    p.add_argument('--lesion_min_voxels', type=int, default=argparse.SUPPRESS,
                   help='Truth lesions of fewer voxels than this are ignored (default: %d).' % LESION_DEFAULTS['lesion_min_voxels'])
    p.add_argument('--lesion_penalty_mm', type=float, default=argparse.SUPPRESS,
                   help='HD95 charged for a missed lesion or a false positive (default: %g).' % LESION_DEFAULTS['lesion_penalty_mm'])
    # likewise the sliding-window flags: `window_kwargs` supplies WINDOW_DEFAULTS
    p.add_argument('--window', type=_window_arg, default=argparse.SUPPRESS,
                   help="Predict blended windows of this extent D,H,W instead of the whole volume; 'crop': each model's recorded crop size.")
    p.add_argument('--window_overlap', type=float, default=argparse.SUPPRESS,
                   help='Fraction of a window shared with its neighbour, in [0, 1) (default: %g).' % WINDOW_DEFAULTS['window_overlap'])
    p.add_argument('--window_mode', type=str, choices=WINDOW_MODES, default=argparse.SUPPRESS,
                   help='Importance of a voxel inside its window (default: %s).' % WINDOW_DEFAULTS['window_mode'])
    p.add_argument('--window_batch', type=int, default=argparse.SUPPRESS,
                   help='Windows and augmented copies per forward (default: as --tta_batch).')
    # and --conform, and --coregister with its bounds, the ones of `python -m bts_amd.preprocess`: absent, the namespace has no such
    # attribute and nothing changes; `coregister_kwargs` supplies COREGISTER_DEFAULTS
    add_geometry_flags(p)
    # and --uncertainty: absent, no map is computed and no file written
    p.add_argument('--uncertainty', type=str, choices=UNCERTAINTY_MODES, default=argparse.SUPPRESS,
                   help='Also write unc_<name>.nii, levels 0..100 per voxel: the entropy of the mean probability, or the deviation '
                        'between the models of --tumor_model A,B,C.')
    # and --bias_correct with its sub-flags, the ones of `python -m bts_amd.preprocess`
    add_bias_flags(p)
    return p


def parse_args(argv=None):
    parser = arg_parser()
    args = parser.parse_args(argv)
    if args.min_component_voxels < 0 or args.et_min_voxels < 0:
        parser.error('--min_component_voxels and --et_min_voxels must not be negative')
    if not all(getattr(args, k, v) >= 0 for k, v in LESION_DEFAULTS.items()):
        parser.error('--lesion_dilation, --lesion_min_voxels and --lesion_penalty_mm must not be negative')
    if not hasattr(args, 'window') and any(hasattr(args, k) for k in WINDOW_DEFAULTS):
        parser.error('--window_overlap, --window_mode and --window_batch need --window')
    if not 0 <= getattr(args, 'window_overlap', 0.5) < 1:
        parser.error('--window_overlap must lie in [0, 1)')
    if getattr(args, 'window_batch', 1) < 1:
        parser.error('--window_batch must be positive')
    check_geometry_flags(args, parser)
    bias_spec(args, parser)
    models, prepros = tumor_models(args), [f for f in args.tumor_prepro.split(',') if f]
    if not models:
        parser.error('--tumor_model names no checkpoint folder')
    if len(prepros) not in (1, len(models)):
        parser.error('--tumor_prepro takes one file for all models or one per model: %d files for %d models' % (len(prepros), len(models)))
    if getattr(args, 'uncertainty', None) == 'std' and len(models) < 2:
        parser.error('--uncertainty std is the deviation between models and needs two at least in --tumor_model A,B')
    if args.skull_largest_component and not args.skull_model:
        parser.error('--skull_largest_component needs --skull_model')
    args.modalities = args.modalities.split(',')
    args.in_locs = args.in_locs.split(',')
    if not 0 < args.threshold < 1:                                                   # args.py:243-244
        raise AssertionError('Threshold must be a probability between (0, 1).')
    if args.skull_model and not args.skull_prepro:                                   # args.py:245-246
        raise AssertionError('Need skull preprocessing stats if model is provided.')
    args.skull_strip = bool(args.skull_model)
    return args


def find_cases(in_locs, out_loc=''):
    """every sub-folder of every folder, folders and entries in sorted order -> [(name, path)]; plain files (a scores.csv of an earlier
    run) and the output folder itself are no cases"""
    out = os.path.realpath(out_loc) if out_loc else None
    return [(os.path.basename(p.rstrip(os.sep)), p) for loc in in_locs for p in sorted(glob.glob(os.path.join(loc, '*')))
            if os.path.isdir(p) and os.path.realpath(p) != out]


def _first(path, name):
    found = sorted(glob.glob(os.path.join(path, '*' + name + '*' + '.nii' + '*')))
    return found[0] if found else None


def decode_case(path, modalities, truth, conform=False):
    """host side of one case (test.py:21-42,226-232) -> {'vols': float32 volumes with the axes reversed (the file's own byte order, see
    preprocess._decode_case), 'pixdim', 'affine': means over the modalities, 'truth': uint8 volume (axes reversed) or None}, or
    {'missing': name} when a modality has no file.  conform: also 'affines', every modality's best affine (float64), the modalities may
    differ in shape, and {'refused': why} for a header without an orientation or a truth volume off the first modality's grid"""
    vols, pixdim, affine, best = [], [], [], []
    for name in modalities:
        card = _first(path, name)
        if card is None:
            return {'missing': name}
        data, header = nifti.load(card)
        vols.append(np.ascontiguousarray(np.asarray(data).astype(np.float32).T))
        pixdim.append(header['pixdim'][:4])
        affine.append(header['affine'])
        if conform:
            try:
                best.append(nifti.best_affine(header))
            except ValueError as e:
                return {'refused': '%s: %s' % (os.path.basename(card), e)}
    y = None
    card = _first(path, truth) if truth else None
    if card is not None:
        data, header = nifti.load(card)
        y = np.ascontiguousarray(np.asarray(data).astype(np.uint8).T)
        if conform:
            try:
                off = truth_grid_shift(vols[0].shape[::-1], best[0], np.asarray(data).shape, nifti.best_affine(header))
            except ValueError as e:
                return {'refused': '%s: %s' % (os.path.basename(card), e)}
            if off is None or off > 1e-3:
                return {'refused': '%s does not lie on the grid of %s (%s)' % (os.path.basename(card), modalities[0], (
                    'another shape' if off is None else 'up to %.3g voxel off at the corners' % off))}
    out = {'vols': vols, 'pixdim': np.mean(pixdim, axis=0, dtype=np.float32), 'affine': np.mean(affine, axis=0, dtype=np.float32),
           'truth': y}
    if conform:
        out['affines'] = best
    return out


def upload_conform_case(case, dev):
    """-> ([one (D,H,W) float32 view per modality, each on its own grid], truth (D,H,W) uint8 or None) on `dev`"""
    vols = [torch.from_numpy(v).to(dev).permute(2, 1, 0) for v in case['vols']]
    y = case['truth']
    if y is not None:
        y = torch.from_numpy(y).to(dev).permute(2, 1, 0).contiguous()
    return vols, y


def upload_case(case, dev):
    """-> (x (D,H,W,C) float32, truth (D,H,W) uint8 or None) on `dev`; the transposition to the scan's axis order runs there"""
    vols = case['vols']
    x = torch.empty(vols[0].shape[::-1] + (len(vols),), dtype=torch.float32, device=dev)
    for ch, v in enumerate(vols):
        if v.shape != vols[0].shape:
            raise ValueError('the modalities differ in shape: %s' % ([u.shape[::-1] for u in vols],))
        x[..., ch].copy_(torch.from_numpy(v).to(dev).permute(2, 1, 0))
    y = case['truth']
    if y is not None:
        y = torch.from_numpy(y).to(dev).permute(2, 1, 0).contiguous()
    return x, y


def load_stage(folder, prepro, args, shape_1mm):
    """checkpoint folder + prepro.npy -> StageSpec: the model rebuilt from train_args.pkl's model_args (args.py:250-260), built, filled
    with load_checkpoint; spatial_res = 2 ** depth; mean / std from the prepro dump; `targets` (how the label map is decoded: the
    arg-max of a network trained on labels, or the regions WT, TC, ET of one trained with --targets regions) from train_args.pkl too,
    'labels' where it records none; `norm` (how a scan is normalised: with the dump's mean / std, or on its own brain voxels when the dump
    was written by `python -m bts_amd.preprocess --norm case`) from the prepro dump, one line printed per stage.  shape_1mm: the first case's extent on the
    1 mm^3 grid, the build shape (padded to the resolution) where train_args.pkl records no crop size"""
    from .model import Model
    targs = load_train_args(folder)
    kw = dict(targs['model_args'])
    kw.setdefault('in_ch', len(args.modalities))
    model = Model(**kw)
    res = 2 ** int(model.encoder.depth)
    crop = targs.get('crop_size')
    build = tuple(int(s) for s in crop) if crop else tuple(s + res - (s % res) for s in shape_1mm)
    model.build((1,) + build + (kw['in_ch'],))
    load_checkpoint(folder, model)
    norm = load_norm(prepro)
    mean, std = norm.mean, norm.std
    print('{}: normalisation {}{}'.format(folder, norm.mode, '' if norm.clip is None else ', clipped to the percentiles %g, %g' % norm.clip),
          flush=True)
    if mean.size != kw['in_ch']:
        raise ValueError('%s holds statistics of %d channels, the model of %s takes %d' % (prepro, mean.size, folder, kw['in_ch']))
    window = window_kwargs(args)
    if window is not None:
        if window['roi'] == 'crop':
            if not crop:
                raise ValueError('--window crop: the train_args.pkl of %s records no crop_size; give --window D,H,W' % folder)
            window['roi'] = tuple(int(s) for s in crop)
        window = WindowSpec(**window)
    return StageSpec(model, mean, std, res, spatial_tta=args.spatial_tta, channel_tta=args.channel_tta, threshold=args.threshold,
                     compute_dtype=args.dtype, tta_batch=args.tta_batch, window=window, targets=targs.get('targets', 'labels'), norm=norm)


def postprocess_kwargs(args):
    """-> the keyword arguments of infer.postprocess_labels the flags ask for, None when they ask for nothing"""
    if not (getattr(args, 'min_component_voxels', 0) or getattr(args, 'et_min_voxels', 0)):
        return None
    return {'min_component_voxels': args.min_component_voxels, 'et_min_voxels': args.et_min_voxels,
            'connectivity': getattr(args, 'component_connectivity', 26)}


def lesion_kwargs(args):
    """-> the keyword arguments of infer.lesionwise_scores the flags ask for, None without --lesionwise"""
    if not getattr(args, 'lesionwise', False):
        return None
    return {'dilation': getattr(args, 'lesion_dilation', LESION_DEFAULTS['lesion_dilation']),
            'min_lesion_voxels': getattr(args, 'lesion_min_voxels', LESION_DEFAULTS['lesion_min_voxels']),
            'penalty_mm': getattr(args, 'lesion_penalty_mm', LESION_DEFAULTS['lesion_penalty_mm'])}


def window_kwargs(args):
    """-> the keyword arguments of infer.WindowSpec the flags ask for ('roi' may still be 'crop': load_stage resolves it per model), None
    without --window"""
    if getattr(args, 'window', None) is None:
        return None
    return {'roi': args.window, 'overlap': getattr(args, 'window_overlap', WINDOW_DEFAULTS['window_overlap']),
            'mode': getattr(args, 'window_mode', WINDOW_DEFAULTS['window_mode']),
            'batch': getattr(args, 'window_batch', WINDOW_DEFAULTS['window_batch'])}


def bias_rule(args):
    """-> the n4.N4Spec every modality of every case is corrected with right after upload, or None: the spec the tumour stage's
    prepro.npy records (its examples were corrected, so its scans must be), or --bias_correct with its sub-flags, which replace the
    recorded fields.  Says which rule applies in one line; silent where none does"""
    prepro = tumor_prepros(args)[0]                           # of an ensemble: the first member's
    recorded = load_bias(prepro) if os.path.isfile(prepro) else None      # a missing dump is load_stage's to report
    spec = bias_spec(args, None, recorded)
    if spec is not None:
        why = ('--bias_correct' + (' over the record of %s' % prepro if recorded is not None else '')
               if hasattr(args, 'bias_correct') else 'recorded by %s' % prepro)
        print('Bias-field correction ({}): {}'.format(why, ', '.join('%s %s' % kv for kv in n4.spec_record(spec).items())), flush=True)
    return spec


def geometry_rule(args):
    """-> (orientation code or None, keyword arguments of coreg.coregister_case or None): how every case is conformed.  Where the tumour
    stage's prepro.npy records a geometry (`python -m bts_amd.preprocess --conform` wrote it: its examples were conformed, so its scans must
    be), that code and, where it records one, that co-registration apply without any flag, and one line says so.  --conform CODE and
    --coregister with its bounds win over the record; a code that differs from the recorded one gets one warning line.  The dumps of an
    ensemble must record the same geometry: ValueError naming the member.  No record and no flag: (None, None), and nothing changes"""
    prepros, models = tumor_prepros(args), tumor_models(args)
    records = [load_geometry(f) if os.path.isfile(f) else None for f in prepros]      # a missing dump is load_stage's to report
    for folder, f, rec in zip(models[1:], prepros[1:], records[1:]):
        if rec != records[0]:
            raise ValueError('%s: %s records the geometry %s, the first member\'s %s records %s: the members of an ensemble must see '
                             'the scan on one grid' % (folder, f, _geometry_text(rec), prepros[0], _geometry_text(records[0])))
    recorded = records[0]
    code = getattr(args, 'conform', None)
    if recorded is None:
        return code, coregister_kwargs(args)
    registering = coregister_kwargs(args, recorded.coregister)
    if code is None:
        print('Geometry (recorded by {}): {}'.format(prepros[0], _geometry_text(recorded._replace(coregister=registering))), flush=True)
        return recorded.orientation, registering
    if code != recorded.orientation:
        print('Warning: --conform {} over the record of {}, whose examples were conformed to {}'.format(code, prepros[0], recorded.orientation),
              flush=True)
    return code, registering


def _geometry_text(spec):
    if spec is None:
        return 'none'
    reg = spec.coregister
    return 'conform to %s at 1 mm%s' % (spec.orientation, '' if reg is None else ', co-register within %g mm and %g degrees on %d bins' % (
        reg['bounds'][0], reg['bounds'][1], reg['bins']))


def print_bias(name, modalities, results):
    """the one line per case of the bias-field correction: sweeps per level and final cv per modality"""
    print('{}. Bias-corrected {}'.format(name, '; '.join(n4.format_result(m, r) for m, r in zip(modalities, results))), flush=True)


def require_gpu():
    """-> the current device; no CPU path: without a GPU the command ends with the Interpolator's message"""
    Interpolator._device_volume(np.zeros((1, 1, 1, 1), dtype=np.float32))
    return torch.device('cuda', torch.cuda.current_device())


def _fmt(v):
    return '%.6f' % v


def score_row(name, s):
    return [name, _fmt(s['macro']), _fmt(s['micro'])] + [_fmt(v) for v in s['dice']] + [_fmt(s[k]) for k in ('wt', 'tc', 'et')]


def surface_row(s):
    """the columns --surface_metrics appends to a score_row"""
    return [_fmt(s[k]) for k in SURFACE_KEYS]


def lesion_columns(lw):
    """infer.lesionwise_scores' dict -> the values of LESION_KEYS by name"""
    out = {}
    for name, _ in BRATS_REGIONS:
        c = lw['lw_counts_' + name]
        out.update({'lw_dice_' + name: lw['lw_dice_' + name], 'lw_hd95_' + name: lw['lw_hd95_' + name], 'lw_lesions_' + name: c['lesions'],
                    'lw_fn_' + name: c['false_negatives'], 'lw_fp_' + name: c['false_positives']})
    return out


def lesion_row(s):
    """the columns --lesionwise appends to a score_row"""
    return [_fmt(s[k]) for k in LESION_SCORE_KEYS] + ['%d' % s[k] for k in LESION_COUNT_KEYS]


def mean_finite(values):
    """mean over the finite values, nan when there is none"""
    vals = [v for v in values if np.isfinite(v)]
    return float(np.mean(vals)) if vals else float('nan')


def _decoded(cases, args, conform=None):
    """the decoded cases in order; with workers > 0 a bounded number of them is decoded ahead by host threads.  conform: do the headers
    decide (default: as --conform says)"""
    if conform is None:
        conform = getattr(args, 'conform', None) is not None
    if args.workers <= 0:
        for _, path in cases:
            yield decode_case(path, args.modalities, args.truth, conform)
        return
    with ThreadPoolExecutor(max_workers=args.workers) as pool:
        pending, nxt = [], 0
        for _ in cases:
            while nxt < len(cases) and len(pending) < args.workers + 1:
                pending.append(pool.submit(decode_case, cases[nxt][1], args.modalities, args.truth, conform))
                nxt += 1
            yield pending.pop(0).result()


def run(args):
    """-> {'cases', 'scored', 'skipped': [(name, modality)], 'scores': [(name, label_scores dict)], 'total': scores of the summed
    confusion matrix or None, 'postprocess': [(name, counts)] of the cases a post-processing flag touched: the counts of
    infer.postprocess_labels, and 'brain_*' those of the skull stage's largest-component step}"""
    dev = require_gpu()
    Interpolator(args.modalities, order=args.order, mode=args.mode)      # refuses an unsupported --order / --mode before any work
    cases = find_cases(args.in_locs, args.out_loc)
    if not cases:
        raise ValueError('no case found under %s' % (args.in_locs,))
    if args.out_loc:
        os.makedirs(args.out_loc, exist_ok=True)
    tumor = skull = None
    scores, skipped, done, cleaned = [], [], 0, []
    post = postprocess_kwargs(args)
    largest = bool(getattr(args, 'skull_largest_component', False))
    lesion = lesion_kwargs(args)
    lesionwise = lesion is not None
    windowed = window_kwargs(args) is not None
    code, registering = geometry_rule(args)
    conf = Conformer(code, (1.0, 1.0, 1.0), args.order) if code is not None else None
    bias = bias_rule(args)
    unc_mode, unc_keys = getattr(args, 'uncertainty', None), ()
    total = np.zeros((N_CLASSES, N_CLASSES), dtype=np.int64)
    t0 = time.time()
    for (name, path), case in zip(cases, _decoded(cases, args, conf is not None)):
        if 'missing' in case:
            print('{}: no *{}*.nii* file, case skipped'.format(name, case['missing']), flush=True)
            skipped.append((name, case['missing']))
            continue
        if 'refused' in case:
            print('{}: {}, case skipped'.format(name, case['refused']), flush=True)
            skipped.append((name, case['refused']))
            continue
        geometry, affine = None, case['affine']
        if conf is None:
            x, y = upload_case(case, dev)
            if bias is not None:
                corrected = [n4.correct(x[..., ch].contiguous(), None, bias) for ch in range(x.shape[3])]
                for ch, r in enumerate(corrected):
                    x[..., ch].copy_(r.out)
                print_bias(name, args.modalities, corrected)
            pixdim = tuple(float(v) for v in case['pixdim'][1:4])
        else:
            vols, y = upload_conform_case(case, dev)
            if bias is not None:
                vols, corrected = n4.correct_case([v.contiguous() for v in vols], bias)
                print_bias(name, args.modalities, corrected)
            affines = case['affines']
            if registering is not None:
                affines, found = coreg.coregister_case(vols, affines, **registering)
                for mod, r in zip(args.modalities[1:], found[1:]):
                    print('{}. Coregistered {}'.format(name, coreg.format_result(mod, r)), flush=True)
            x, geometry, affine = None, (conf, vols, affines), case['affines'][0]
            plan = conf.plan([tuple(v.shape) for v in vols], affines)
            pixdim = plan['native_spacing']                      # the distances of the scores are taken on the native grid
            print('{}. Orientation {} -> {}, voxel size {:.4g} x {:.4g} x {:.4g} mm, {}'.format(
                name, plan['code'], conf.orientation, pixdim[0], pixdim[1], pixdim[2],
                'exact reorientation' if all(ro is not None for ro in plan['reorient']) else 'resampled at order %d' % conf.order), flush=True)
        if tumor is None:
            unit = all(f == 1.0 for f in pixdim)
            if conf is not None:
                shape_1mm = plan['shape']
            else:
                shape_1mm = tuple(x.shape[:3]) if unit else zoom_output_shape(tuple(x.shape[:3]), pixdim)
            members = [load_stage(folder, prepro, args, shape_1mm) for folder, prepro in zip(tumor_models(args), tumor_prepros(args))]
            tumor = members[0]
            if len(members) > 1 or unc_mode is not None:             # one model and no map: the code path there has always been
                print('Ensemble of {}: {}'.format(len(members), ', '.join(
                    '%s (%s)' % (f, m.targets) for f, m in zip(tumor_models(args), members))), flush=True)
                tumor = StageEnsemble(members, unc_mode)
                unc_keys = uncertainty_keys(tumor.targets)
            if args.skull_strip:
                skull = load_stage(args.skull_model, args.skull_prepro, args, shape_1mm)
                if largest:
                    skull.largest_component = True
        geo = {} if geometry is None else {'geometry': geometry}          # without --conform the call is the one it has always been
        unc = None
        if post is None and not largest and unc_mode is None:
            _, lab = segment_case(tumor, x, pixdim, skull=skull, order=args.order, **geo)
        elif post is None and not largest:
            _, lab, st = segment_case(tumor, x, pixdim, skull=skull, order=args.order, return_stages=True, **geo)
            unc = st['uncertainty']
        else:
            _, lab, st = segment_case(tumor, x, pixdim, skull=skull, order=args.order, return_stages=True, postprocess=post, **geo)
            unc = st.get('uncertainty')
            counts = dict(st.get('postprocess') or {})
            counts.update({'brain_' + k: v for k, v in (st.get('brain_counts') or {}).items()})
            cleaned.append((name, counts))
            print('{}. Post-processing: {}'.format(name, ', '.join('%s %d' % kv for kv in sorted(counts.items()))), flush=True)
        if windowed:
            print('{}. Windows run (skipped as empty): {}'.format(name, '. '.join(
                '%s %d (%d)' % ((what,) + stage.window_counts) for what, stage in (('skull', skull), ('tumor', tumor)) if stage is not None)),
                flush=True)
        s = None
        if y is not None:
            s = label_scores(y, lab, N_CLASSES)
            total += s['confusion']
            if args.surface_metrics:
                hd = surface_scores(y, lab, pixdim, N_CLASSES)
                s.update({k: hd[k] for k in HD95_KEYS})
                s.update(region_rates_from_confusion(s['confusion']))
            if lesionwise:
                s.update(lesion_columns(lesionwise_scores(y, lab, pixdim, N_CLASSES, **lesion)))
            if unc is not None:                                      # counted inside the brain mask the map was taken with
                brain = (st['uncertainty_mask'] > 0).to(torch.uint8).reshape(tuple(lab.shape)).contiguous()
                s.update(uncertainty_scores(y, lab.contiguous(), unc, brain, tumor.targets, N_CLASSES))
        where = os.path.join(args.out_loc, name) if args.out_loc else path
        os.makedirs(where, exist_ok=True)
        nifti.save(os.path.join(where, 'mask.nii'), lab.cpu().numpy(), affine)
        if unc is not None:
            levels = unc.cpu().numpy()
            for ch, fname in enumerate(UNCERTAINTY_FILE_NAMES[tumor.targets]):
                nifti.save(os.path.join(where, 'unc_%s.nii' % fname), np.ascontiguousarray(levels[..., ch]), affine)
        done += 1
        if s is not None:
            scores.append((name, s))
            print('{}. Macro: {ma: 1.4f}. Micro: {mi: 1.4f}'.format(name, ma=s['macro'], mi=s['micro']), flush=True)    # test.py:269
            if args.surface_metrics:
                print('{}. HD95 WT: {:1.4f}. TC: {:1.4f}. ET: {:1.4f}'.format(name, *[s[k] for k in HD95_KEYS]), flush=True)
            if lesionwise:
                print('{}. Lesion-wise Dice WT: {:1.4f}. TC: {:1.4f}. ET: {:1.4f}. HD95 WT: {:1.4f}. TC: {:1.4f}. ET: {:1.4f}. '
                      'Lesions (missed, false positives) WT: {:d} ({:d}, {:d}). TC: {:d} ({:d}, {:d}). ET: {:d} ({:d}, {:d})'.format(
                          name, *([s[k] for k in LESION_SCORE_KEYS] +
                                  [s['lw_%s_%s' % (what, r)] for r, _ in BRATS_REGIONS for what in ('lesions', 'fn', 'fp')])), flush=True)
            if unc is not None:
                print('{}. Uncertainty ({}) {}'.format(name, unc_mode, '. '.join('%s: %1.4f' % (k, s[k]) for k in unc_keys)), flush=True)
    overall = scores_from_confusion(total) if scores else None
    n_inf = 0
    if args.surface_metrics:
        n_inf = sum(1 for _, s in scores for k in HD95_KEYS if np.isinf(s[k]))
        if overall is not None:
            overall.update({k: mean_finite([s[k] for _, s in scores]) for k in HD95_KEYS})
            overall.update(region_rates_from_confusion(total))
    if lesionwise and overall is not None:
        overall.update({k: mean_finite([s[k] for _, s in scores]) for k in LESION_SCORE_KEYS})
        overall.update({k: sum(s[k] for _, s in scores) for k in LESION_COUNT_KEYS})
    if unc_keys and overall is not None:
        overall.update({k: mean_finite([s[k] for _, s in scores]) for k in unc_keys})
    if args.out_loc:
        head = ['case', 'macro', 'micro'] + ['dice_%d' % c for c in range(1, N_CLASSES)] + ['wt', 'tc', 'et']
        rows = [head] + [score_row(n, s) for n, s in scores]
        if overall is not None:
            rows.append(score_row('total', overall))
        if args.surface_metrics:
            extra = [list(SURFACE_KEYS)] + [surface_row(s) for _, s in scores] + ([surface_row(overall)] if overall is not None else [])
            rows = [r + e for r, e in zip(rows, extra)]
        if lesionwise:
            extra = [list(LESION_KEYS)] + [lesion_row(s) for _, s in scores] + ([lesion_row(overall)] if overall is not None else [])
            rows = [r + e for r, e in zip(rows, extra)]
        if unc_keys:
            extra = [list(unc_keys)] + [[_fmt(s[k]) for k in unc_keys] for _, s in scores] + (
                [[_fmt(overall[k]) for k in unc_keys]] if overall is not None else [])
            rows = [r + e for r, e in zip(rows, extra)]
        with open(os.path.join(args.out_loc, 'scores.csv'), 'w') as f:
            f.write(''.join(','.join(r) + '\n' for r in rows))
    dt = time.time() - t0
    print('{} cases segmented ({} scored) in {:.1f} s, {:.2f} cases/s; {} skipped for a missing modality{}'.format(
        done, len(scores), dt, done / dt if dt > 0 else 0.0, len(skipped),
        (': ' + ', '.join('%s (%s)' % sk for sk in skipped) if skipped else '') +
        ('; {} region distances infinite (a region empty in one of the two maps)'.format(n_inf) if args.surface_metrics else '')), flush=True)
    return {'cases': done, 'scored': len(scores), 'skipped': skipped, 'scores': scores, 'total': overall, 'postprocess': cleaned}


def main(argv=None):
    args = parse_args(argv)
    print('Test args: {}'.format(args))
    run(args)
    return 0


if __name__ == '__main__':
    sys.exit(main())
