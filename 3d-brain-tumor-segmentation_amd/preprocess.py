"""Dataset preprocessing on the device: folders of NIfTI scans -> train-ready examples (reference preprocess.py:12-131).

    python -m bts_amd.preprocess --in_locs a,b --modalities t1ce,flair --truth seg [--create_val] [--out_loc ./data]
                                 [--norm dataset|case] [--clip_percentiles LO,HI]
                                 [--bias_correct [--bias_shrink 4] [--bias_levels 4] [--bias_iters 50] [--bias_threshold 0.001]
                                  [--bias_fwhm 0.15]]
                                 [--conform [CODE] [--label_interp vote|nearest]
                                  [--coregister [--coregister_max_mm 30] [--coregister_max_deg 20] [--coregister_bins 32]]]

The names, the argument order and the results are the reference's: `create_dataset` finds the bounding box of all non-zero voxels
of all cases and crops every case to it, `compute_norm` gives the per-channel mean and standard deviation of the training cases,
`preprocess` (the reference's `main`) writes the normalised examples and `prepro.npy`.  What runs where: files are decoded on a
thread pool of the host (bts_amd.nifti; zlib releases the GIL), each volume is uploaded once and stays resident, and the three
passes over the voxels are kernels of csrc/prepro.hip (ops.prepro_occupancy, prepro_sums, prepro_crop_norm).

Quirks of the reference that are kept, because the sizes in prepro.npy and everything downstream depend on them:
  * the crop is [min:max] of the first / last occupied plane, so the last occupied plane of each axis is dropped and
    size = max - min (preprocess.py:55-63);
  * mean = sum(x) / #(x > 0) and std = sqrt(sum((x - mean)^2) / #(x > 0)): both sums run over every voxel of the crop, the count
    over the strictly positive ones only (preprocess.py:75-83);
  * "non-zero" is numpy's truth value: NaN counts, -0.0 does not (preprocess.py:39-47);
  * with create_val the validation set is the first len // 11 cases in visiting order (the shuffled index list of
    preprocess.py:105-106 is never used) and the statistics come from the training cases alone;
  * labels >= 4 become 3 (preprocess.py:36); files are numbered from 1 per folder.

Deviations:
  * cases are visited in sorted order of their paths; the reference's order is whatever glob returns, i.e. the file system's;
  * sum(x) is accumulated in float64.  The reference adds each volume up in float32 (np.sum of a float32 array) before it adds the
    volumes in float64; on real scans the totals pass 2^24 and that float32 sum is inexact, so its mean differs from ours in the
    low digits.  On integer-valued volumes whose per-volume totals stay below 2^24 the two are bit-equal;
  * the label rule is applied by the kernel that writes the example, not to the resident volume (`remap_labels` is the eager form);
  * examples are stored as `.npz` files with the arrays `x` and `y`, the form data.prepare_dataset reads, not as TFRecords;
  * --norm case (off by default) normalises every case on its own brain voxels instead, as the paper the model comes from does, with
    --clip_percentiles LO,HI after clamping them to robust percentiles (`normalize_case`, ops.case_norm, csrc/casenorm.hip); prepro.npy
    then records the mode, and `python -m bts_amd.test` normalises each scan the same way (`load_norm`);
  * --bias_correct (off by default) removes the coil shading of every modality of every case by N4 (bts_amd.n4, csrc/n4.hip) right after
    upload, before the bounding box, the statistics and the normalisation, on that modality's own positive voxels; prepro.npy then gains a
    `bias` entry with the spec, and `python -m bts_amd.test` corrects each scan the same way (`load_bias`);
  * --conform [CODE] (off by default) lets the NIfTI headers decide where the voxels are, as `python -m bts_amd.test --conform` does.  The
    modalities of a case, and the cases, may differ in shape.  Per case, on the device (`conform_case`): N4 on each modality's own grid
    where asked for; with --coregister the modalities after the first are registered to it (bts_amd.coreg) and the truth follows the
    modality on whose grid it lies (`truth_follows`); infer.Conformer brings the scan onto one 1 mm grid of that orientation; the labels
    go there by an exact reorientation where one does it, else by vote (ops.label_resample3d, csrc/conform.hip: the 8 linear taps vote
    with their weights, the strongest value wins, of equal ones the smallest -- nnU-Net's rule, one gather) or, with --label_interp
    nearest, at order 0.  Each case is cropped to its OWN occupancy box and centred on a zero canvas of the largest box
    (`canvas_layout`), and the statistics, the normalisation and the files run on those canvases.  Here the box is the full one, [first
    occupied plane, last occupied plane + 1): the reference's dropped last plane (first quirk above) belongs to the default mode and is
    not carried into this one.  prepro.npy gains a `geometry` entry, and `python -m bts_amd.test` conforms each scan the same way
    (`load_geometry`).
"""
import argparse
import collections
import glob
import os
import shutil
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import n4, nifti, ops


def get_npy_image(path, name):
    """float32 array of the first file, in sorted order, that matches path/*<name>.nii* (preprocess.py:12-14)"""
    found = sorted(glob.glob(os.path.join(path, '*' + name + '.nii' + '*')))
    if not found:
        raise ValueError('%s: no file matches *%s.nii*' % (path, name))
    return np.asarray(nifti.load(found[0])[0]).astype(np.float32)


def remap_labels(y):
    """labels >= 4 -> 3 (preprocess.py:36), a new tensor or array; `normalize_example` applies the same rule when it writes"""
    if isinstance(y, torch.Tensor):
        return torch.where(y >= 4, torch.full_like(y, 3.0), y)
    y = np.array(y, copy=True)
    y[y >= 4] = 3
    return y


def _device(device):
    return torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())


def _decode_case(path, names):
    """every volume of one case as a C-contiguous float32 array with the axes reversed (NIfTI data is Fortran-ordered, so this is
    the file's own byte order and costs no transposition on the host)"""
    return [np.ascontiguousarray(get_npy_image(path, name).T) for name in names]


def _upload_case(vols, dev, bias=None):
    """the decoded volumes of one case (axes reversed, see `_decode_case`) -> resident x (h,w,d,c) and y (h,w,d,1); bias: None or the
    N4Spec every modality is corrected with on its own positive voxels before it is stored"""
    c = len(vols) - 1
    x = torch.empty(vols[0].shape[::-1] + (c,), dtype=torch.float32, device=dev)
    for ch in range(c):
        v = torch.from_numpy(vols[ch]).to(dev).permute(2, 1, 0)
        x[..., ch].copy_(v if bias is None else n4.correct(v.contiguous(), None, bias).out)
    y = torch.from_numpy(vols[c]).to(dev).permute(2, 1, 0).contiguous().unsqueeze(-1)
    return x, y


def create_dataset(locs, modalities, truth, device=None, workers=8, bias=None, geometry=None):
    """-> (x, y, size): lists of device views (h,w,d,c) / (h,w,d,1) of the resident raw volumes, restricted to the bounding box
    common to all cases, and size = {'h','w','d','c'}   [preprocess.py:17-65]
    Every entry of every folder of `locs` is a case; folders and cases are visited in sorted order (the reference visits them in
    the file system's order).  Files are decoded by `workers` threads.  `y` holds the labels as stored; see `remap_labels`.
    bias: None or the n4.N4Spec every modality is corrected with right after upload.
    geometry: None, or the GeometrySpec by which the headers decide where the voxels are: the modalities of a case, and the cases, may then
    differ in shape; every case is conformed to one oriented 1 mm grid (`conform_case`), cropped to its own FULL occupancy box and centred
    on a dense zero canvas of the per-axis largest box (`canvas_layout`), which is `size`; x and y are those canvases."""
    dev = _device(device)
    cases = [p for loc in locs for p in sorted(glob.glob(os.path.join(loc, '*')))]
    if not cases:
        raise ValueError('no case found under %s' % (list(locs),))
    workers = max(1, int(workers))
    if geometry is not None:
        return _create_dataset_conformed(cases, list(modalities), truth, dev, workers, bias, check_geometry(geometry))
    names = list(modalities) + [truth]
    c = len(modalities)
    xs, ys, shape, occ = [], [], None, None
    with ThreadPoolExecutor(max_workers=workers) as pool:
        pending, nxt = [], 0
        for k, path in enumerate(cases):
            while nxt < len(cases) and len(pending) < 2 * workers:       # bounded look-ahead: decoded volumes wait on the host
                pending.append(pool.submit(_decode_case, cases[nxt], names))
                nxt += 1
            vols = pending.pop(0).result()
            for v in vols:
                if v.ndim != 3:
                    raise ValueError('%s: a volume of rank %d, expected 3' % (path, v.ndim))
                if v.shape != vols[0].shape:
                    raise ValueError('%s: the volumes of this case differ in shape: %s' % (path, [u.shape[::-1] for u in vols]))
            if shape is None:
                shape = vols[0].shape[::-1]
                need = len(cases) * int(np.prod(shape)) * (c + 1) * 4
                free = torch.cuda.mem_get_info(dev)[0]
                if need > free:
                    raise MemoryError('the dataset stays resident on the device: %d cases of %s x %d channels + labels need %.1f GB, '
                                      '%.1f GB are free on %s' % (len(cases), shape, c, need / 1e9, free / 1e9, dev))
                occ = torch.zeros((len(cases), sum(shape)), dtype=torch.int32, device=dev)
            elif vols[0].shape[::-1] != shape:
                raise ValueError('%s: shape %s differs from the %s of %s' % (path, vols[0].shape[::-1], shape, cases[0]))
            x_, y_ = _upload_case(vols, dev, bias)
            ops.prepro_occupancy(x_, occ[k])
            xs.append(x_)
            ys.append(y_)
    occ_h = occ.cpu().numpy()                                               # the one read-back of the search
    for k, path in enumerate(cases):
        if not occ_h[k].any():
            raise ValueError('%s: the case has no non-zero voxel' % path)
    total = occ_h.any(axis=0)
    lo, hi, off = [], [], 0
    for n in shape:
        idx = np.nonzero(total[off:off + n])[0]
        lo.append(int(idx[0]))
        hi.append(int(idx[-1]))
        off += n
    if min(h - l for l, h in zip(lo, hi)) < 1:
        raise ValueError('the bounding box [%s, %s) of %s has an axis of zero extent (the last occupied plane is dropped)'
                         % (lo, hi, cases[0] if len(cases) == 1 else '%d cases' % len(cases)))
    x = [v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], :] for v in xs]
    y = [v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], :] for v in ys]
    size = {'h': hi[0] - lo[0], 'w': hi[1] - lo[1], 'd': hi[2] - lo[2], 'c': c}
    print('Maximal crop size: [{}, {}, {}, {}]'.format(size['h'], size['w'], size['d'], size['c']))
    return x, y, size


LABEL_INTERPS = ('vote', 'nearest')
GEOMETRY_SPACING = (1.0, 1.0, 1.0)
GeometrySpec = collections.namedtuple('GeometrySpec', ('orientation', 'label_interp', 'coregister'))
GeometrySpec.__new__.__defaults__ = ('LPS', 'vote', None)
GeometrySpec.__doc__ = """how `preprocess(geometry=...)` places every case: the orientation code of the 1 mm grid, how the labels get there where
that is no exact reorientation ('vote' | 'nearest'), and the keyword arguments of coreg.coregister_case ({'bounds': (mm, degrees),
'bins': n}) or None where the modalities are not registered first"""


def check_geometry(spec):
    """-> the spec with plain Python values; ValueError for a code that is none, another label rule or bounds out of range"""
    if not isinstance(spec, GeometrySpec):
        raise ValueError('geometry must be a GeometrySpec, got %r' % (spec,))
    nifti.reorientation(str(spec.orientation), str(spec.orientation))
    if spec.label_interp not in LABEL_INTERPS:
        raise ValueError('geometry: label_interp must be one of %s, got %r' % (LABEL_INTERPS, spec.label_interp))
    reg = spec.coregister
    if reg is not None:
        try:
            mm, deg = (float(v) for v in reg['bounds'])
            bins = reg['bins']
            ok = set(reg) == {'bounds', 'bins'} and 0 < mm < float('inf') and 0 < deg <= 180 and not isinstance(bins, bool) \
                and int(bins) == bins and 2 <= int(bins) <= 64
        except (TypeError, ValueError, KeyError):
            ok = False
        if not ok:
            raise ValueError("geometry: coregister must be None or {'bounds': (mm > 0, 0 < degrees <= 180), 'bins': 2..64}, got %r" % (reg,))
        reg = {'bounds': (mm, deg), 'bins': int(bins)}
    return GeometrySpec(str(spec.orientation), spec.label_interp, reg)


def geometry_record(spec):
    """the spec as the plain dict prepro.npy's `geometry` entry holds; `geometry_from_record` is its inverse"""
    spec = check_geometry(spec)
    return {'orientation': spec.orientation, 'spacing': GEOMETRY_SPACING, 'label_interp': spec.label_interp,
            'coregister': None if spec.coregister is None else dict(spec.coregister)}


def geometry_from_record(d):
    try:
        spacing = tuple(float(v) for v in d['spacing'])
        spec = GeometrySpec(d['orientation'], d['label_interp'], d['coregister'])
    except (TypeError, ValueError, KeyError):
        raise ValueError('not a geometry record: %r' % (d,))
    if spacing != GEOMETRY_SPACING:
        raise ValueError('a geometry record of spacing %s: only %s is supported' % (spacing, GEOMETRY_SPACING))
    return check_geometry(spec)


def truth_grid_shift(shape, affine, truth_shape, truth_affine):
    """how far, in voxels along any axis, the truth volume's affine moves a corner of the reference grid from where the reference's own
    puts it; None when the shapes differ"""
    if tuple(int(v) for v in shape) != tuple(int(v) for v in truth_shape):
        return None
    n = [float(int(v) - 1) for v in shape]
    corners = np.array([[a, b, c, 1.0] for a in (0.0, n[0]) for b in (0.0, n[1]) for c in (0.0, n[2])], dtype=np.float64).T
    moved = np.linalg.inv(np.asarray(affine, dtype=np.float64)) @ np.asarray(truth_affine, dtype=np.float64) @ corners
    return float(np.abs(moved[:3] - corners[:3]).max())


def truth_follows(shapes, affines, truth_shape, truth_affine):
    """-> the index of the first modality on whose grid the truth volume lies (the same shape, and within 1e-3 voxel at the corners:
    `truth_grid_shift`), None where it lies on none.  Co-registration moves the truth with that modality: on the first one's grid it
    stays where it is, on no modality's grid it keeps its own affine"""
    for c, (shape, affine) in enumerate(zip(shapes, affines)):
        off = truth_grid_shift(shape, affine, truth_shape, truth_affine)
        if off is not None and off <= 1e-3:
            return c
    return None


def canvas_layout(extents):
    """the boxes of all cases on one canvas: extents, one (e0, e1, e2) per case -> (size, offsets): size the per-axis maximum, and per
    case the corner (size - extent) // 2 its box is put at, so an odd remainder goes to the high side"""
    ext = [tuple(int(v) for v in e) for e in extents]
    if not ext or any(len(e) != 3 or min(e) < 1 for e in ext):
        raise ValueError('canvas_layout: one positive (e0, e1, e2) per case, got %r' % (extents,))
    size = tuple(max(e[a] for e in ext) for a in range(3))
    return size, [tuple((size[a] - e[a]) // 2 for a in range(3)) for e in ext]


def _decode_case_headers(path, names):
    """as `_decode_case`, with each volume's own best affine (nifti.best_affine) -> [(array with the axes reversed, 4x4 float64)]; a
    header without an orientation refuses the case by path"""
    out = []
    for name in names:
        found = sorted(glob.glob(os.path.join(path, '*' + name + '.nii' + '*')))
        if not found:
            raise ValueError('%s: no file matches *%s.nii*' % (path, name))
        data, header = nifti.load(found[0])
        try:
            affine = nifti.best_affine(header)
        except ValueError as e:
            raise ValueError('%s: %s: %s' % (path, os.path.basename(found[0]), e))
        out.append((np.ascontiguousarray(np.asarray(data).astype(np.float32).T), affine))
    return out


def conform_case(vols, affines, truth, truth_affine, geometry, bias=None):
    """one case onto the grid `geometry` names, everything on the device.  vols: one (D,H,W) float32 device volume per modality, each on
    its own grid; affines: their 4x4 voxel -> world matrices; truth: the (D,H,W) float32 label volume and its affine.
    In this order: N4 per modality on its native grid (bias); with geometry.coregister, coreg.coregister_case corrects the affines of
    modalities 1 and up, and the truth's where it lies on the grid of one of them (`truth_follows`); infer.Conformer(orientation) gives x
    on the target grid; the labels are read through M_y = inv(A_truth) @ target_affine -- ops.reorient3d where that is an exact
    reorientation (infer.signed_permutation), else ops.label_resample3d ('vote') or ops.affine_resample3d at order 0 ('nearest').  A truth
    whose affine IS a modality's takes that modality's matrix of the plan, the same product as the Conformer forms it.
    -> {'x' (D,H,W,C), 'y' (D,H,W,1), 'plan', 'affines', 'truth_affine', 'truth_matrix' (M_y), 'follows', 'coreg': [None, CoregResult...]
    or None, 'bias': [N4Result...] or None, 'label_path': 'reorient' | 'vote' | 'nearest'}"""
    from . import coreg, infer
    geometry = check_geometry(geometry)
    shapes = [tuple(int(s) for s in v.shape) for v in vols]
    affines = [np.asarray(a, dtype=np.float64) for a in affines]
    truth_affine = np.asarray(truth_affine, dtype=np.float64)
    truth_shape = tuple(int(s) for s in truth.shape[:3])
    corrected = None
    if bias is not None:
        vols, corrected = n4.correct_case([v.contiguous() for v in vols], bias)
    follows = truth_follows(shapes, affines, truth_shape, truth_affine)
    found = None
    if geometry.coregister is not None:
        affines, found = coreg.coregister_case(vols, affines, **geometry.coregister)
        if follows:                                                     # on the first modality's grid, or on none: not moved
            truth_affine = np.linalg.inv(found[follows].matrix) @ truth_affine
    conf = infer.Conformer(geometry.orientation, GEOMETRY_SPACING)
    x, _, shape = conf.forward(vols, affines)
    plan = conf.last
    shape = tuple(shape)
    m_y = (np.linalg.inv(truth_affine) @ plan['target_affine'])[:3]
    for c, a in enumerate(affines):
        if shapes[c] == truth_shape and np.array_equal(a, truth_affine):
            m_y = plan['matrices'][c]
            break
    y = truth.reshape(truth_shape + (1,)).contiguous()
    ro = infer.signed_permutation(m_y, truth_shape, shape)
    if ro is not None:
        how = 'reorient'
        y = y if ro == infer.IDENTITY_REORIENTATION else ops.reorient3d(y, *ro)
    elif geometry.label_interp == 'vote':
        how, y = 'vote', ops.label_resample3d(y, m_y, shape)
    else:
        how, y = 'nearest', ops.affine_resample3d(y, m_y, shape, order=0)
    return {'x': x, 'y': y, 'plan': plan, 'affines': affines, 'truth_affine': truth_affine, 'truth_matrix': m_y, 'follows': follows,
            'coreg': found, 'bias': corrected, 'label_path': how}


def _create_dataset_conformed(cases, modalities, truth, dev, workers, bias, geometry):
    """`create_dataset` with a geometry: every case conformed by its headers (`conform_case`), cropped to its OWN full occupancy box and
    centred on a zero canvas of the largest box (`canvas_layout`)"""
    from . import coreg
    names = list(modalities) + [truth]
    c = len(modalities)
    xs, ys, occs = [], [], []
    with ThreadPoolExecutor(max_workers=workers) as pool:
        pending, nxt = [], 0
        for k, path in enumerate(cases):
            while nxt < len(cases) and len(pending) < 2 * workers:
                pending.append(pool.submit(_decode_case_headers, cases[nxt], names))
                nxt += 1
            decoded = pending.pop(0).result()
            for v, _ in decoded:
                if v.ndim != 3:
                    raise ValueError('%s: a volume of rank %d, expected 3' % (path, v.ndim))
            vols = [torch.from_numpy(v).to(dev).permute(2, 1, 0) for v, _ in decoded[:c]]
            y = torch.from_numpy(decoded[c][0]).to(dev).permute(2, 1, 0).contiguous()
            try:
                plan = _planned_extent(geometry, [tuple(v.shape) for v in vols], [a for _, a in decoded[:c]])
            except ValueError as e:
                raise ValueError('%s: %s' % (path, e))
            need = 2 * int(np.prod(plan)) * (c + 1) * 4                      # the conformed case and, later, its canvas
            free = torch.cuda.mem_get_info(dev)[0]
            if need > free:
                raise MemoryError('the dataset stays resident on the device: case %d of %d, %s, conformed to %s x %d channels + labels '
                                  'needs %.1f GB, %.1f GB are free on %s' % (k + 1, len(cases), path, plan, c, need / 1e9, free / 1e9, dev))
            try:
                r = conform_case(vols, [a for _, a in decoded[:c]], y, decoded[c][1], geometry, bias)
            except ValueError as e:
                raise ValueError('%s: %s' % (path, e))
            if r['coreg'] is not None:
                for mod, res in zip(modalities[1:], r['coreg'][1:]):
                    print('{}. Coregistered {}'.format(os.path.basename(path.rstrip(os.sep)), coreg.format_result(mod, res)), flush=True)
            occ = torch.zeros(sum(r['x'].shape[:3]), dtype=torch.int32, device=dev)
            ops.prepro_occupancy(r['x'], occ)
            xs.append(r['x'])
            ys.append(r['y'])
            occs.append(occ)
    occ_h = torch.cat(occs).cpu().numpy()                                   # the one read-back of the search
    boxes, off = [], 0
    for k, path in enumerate(cases):
        lo, hi = [], []
        for n in xs[k].shape[:3]:
            idx = np.nonzero(occ_h[off:off + n])[0]
            if not idx.size:
                raise ValueError('%s: the case has no non-zero voxel' % path)
            lo.append(int(idx[0]))
            hi.append(int(idx[-1]) + 1)                                     # the full box: the last occupied plane is kept
            off += n
        boxes.append((lo, hi))
    size3, offsets = canvas_layout([[h - l for l, h in zip(lo, hi)] for lo, hi in boxes])
    x, y = [], []
    for k, ((lo, hi), o) in enumerate(zip(boxes, offsets)):
        for src, dst, ch in ((xs, x, c), (ys, y, 1)):
            canvas = torch.zeros(size3 + (ch,), dtype=torch.float32, device=dev)
            canvas[o[0]:o[0] + hi[0] - lo[0], o[1]:o[1] + hi[1] - lo[1], o[2]:o[2] + hi[2] - lo[2]].copy_(
                src[k][lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]])
            dst.append(canvas)
            src[k] = None                                                   # the conformed volume is released as its canvas is made
    size = {'h': size3[0], 'w': size3[1], 'd': size3[2], 'c': c}
    print('Maximal crop size: [{}, {}, {}, {}]'.format(size['h'], size['w'], size['d'], size['c']))
    return x, y, size


def _planned_extent(geometry, shapes, affines):
    """the extent a case will have on the target grid, from its headers alone"""
    from . import infer
    return infer.Conformer(geometry.orientation, GEOMETRY_SPACING).plan(shapes, affines)['shape']


def compute_norm(x_train, in_ch):
    """-> (mean, std), numpy float64 of shape (1,1,1,in_ch)   [preprocess.py:68-85]
    Two passes of ops.prepro_sums over the device views; the divisions and the square root run in float64 on the host."""
    if not x_train:
        raise ValueError('compute_norm needs at least one training case')
    dev = x_train[0].device
    acc = torch.zeros(2 * in_ch, dtype=torch.float64, device=dev)
    for x in x_train:
        ops.prepro_sums(x, acc)
    acc = acc.cpu().numpy()
    n = acc[in_ch:].reshape(1, 1, 1, in_ch)
    mean = acc[:in_ch].reshape(1, 1, 1, in_ch) / n
    mean_d = torch.from_numpy(np.ascontiguousarray(mean.reshape(-1))).to(dev)
    acc2 = torch.zeros(in_ch, dtype=torch.float64, device=dev)
    for x in x_train:
        ops.prepro_sums(x, acc2, mean=mean_d)
    std = np.sqrt(acc2.cpu().numpy().reshape(1, 1, 1, in_ch) / n)
    return mean, std


def _stats_on(dev, v):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))).to(dev)


def normalize_example(x, y, mean, std):
    """device views x (h,w,d,c), y (h,w,d,1) -> dense device (float32((x - mean) / std) evaluated in float64, y with labels
    >= 4 -> 3)   [preprocess.py:36,124]; mean / std: anything of c values (numpy, or float64 tensors already on the device)"""
    m = mean if isinstance(mean, torch.Tensor) else _stats_on(x.device, mean)
    s = std if isinstance(std, torch.Tensor) else _stats_on(x.device, std)
    return ops.prepro_crop_norm(x, y, m, s)


def normalize_case(x, y, clip=None):
    """device views x (h,w,d,c), y (h,w,d,1) of ONE case -> dense device (x normalised on the case's own brain voxels, y with labels
    >= 4 -> 3): zero mean and unit deviation per channel over the voxels where any channel is > 0 (the brain mask of test.py:53-54),
    after clamping them to the percentiles clip = (lo, hi) when given; 0 outside the mask (ops.case_norm, one call, no host round trip)"""
    xn, yn, _ = ops.case_norm(x, None, clip, y=y)
    return xn, yn


def make_dirs(out_loc):
    """the folders of PreproArgParser.parse_args (args.py:72-81): out_loc is replaced if it exists -> (train_loc, val_loc)"""
    if os.path.isdir(out_loc):
        shutil.rmtree(out_loc)
    train_loc, val_loc = os.path.join(out_loc, 'train'), os.path.join(out_loc, 'val')
    os.mkdir(out_loc)
    os.mkdir(train_loc)
    os.mkdir(val_loc)
    return train_loc, val_loc


def _write(folder, x, y, mean_d, std_d, norm='dataset', clip=None):
    for i, (xv, yv) in enumerate(zip(x, y), 1):
        xn, yn = normalize_example(xv, yv, mean_d, std_d) if norm == 'dataset' else normalize_case(xv, yv, clip)
        np.savez(os.path.join(folder, '{}.npz'.format(i)), x=xn.cpu().numpy(), y=yn.cpu().numpy())


def _refuse_inputs_inside(out_loc, in_locs):
    out = os.path.realpath(out_loc)
    for loc in in_locs:
        real = os.path.realpath(loc)
        if real == out or real.startswith(out + os.sep):
            raise ValueError('out_loc %s is replaced as a whole and contains the input folder %s' % (out_loc, loc))


NORM_MODES = ('dataset', 'case')
BIAS_DEFAULTS = {'bias_shrink': 4, 'bias_levels': 4, 'bias_iters': 50, 'bias_threshold': 1e-3, 'bias_fwhm': 0.15}
BIAS_FIELDS = {'bias_shrink': 'shrink', 'bias_levels': 'levels', 'bias_iters': 'iters', 'bias_threshold': 'threshold', 'bias_fwhm': 'fwhm'}


def prepro_record(size, mean, std, norm='dataset', clip=None, bias=None, geometry=None):
    """what prepro.npy holds: {'size', 'norm': {'mean', 'std'}} as the reference writes it; the mode and the clip percentiles with norm
    'case'; a `bias` entry (n4.spec_record) only where the examples were bias-corrected; and a `geometry` entry (`geometry_record`) only
    where they were conformed by their headers.  Without the new options the file is byte for byte what it has always been"""
    nd = {'mode': 'case', 'clip': clip, 'mean': mean, 'std': std} if norm == 'case' else {'mean': mean, 'std': std}
    rec = {'size': size, 'norm': nd}
    if bias is not None:
        rec['bias'] = n4.spec_record(bias)
    if geometry is not None:
        rec['geometry'] = geometry_record(geometry)
    return rec


def preprocess(in_locs, modalities, truth, out_loc, create_val=False, device=None, workers=8, norm='dataset', clip=None, bias=None,
               geometry=None):
    """the reference's main (preprocess.py:99-131): out_loc/train/{i}.npz, out_loc/val/{i}.npz (arrays x (h,w,d,c) and y (h,w,d,1),
    float32) and out_loc/prepro.npy -> {'size', 'mean', 'std', 'n_train', 'n_val'}
    An existing out_loc is REMOVED with everything in it and created anew before any scan is read, as the reference's argument
    parser does (args.py:73-74, `make_dirs`); an out_loc that is or contains one of `in_locs` raises ValueError and removes
    nothing.
    norm: 'dataset' (the default: one mean and deviation per channel over the training cases, `compute_norm`, as the reference) |
    'case' (every case on its own brain voxels, `normalize_case`, as the paper the model comes from; `compute_norm` is not run and
    prepro.npy records the mode with an identity mean / std, so that every reader of the file keeps working).  clip: None or the
    percentiles (lo, hi) of a case's brain voxels its intensities are clamped to first; 'case' only.  bias: None or the n4.N4Spec of the
    bias-field correction every modality gets first; prepro.npy then records it as `bias` (`prepro_record`).  geometry: None or the
    GeometrySpec by which every case is conformed to one oriented 1 mm grid by its headers, the modalities registered to one another first
    where it says so, and the labels moved by vote (`create_dataset`); prepro.npy then records it as `geometry`."""
    if norm not in NORM_MODES:
        raise ValueError('norm must be one of %s, got %r' % (NORM_MODES, norm))
    clip = ops.check_clip(clip)
    if clip is not None and norm != 'case':
        raise ValueError("clip needs norm='case'")
    bias = n4.check_spec(bias) if bias is not None else None
    geometry = check_geometry(geometry) if geometry is not None else None
    _refuse_inputs_inside(out_loc, in_locs)
    train_loc, val_loc = make_dirs(out_loc)
    geo = {} if geometry is None else {'geometry': geometry}          # without one the calls are the ones they have always been
    x_train, y_train, size = create_dataset(in_locs, modalities, truth, device=device, workers=workers, bias=bias, **geo)
    x_val, y_val = [], []
    if create_val:
        split = len(x_train) // 11
        x_val, y_val = x_train[:split], y_train[:split]
        x_train, y_train = x_train[split:], y_train[split:]
        print('{} validation examples.'.format(len(x_val)))
    print('{} training examples.'.format(len(x_train)))
    if norm == 'case':
        if not x_train:
            raise ValueError('preprocess needs at least one training case')
        mean, std = np.zeros((1, 1, 1, len(modalities))), np.ones((1, 1, 1, len(modalities)))
        np.save(os.path.join(out_loc, 'prepro.npy'), prepro_record(size, mean, std, norm, clip, bias, **geo))
        mean_d = std_d = None
    else:
        mean, std = compute_norm(x_train, len(modalities))
        np.save(os.path.join(out_loc, 'prepro.npy'), prepro_record(size, mean, std, norm, clip, bias, **geo))
        dev = x_train[0].device
        mean_d, std_d = _stats_on(dev, mean), _stats_on(dev, std)
    _write(train_loc, x_train, y_train, mean_d, std_d, norm, clip)
    if create_val:
        _write(val_loc, x_val, y_val, mean_d, std_d, norm, clip)
    return {'size': size, 'mean': mean, 'std': std, 'n_train': len(x_train), 'n_val': len(x_val)}


def load_prepro(path):
    """prepro.npy -> ((h,w,d,c), mean (c,), std (c,)): what data.prepare_dataset(prepro_size=...) and
    infer.TestTimeAugmentor(mean, std, ...) take (args.py:166-167, test.py:107)"""
    p = np.load(path, allow_pickle=True).item()
    size = tuple(int(p['size'][k]) for k in ('h', 'w', 'd', 'c'))
    mean = np.asarray(p['norm']['mean'], dtype=np.float64).reshape(-1)
    std = np.asarray(p['norm']['std'], dtype=np.float64).reshape(-1)
    if mean.shape != (size[3],) or std.shape != (size[3],):
        raise ValueError('%s: mean / std of %d / %d values for %d channels' % (path, mean.size, std.size, size[3]))
    return size, mean, std


def load_bias(path):
    """prepro.npy -> the n4.N4Spec its examples were bias-corrected with, None where it records none"""
    rec = np.load(path, allow_pickle=True).item().get('bias')
    return n4.spec_from_record(rec) if rec is not None else None


def add_bias_flags(p):
    """--bias_correct and its sub-flags, shared with `python -m bts_amd.test`: in the namespace only where the command line gives them"""
    p.add_argument('--bias_correct', action='store_true', default=argparse.SUPPRESS,
                   help='Remove the coil shading of every modality by N4 bias-field correction on the device.')
    p.add_argument('--bias_shrink', type=int, default=argparse.SUPPRESS,
                   help='Stride of the lattice the field is estimated on (default: %d).' % BIAS_DEFAULTS['bias_shrink'])
    p.add_argument('--bias_levels', type=int, default=argparse.SUPPRESS,
                   help='Fitting levels, the spline mesh doubling from one to the next, 1..6 (default: %d).' % BIAS_DEFAULTS['bias_levels'])
    p.add_argument('--bias_iters', type=int, default=argparse.SUPPRESS,
                   help='Sweeps per level at most (default: %d).' % BIAS_DEFAULTS['bias_iters'])
    p.add_argument('--bias_threshold', type=float, default=argparse.SUPPRESS,
                   help='A level ends when the field changes by less than this coefficient of variation (default: %g).'
                        % BIAS_DEFAULTS['bias_threshold'])
    p.add_argument('--bias_fwhm', type=float, default=argparse.SUPPRESS,
                   help='Width of the Gaussian the log histogram is deconvolved by (default: %g).' % BIAS_DEFAULTS['bias_fwhm'])


def bias_spec(args, parser=None, recorded=None):
    """-> the n4.N4Spec the flags ask for: None without --bias_correct (then `recorded`, a prepro.npy's own spec, stands as it is); with
    it, the recorded spec or the defaults, each sub-flag given replacing its field.  A sub-flag without --bias_correct, or a value out of
    range, ends in parser.error (ValueError without a parser)"""
    def fail(msg):
        if parser is not None:
            parser.error(msg)
        raise ValueError(msg)
    given = {BIAS_FIELDS[k]: getattr(args, k) for k in BIAS_DEFAULTS if hasattr(args, k)}
    if not hasattr(args, 'bias_correct'):
        if given:
            fail('--bias_shrink, --bias_levels, --bias_iters, --bias_threshold and --bias_fwhm need --bias_correct')
        return recorded
    try:
        return n4.check_spec((recorded if recorded is not None else n4.N4Spec())._replace(**given))
    except ValueError as e:
        fail(str(e).replace('n4: ', '--bias_'))


def load_geometry(path):
    """prepro.npy -> the GeometrySpec its examples were conformed with, None where it records none"""
    rec = np.load(path, allow_pickle=True).item().get('geometry')
    try:
        return geometry_from_record(rec) if rec is not None else None
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))


COREGISTER_DEFAULTS = {'coregister_max_mm': 30.0, 'coregister_max_deg': 20.0, 'coregister_bins': 32}
CONFORM_HELP = 'Bring every modality onto one 1 mm grid of this orientation by its affine (default code: LPS), and the labels back.'


def code_arg(text):
    """--conform: an orientation code, one letter from each of R/L, A/P, S/I"""
    try:
        nifti.reorientation(text.upper(), text.upper())
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return text.upper()


def add_geometry_flags(p, conform_help=CONFORM_HELP, label_interp=False):
    """--conform, --coregister and its bounds, shared with `python -m bts_amd.test`, and with label_interp --label_interp: in the
    namespace only where the command line gives them (`coregister_kwargs` supplies COREGISTER_DEFAULTS)"""
    p.add_argument('--conform', type=code_arg, nargs='?', const='LPS', default=argparse.SUPPRESS, metavar='CODE', help=conform_help)
    p.add_argument('--coregister', action='store_true', default=argparse.SUPPRESS,
                   help='With --conform: register every modality to the first by mutual information and correct its affine.')
    p.add_argument('--coregister_max_mm', type=float, default=argparse.SUPPRESS,
                   help='Largest translation searched per axis, mm (default: %g).' % COREGISTER_DEFAULTS['coregister_max_mm'])
    p.add_argument('--coregister_max_deg', type=float, default=argparse.SUPPRESS,
                   help='Largest rotation searched per axis, degrees (default: %g).' % COREGISTER_DEFAULTS['coregister_max_deg'])
    p.add_argument('--coregister_bins', type=int, default=argparse.SUPPRESS,
                   help='Intensity bins per modality of the joint histogram, 2..64 (default: %d).' % COREGISTER_DEFAULTS['coregister_bins'])
    if label_interp:
        p.add_argument('--label_interp', type=str, choices=LABEL_INTERPS, default=argparse.SUPPRESS,
                       help="With --conform: how a label map is resampled where no exact reorientation does it: 'vote', each class "
                            "interpolated linearly and the strongest taken (default), or 'nearest'.")


def check_geometry_flags(args, parser):
    """the refusals of the flags of `add_geometry_flags`, through parser.error"""
    if hasattr(args, 'coregister') and not hasattr(args, 'conform'):
        parser.error('--coregister needs --conform: without it the modalities are stacked voxel for voxel and there is no affine to correct')
    if not hasattr(args, 'coregister') and any(hasattr(args, k) for k in COREGISTER_DEFAULTS):
        parser.error('--coregister_max_mm, --coregister_max_deg and --coregister_bins need --coregister')
    if not 0 < getattr(args, 'coregister_max_mm', 30.0) < float('inf'):
        parser.error('--coregister_max_mm must be positive')
    if not 0 < getattr(args, 'coregister_max_deg', 20.0) <= 180:
        parser.error('--coregister_max_deg must lie in (0, 180]')
    if not 2 <= getattr(args, 'coregister_bins', 32) <= 64:
        parser.error('--coregister_bins must lie in 2..64')
    if hasattr(args, 'label_interp') and not hasattr(args, 'conform'):
        parser.error('--label_interp needs --conform: without it the labels are stacked voxel for voxel like the scans')


def coregister_kwargs(args, recorded=None):
    """None without --coregister (then `recorded`, a prepro.npy's own, stands as it is), else the keyword arguments of
    coreg.coregister_case: the recorded ones or the defaults, each sub-flag given replacing its value"""
    if not getattr(args, 'coregister', False):
        return recorded
    v = dict(COREGISTER_DEFAULTS)
    if recorded is not None:
        v.update({'coregister_max_mm': recorded['bounds'][0], 'coregister_max_deg': recorded['bounds'][1], 'coregister_bins': recorded['bins']})
    v.update({k: getattr(args, k) for k in COREGISTER_DEFAULTS if hasattr(args, k)})
    return {'bounds': (float(v['coregister_max_mm']), float(v['coregister_max_deg'])), 'bins': int(v['coregister_bins'])}


def geometry_spec(args):
    """-> the GeometrySpec the flags ask for, None without --conform"""
    if getattr(args, 'conform', None) is None:
        return None
    return GeometrySpec(args.conform, getattr(args, 'label_interp', 'vote'), coregister_kwargs(args))


NormSpec = collections.namedtuple('NormSpec', ('mode', 'clip', 'mean', 'std'))


def load_norm(path):
    """prepro.npy -> NormSpec(mode, clip, mean (c,), std (c,)): how the examples of that dump were normalised, and so how a scan must be
    before the model trained on them sees it (infer.TestTimeAugmentor(norm=...)).  mode 'dataset': (x - mean) / std with the dump's
    statistics; a file that records no mode is one.  mode 'case': ops.case_norm with `clip`; mean / std are the identity."""
    _, mean, std = load_prepro(path)
    nd = np.load(path, allow_pickle=True).item()['norm']
    mode = nd.get('mode', 'dataset')
    if mode not in NORM_MODES:
        raise ValueError('%s: unknown normalisation mode %r' % (path, mode))
    clip = ops.check_clip(nd.get('clip'), '%s: clip' % path)
    if clip is not None and mode != 'case':
        raise ValueError("%s: clip percentiles with mode %r" % (path, mode))
    return NormSpec(mode, clip, mean, std)


def _clip_arg(text):
    """--clip_percentiles: LO,HI with 0 <= LO <= HI <= 100"""
    try:
        lo, hi = (float(v) for v in text.split(','))
    except ValueError:
        raise argparse.ArgumentTypeError('expected LO,HI (two percentiles), got %r' % (text,))
    if not 0.0 <= lo <= hi <= 100.0:
        raise argparse.ArgumentTypeError('expected 0 <= LO <= HI <= 100, got %r' % (text,))
    return lo, hi


def arg_parser():
    """the flags of the reference's PreproArgParser (args.py:51-61), and --norm / --clip_percentiles"""
    p = argparse.ArgumentParser(prog='python -m bts_amd.preprocess', description=__doc__.split('\n')[0])
    p.add_argument('--in_locs', type=str, required=True, help='Comma-separated list of paths to all data folders.')
    p.add_argument('--modalities', type=str, required=True, help='Comma-separated list of all input modalities to use.')
    p.add_argument('--truth', type=str, required=True, help='Truth label pattern to use.')
    p.add_argument('--create_val', action='store_true', default=False, help='Whether to create validation set.')
    p.add_argument('--out_loc', type=str, default='./data', help='Location to write preprocessed data.')
    # the two flags below exist in the namespace only where the command line gives them: a plain command line parses to what it
    # always has; `norm_kwargs` supplies the defaults
    p.add_argument('--norm', type=str, choices=NORM_MODES, default=argparse.SUPPRESS,
                   help="'dataset': one mean and deviation per channel over the training set (default); 'case': every case on its own "
                        'brain voxels.')
    p.add_argument('--clip_percentiles', type=_clip_arg, default=argparse.SUPPRESS, metavar='LO,HI',
                   help='With --norm case: clamp the brain voxels of each case to these percentiles first, e.g. 0.5,99.5.')
    add_bias_flags(p)
    add_geometry_flags(p, 'Let the NIfTI headers decide where the voxels are: bring every modality and the labels of every case onto one '
                          '1 mm grid of this orientation (default code: LPS); the cases may then differ in shape.', label_interp=True)
    return p


def norm_kwargs(args):
    """-> the norm / clip keyword arguments of `preprocess` the flags ask for"""
    return {'norm': getattr(args, 'norm', 'dataset'), 'clip': getattr(args, 'clip_percentiles', None)}


def parse_args(argv=None):
    parser = arg_parser()
    args = parser.parse_args(argv)
    if hasattr(args, 'clip_percentiles') and getattr(args, 'norm', 'dataset') != 'case':
        parser.error('--clip_percentiles needs --norm case')
    check_geometry_flags(args, parser)
    bias_spec(args, parser)
    args.in_locs = args.in_locs.split(',')
    args.modalities = args.modalities.split(',')
    return args


def main(argv=None):
    args = parse_args(argv)
    print('Preprocess args: {}'.format(args))
    geometry = geometry_spec(args)
    geo = {} if geometry is None else {'geometry': geometry}
    r = preprocess(args.in_locs, args.modalities, args.truth, args.out_loc, create_val=args.create_val, bias=bias_spec(args), **norm_kwargs(args),
                   **geo)
    print('mean {} std {}'.format(r['mean'].reshape(-1), r['std'].reshape(-1)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
