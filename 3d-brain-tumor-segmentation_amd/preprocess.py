"""Dataset preprocessing on the device: folders of NIfTI scans -> train-ready examples (reference preprocess.py:12-131).

    python -m bts_amd.preprocess --in_locs a,b --modalities t1ce,flair --truth seg [--create_val] [--out_loc ./data]
                                 [--norm dataset|case] [--clip_percentiles LO,HI]
                                 [--bias_correct [--bias_shrink 4] [--bias_levels 4] [--bias_iters 50] [--bias_threshold 0.001]
                                  [--bias_fwhm 0.15]]

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
    `bias` entry with the spec, and `python -m bts_amd.test` corrects each scan the same way (`load_bias`).
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


def create_dataset(locs, modalities, truth, device=None, workers=8, bias=None):
    """-> (x, y, size): lists of device views (h,w,d,c) / (h,w,d,1) of the resident raw volumes, restricted to the bounding box
    common to all cases, and size = {'h','w','d','c'}   [preprocess.py:17-65]
    Every entry of every folder of `locs` is a case; folders and cases are visited in sorted order (the reference visits them in
    the file system's order).  Files are decoded by `workers` threads.  `y` holds the labels as stored; see `remap_labels`.
    bias: None or the n4.N4Spec every modality is corrected with right after upload."""
    dev = _device(device)
    cases = [p for loc in locs for p in sorted(glob.glob(os.path.join(loc, '*')))]
    if not cases:
        raise ValueError('no case found under %s' % (list(locs),))
    names = list(modalities) + [truth]
    c = len(modalities)
    xs, ys, shape, occ = [], [], None, None
    workers = max(1, int(workers))
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


def prepro_record(size, mean, std, norm='dataset', clip=None, bias=None):
    """what prepro.npy holds: {'size', 'norm': {'mean', 'std'}} as the reference writes it; the mode and the clip percentiles with norm
    'case'; and a `bias` entry (n4.spec_record) only where the examples were bias-corrected.  Without the new options the file is byte for
    byte what it has always been"""
    nd = {'mode': 'case', 'clip': clip, 'mean': mean, 'std': std} if norm == 'case' else {'mean': mean, 'std': std}
    rec = {'size': size, 'norm': nd}
    if bias is not None:
        rec['bias'] = n4.spec_record(bias)
    return rec


def preprocess(in_locs, modalities, truth, out_loc, create_val=False, device=None, workers=8, norm='dataset', clip=None, bias=None):
    """the reference's main (preprocess.py:99-131): out_loc/train/{i}.npz, out_loc/val/{i}.npz (arrays x (h,w,d,c) and y (h,w,d,1),
    float32) and out_loc/prepro.npy -> {'size', 'mean', 'std', 'n_train', 'n_val'}
    An existing out_loc is REMOVED with everything in it and created anew before any scan is read, as the reference's argument
    parser does (args.py:73-74, `make_dirs`); an out_loc that is or contains one of `in_locs` raises ValueError and removes
    nothing.
    norm: 'dataset' (the default: one mean and deviation per channel over the training cases, `compute_norm`, as the reference) |
    'case' (every case on its own brain voxels, `normalize_case`, as the paper the model comes from; `compute_norm` is not run and
    prepro.npy records the mode with an identity mean / std, so that every reader of the file keeps working).  clip: None or the
    percentiles (lo, hi) of a case's brain voxels its intensities are clamped to first; 'case' only.  bias: None or the n4.N4Spec of the
    bias-field correction every modality gets first; prepro.npy then records it as `bias` (`prepro_record`)."""
    if norm not in NORM_MODES:
        raise ValueError('norm must be one of %s, got %r' % (NORM_MODES, norm))
    clip = ops.check_clip(clip)
    if clip is not None and norm != 'case':
        raise ValueError("clip needs norm='case'")
    bias = n4.check_spec(bias) if bias is not None else None
    _refuse_inputs_inside(out_loc, in_locs)
    train_loc, val_loc = make_dirs(out_loc)
    x_train, y_train, size = create_dataset(in_locs, modalities, truth, device=device, workers=workers, bias=bias)
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
        np.save(os.path.join(out_loc, 'prepro.npy'), prepro_record(size, mean, std, norm, clip, bias))
        mean_d = std_d = None
    else:
        mean, std = compute_norm(x_train, len(modalities))
        np.save(os.path.join(out_loc, 'prepro.npy'), prepro_record(size, mean, std, norm, clip, bias))
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
    return p


def norm_kwargs(args):
    """-> the norm / clip keyword arguments of `preprocess` the flags ask for"""
    return {'norm': getattr(args, 'norm', 'dataset'), 'clip': getattr(args, 'clip_percentiles', None)}


def parse_args(argv=None):
    parser = arg_parser()
    args = parser.parse_args(argv)
    if hasattr(args, 'clip_percentiles') and getattr(args, 'norm', 'dataset') != 'case':
        parser.error('--clip_percentiles needs --norm case')
    bias_spec(args, parser)
    args.in_locs = args.in_locs.split(',')
    args.modalities = args.modalities.split(',')
    return args


def main(argv=None):
    args = parse_args(argv)
    print('Preprocess args: {}'.format(args))
    r = preprocess(args.in_locs, args.modalities, args.truth, args.out_loc, create_val=args.create_val, bias=bias_spec(args), **norm_kwargs(args))
    print('mean {} std {}'.format(r['mean'].reshape(-1), r['std'].reshape(-1)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
