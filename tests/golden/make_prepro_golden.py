#!/usr/bin/env python3
"""Records tests/golden/prepro_vectors.npz for tests/test_prepro_host.py and tests/test_prepro_gpu.py (run from the repository root:
python tests/golden/make_prepro_golden.py <checkout of the reference>).

The reference's preprocess.py needs nibabel, tqdm, tensorflow and its own args module at import.  They are replaced here by
in-process stubs -- nibabel.load is backed by bts_amd.nifti.load, tqdm passes its iterable through, tensorflow and args are empty
shells (only the TFRecord writer and the command line use them, and neither is called).  The synthetic cases below are written as
`.nii.gz` files into a temporary folder, the reference's own create_dataset and compute_norm run on them, and (x - mean) / std is
applied as its main does.  Recorded per set, with the cases in the order the reference visited them:
  <set>_raw_x (n,S0,S1,S2,C) and <set>_raw_y (n,S0,S1,S2) as stored in the files, <set>_names (the visited folder names),
  <set>_lo / <set>_hi (box bounds), <set>_size (h,w,d,c), <set>_mean / <set>_std (C,) float64, <set>_x (n,h,w,d,C) float32 normalised,
  <set>_y (n,h,w,d,1) float32, <set>_n_val (validation cases taken from the front; 0 without create_val)
and `spec`, a JSON list of {set, modalities, truth, create_val}.  Data only: nothing of the reference's program text is recorded.
Run the result in a fresh interpreter: the reference's module is imported into this one."""
import glob
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'prepro_vectors.npz')
LIMIT = 505390                                        # the largest fixture already in tests/golden


def fill(rng, vol, box, hi_val, zero_share=0.25):
    """random integers 1..hi_val in box = ((a0,b0),(a1,b1),(a2,b2)) (inclusive), a share of them zeroed; corners kept non-zero so the
    box of the region is the box asked for"""
    sl = tuple(slice(a, b + 1) for a, b in box)
    v = rng.integers(1, hi_val + 1, size=vol[sl].shape).astype(vol.dtype)
    v[rng.random(v.shape) < zero_share] = 0
    v[0, 0, 0] = v[-1, -1, -1] = 7
    vol[sl] = v


def label_volume(rng, shape, values=(0, 1, 2, 4)):
    return rng.choice(np.array(values, dtype=np.int16), size=shape, p=[0.55] + [0.45 / (len(values) - 1)] * (len(values) - 1))


def set_a(rng):
    """5 cases of 19x13x11, two int16 modalities in 0..900.  Case 0 touches index 0 and the last index of axis 0; the upper bound
    of axis 1 is set by one voxel of one channel of case 3; every region starts at index 1 of axis 2, so the window origin is
    1 * C = 2 floats into a row (with C = 2 the product cannot be odd; 2 floats break 16-byte alignment all the same)."""
    shape, cases = (19, 13, 11), []
    boxes = [((0, 18), (3, 9), (1, 8)), ((2, 15), (2, 8), (2, 9)), ((4, 12), (4, 10), (1, 6)), ((5, 9), (5, 7), (3, 5)),
             ((1, 17), (2, 10), (1, 9))]
    for k, box in enumerate(boxes):
        mods = [np.zeros(shape, np.int16) for _ in range(2)]
        fill(rng, mods[0], box, 900)
        fill(rng, mods[1], tuple((a + 1, b - 1) for a, b in box), 900)
        if k == 3:
            mods[1][7, 11, 4] = 333                   # alone in its plane of axis 1: hi[1] = 11 comes from this voxel
        cases.append((mods, label_volume(rng, shape)))
    return dict(name='A', modalities=['t1ce', 'flair'], truth='seg', create_val=False), cases


def set_b(rng):
    """3 cases of 12x10x9, one int16 modality; the box starts at index 1 of axis 2: lo2 * C = 1 is odd; a label 5 among the 4s"""
    shape, cases = (12, 10, 9), []
    for box in [((2, 9), (1, 7), (1, 7)), ((3, 10), (2, 8), (2, 6)), ((2, 5), (3, 4), (3, 8))]:
        m = np.zeros(shape, np.int16)
        fill(rng, m, box, 900)
        cases.append(([m], label_volume(rng, shape, (0, 1, 2, 4, 5))))
    return dict(name='B', modalities=['t1'], truth='seg', create_val=False), cases


def set_c(rng):
    """11 cases of 8x8x8, four int16 modalities, create_val: 11 // 11 = 1 validation case"""
    shape, cases = (8, 8, 8), []
    for k in range(11):
        a = [int(v) for v in rng.integers(0, 3, 3)]
        b = [int(v) for v in rng.integers(5, 8, 3)]
        mods = [np.zeros(shape, np.int16) for _ in range(4)]
        for m in mods:
            fill(rng, m, tuple(zip(a, b)), 900)
        cases.append((mods, label_volume(rng, shape)))
    return dict(name='C', modalities=['t1', 't1ce', 't2', 'flair'], truth='seg', create_val=True), cases


def set_d(rng):
    """2 cases of 10x9x7, three float32 modalities: non-integer, non-negative values, a few negative voxels, one -0.0 outside the
    box (it must not widen it) and one plane of axis 0 (index 8) that holds nothing but one negative value (it must)"""
    shape, cases = (10, 9, 7), []
    for k, box in enumerate([((1, 6), (1, 7), (1, 5)), ((2, 7), (2, 6), (2, 6))]):
        mods = []
        for c in range(3):
            m = np.zeros(shape, np.float32)
            sl = tuple(slice(a, b + 1) for a, b in box)
            v = (rng.random(m[sl].shape) * 700.0 + 0.125).astype(np.float32)
            v[rng.random(v.shape) < 0.25] = 0.0
            v[rng.random(v.shape) < 0.03] *= np.float32(-0.01)
            v[0, 0, 0] = v[-1, -1, -1] = np.float32(3.3)
            m[sl] = v
            mods.append(m)
        if k == 0:
            mods[1][0, 0, 0] = np.float32(-0.0)
            mods[2][8, 4, 3] = np.float32(-12.75)
        cases.append((mods, label_volume(rng, shape)))
    return dict(name='D', modalities=['t1', 't2', 'flair'], truth='seg', create_val=False), cases


def install_stubs():
    from bts_amd import nifti
    nib = types.ModuleType('nibabel')

    class _Image(object):
        def __init__(self, path):
            self.dataobj = nifti.load(path)[0]
    nib.load = _Image
    tq = types.ModuleType('tqdm')
    tq.tqdm = lambda it=None, **kw: it
    tf = types.ModuleType('tensorflow')
    ar = types.ModuleType('args')
    ar.PreproArgParser = type('PreproArgParser', (object,), {})
    for name, mod in (('nibabel', nib), ('tqdm', tq), ('tensorflow', tf), ('args', ar)):
        assert name not in sys.modules, '%s is already imported' % name
        sys.modules[name] = mod


def record(ref, spec, cases, tmp):
    from bts_amd import nifti
    loc = os.path.join(tmp, spec['name'])
    os.mkdir(loc)
    for k, (mods, lab) in enumerate(cases):
        d = os.path.join(loc, 'case_%02d' % k)
        os.mkdir(d)
        for name, m in zip(spec['modalities'], mods):
            nifti.save(os.path.join(d, 'case_%02d_%s.nii.gz' % (k, name)), m, np.eye(4))
        nifti.save(os.path.join(d, 'case_%02d_%s.nii.gz' % (k, spec['truth'])), lab, np.eye(4))
    visited = glob.glob(os.path.join(loc, '*'))       # the call the reference makes, on the same folder: the same order
    x, y, size = ref.create_dataset([loc], spec['modalities'], spec['truth'])
    order = [int(os.path.basename(p).split('_')[1]) for p in visited]
    n_val = len(x) // 11 if spec['create_val'] else 0
    mean, std = ref.compute_norm(x[n_val:], len(spec['modalities']))
    xn = np.stack([((v - mean) / std).astype(np.float32) for v in x])
    yn = np.stack([np.asarray(v, dtype=np.float32) for v in y])
    raw_x = np.stack([np.stack(cases[k][0], axis=-1) for k in order])
    raw_y = np.stack([cases[k][1] for k in order])
    # the box bounds are not returned by the reference; they follow from where its crop sits in the raw volumes
    full = np.ascontiguousarray(raw_x[0].astype(np.float32))
    h, w, d = size['h'], size['w'], size['d']
    found = [(a, b, c) for a in range(full.shape[0] - h + 1) for b in range(full.shape[1] - w + 1) for c in range(full.shape[2] - d + 1)
             if np.array_equal(full[a:a + h, b:b + w, c:c + d], x[0], equal_nan=True)]
    assert len(found) == 1, found
    lo = found[0]
    s = spec['name']
    return {s + '_raw_x': raw_x, s + '_raw_y': raw_y, s + '_names': np.array([os.path.basename(p) for p in visited]),
            s + '_lo': np.array(lo), s + '_hi': np.array([lo[0] + h, lo[1] + w, lo[2] + d]),
            s + '_size': np.array([h, w, d, size['c']]), s + '_mean': np.asarray(mean, np.float64).reshape(-1),
            s + '_std': np.asarray(std, np.float64).reshape(-1), s + '_x': xn, s + '_y': yn, s + '_n_val': np.array(n_val)}


def main(ref_dir):
    ref_dir = os.path.abspath(ref_dir)
    import bts_amd  # noqa: F401
    install_stubs()
    sys.path.insert(0, ref_dir)
    ref = importlib.import_module('preprocess')
    assert ref.__file__.startswith(ref_dir)
    rng = np.random.default_rng(20181)
    arrays, specs = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for make in (set_a, set_b, set_c, set_d):
            spec, cases = make(rng)
            arrays.update(record(ref, spec, cases, tmp))
            specs.append(dict(spec, set=spec.pop('name')))
            s = specs[-1]['set']
            print('set %s: %d cases, box %s..%s, size %s, mean %s, std %s' % (s, len(cases), arrays[s + '_lo'], arrays[s + '_hi'],
                                                                           arrays[s + '_size'], arrays[s + '_mean'], arrays[s + '_std']))
    arrays['spec'] = np.array(json.dumps(specs))
    np.savez_compressed(OUT, **arrays)
    print('%s: %d bytes' % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) <= LIMIT


if __name__ == '__main__':
    main(sys.argv[1])
