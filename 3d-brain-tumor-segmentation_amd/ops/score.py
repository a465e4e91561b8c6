"""The per-case score on the device (test.py:266-270): the confusion table (csrc/segment.hip), surfaces and exact distances
(csrc/surface.hip), connected components (csrc/components.hip) and the lesion-wise pairing (csrc/lesion.hip)."""
import ctypes

import numpy as np
import torch

from . import _core

u8, i32, i64, f64 = torch.uint8, torch.int32, torch.int64, torch.float64


def label_confusion(truth, pred, n_classes=4, counts=None):
    """truth, pred: dense uint8 label maps of equal size on the GPU -> counts (K,K) int64 on the GPU with
    counts[min(t,K-1), min(p,K-1)] += 1 per voxel.  counts: a zeroed (or partly filled) buffer to add into; a new one otherwise"""
    k = int(n_classes)
    _core.dense(truth, u8, 'label_confusion: truth')
    _core.dense(pred, u8, 'label_confusion: pred')
    if truth.numel() != pred.numel():
        raise ValueError('label_confusion: %d truth and %d predicted voxels' % (truth.numel(), pred.numel()))
    counts = _core.out_or_new(counts, (max(k, 0), max(k, 0)), i64, truth.device, 'label_confusion: counts', numel=k * k, zero=True)
    _core.lib().call('bts_label_confusion', _core._p(truth), _core._p(pred), truth.numel(), k, _core._p(counts), _core._stream())
    return counts


UNCERTAINTY_LEVELS = 101      # levels 0..100 of an uncertainty map


def uncertainty_confusion(truth, pred, unc, class_masks, mask=None, n_classes=4, table=None):
    """truth, pred: dense uint8 label maps of V voxels on the GPU; unc: dense uint8 levels (V, C), channels last (a level above 100 counts
    as 100); class_masks: C host integers, channel c's region = the classes min(label, K-1) whose bit is set in class_masks[c]; mask:
    dense uint8 of V voxels or None, only voxels with mask != 0 count
    -> table (C, 101, 4) int64 on the GPU with table[c, unc[v, c], 2 t + pr] += 1 (cells TN, FP, FN, TP).  table: a zeroed (or partly
    filled) buffer to add into; a new one otherwise   [csrc/ensemble.hip]"""
    k = int(n_classes)
    masks = [int(m) for m in class_masks]
    c = len(masks)
    _core.dense(truth, u8, 'uncertainty_confusion: truth')
    _core.dense(pred, u8, 'uncertainty_confusion: pred', numel=truth.numel())
    _core.dense(unc, u8, 'uncertainty_confusion: unc', numel=truth.numel() * c)
    if mask is not None:
        _core.dense(mask, u8, 'uncertainty_confusion: mask', numel=truth.numel())
    if any(m < 0 or m >> max(k, 0) for m in masks):
        raise ValueError('uncertainty_confusion: class masks must lie in [0, 2^%d), got %r' % (k, masks))
    table = _core.out_or_new(table, (c, UNCERTAINTY_LEVELS, 4), i64, truth.device, 'uncertainty_confusion: table',
                             numel=c * UNCERTAINTY_LEVELS * 4, zero=True)
    _core.lib().call('bts_uncertainty_confusion', _core._p(truth), _core._p(pred), _core._p(unc), _core._p(mask), truth.numel(), c, k,
                     _core.carray(ctypes.c_uint, masks), _core._p(table), _core._stream())
    return table


def region_surface(lab, n_classes=4, class_mask=0b1110, out=None, count=None):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask
    -> (surf uint8 (D,H,W): 1 on the region's surface voxels (a face neighbour outside the region or the volume), 0 elsewhere;
    count: one int64 on the GPU, += their number).  out: a dense uint8 tensor of lab's size to write into; count: a zeroed (or partly
    filled) int64 element to add into; new ones otherwise"""
    _core.dense(lab, u8, 'region_surface: lab', rank=3)
    out = _core.out_or_new(out, lab.shape, u8, lab.device, 'region_surface: out', numel=lab.numel())
    count = _core.out_or_new(count, (1,), i64, lab.device, 'region_surface: count', numel=1, zero=True)
    d, h, w = lab.shape
    _core.lib().call('bts_region_surface', _core._p(lab), _core._p(out), _core._p(count), d, h, w, int(n_classes), int(class_mask), _core._stream())
    return out, count


def edt3d_sq(feat, spacing=(1.0, 1.0, 1.0), out=None):
    """feat: dense uint8 (D,H,W) on the GPU, spacing (sd,sh,sw) in mm -> float64 (D,H,W): the squared distance in mm^2 to the nearest
    voxel with feat != 0 (+inf when there is none), exact.  out: a dense float64 tensor of feat's size to write into"""
    _core.dense(feat, u8, 'edt3d_sq: feat', rank=3)
    sd, sh, sw = (float(s) for s in spacing)
    out = _core.out_or_new(out, feat.shape, f64, feat.device, 'edt3d_sq: out', numel=feat.numel())
    d, h, w = feat.shape
    _core.lib().call('bts_edt3d_sq', _core._p(feat), _core._p(out), d, h, w, sd, sh, sw, _core._stream())
    return out


def masked_select(v, mask, ranks, out=None):
    """v: dense NON-NEGATIVE float64, mask: dense uint8 of the same size, both on the GPU; ranks: up to 8 host integers
    -> float64 (len(ranks),) on the GPU: the ranks[i]-th smallest (0-based) of v[mask != 0], the bits np.sort gives; nan where
    ranks[i] is not below the number of selected values.  out: a dense float64 tensor of len(ranks) values to write into"""
    _core.dense(v, f64, 'masked_select: v')
    _core.dense(mask, u8, 'masked_select: mask')
    if v.numel() != mask.numel():
        raise ValueError('masked_select: %d values and %d mask bytes' % (v.numel(), mask.numel()))
    ranks = [int(r) for r in ranks]
    nr = len(ranks)
    out = _core.out_or_new(out, (nr,), f64, v.device, 'masked_select: out', numel=nr)
    if nr == 0:
        return out
    ws, nb = _core.scratch('bts_masked_select_workspace', v.device, nr)
    _core.lib().call('bts_masked_select', _core._p(v), _core._p(mask), v.numel(), _core.carray(ctypes.c_long, ranks), nr, _core._p(out), _core._p(ws),
                     _core._stream())
    if v.numel() == 0:
        out.fill_(float('nan'))                                  # nothing is selected, and the call launches nothing for no values
    return out


def components3d(lab, class_mask, K=4, connectivity=26, out=None):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask;
    connectivity 6 | 18 | 26 (scipy's generate_binary_structure(3, 1 | 2 | 3))
    -> comp int32 (D,H,W): 0 outside the region, 1 + the smallest linear index of the voxel's component inside (the same bytes in
    every run; comp[v] == v + 1 marks a root).  out: a dense int32 tensor of lab's size to write into"""
    _core.dense(lab, u8, 'components3d: lab', rank=3)
    out = _core.out_or_new(out, lab.shape, i32, lab.device, 'components3d: out', numel=lab.numel())
    d, h, w = lab.shape
    _core.lib().call('bts_components3d', _core._p(lab), _core._p(out), d, h, w, int(K), int(class_mask), int(connectivity), _core._stream())
    return out


def component_sizes(comp, out=None, count=None):
    """comp: the int32 map of components3d -> (size int32 (comp.numel(),): size[r] = voxels of the component whose root is r, 0
    elsewhere; count: one int64 on the GPU, += the number of components).  out: a dense int32 tensor of that size to write into (the
    call zeroes it); count: a zeroed (or partly filled) int64 element to add into; new ones otherwise"""
    _core.dense(comp, i32, 'component_sizes: comp')
    n = comp.numel()
    out = _core.out_or_new(out, (n,), i32, comp.device, 'component_sizes: out', numel=n)
    count = _core.out_or_new(count, (1,), i64, comp.device, 'component_sizes: count', numel=1, zero=True)
    _core.lib().call('bts_component_sizes', _core._p(comp), n, _core._p(out), _core._p(count), _core._stream())
    return out, count


def component_largest(size, out=None):
    """size: the int32 sizes of component_sizes -> key: one int64 on the GPU holding (size << 32) | (0xFFFFFFFF - root) of the largest
    component, the smallest root among equal sizes; 0 when there is none.  out: an int64 element to write into"""
    _core.dense(size, i32, 'component_largest: size')
    out = _core.out_or_new(out, (1,), i64, size.device, 'component_largest: out', numel=1, zero=True)
    _core.lib().call('bts_component_largest', _core._p(size), size.numel(), _core._p(out), _core._stream())
    return out


def components_apply(lab, comp, size, key=None, min_voxels=0, largest_only=False, fill=0, removed=None):
    """in place on the dense uint8 map `lab`: every voxel of a component (comp, size as above) that fails `size >= min_voxels and (not
    largest_only or it is the component of key)` becomes `fill`; no other voxel is written
    -> removed: two int64 on the GPU, += (voxels, components) removed.  removed: a zeroed (or partly filled) pair to add into"""
    _core.dense(lab, u8, 'components_apply: lab')
    _core.dense(comp, i32, 'components_apply: comp')
    _core.dense(size, i32, 'components_apply: size')
    n = lab.numel()
    if comp.numel() != n or size.numel() != n:
        raise ValueError('components_apply: lab holds %d voxels, comp %d, size %d' % (n, comp.numel(), size.numel()))
    if largest_only and key is None:
        raise ValueError('components_apply: largest_only needs the key of component_largest')
    if key is not None:
        _core.dense(key, i64, 'components_apply: key', numel=1)
    removed = _core.out_or_new(removed, (2,), i64, lab.device, 'components_apply: removed', numel=2, zero=True)
    _core.lib().call('bts_components_apply', _core._p(lab), _core._p(comp), _core._p(size), _core._p(key), n, int(min_voxels),
                     1 if largest_only else 0, int(fill), _core._p(removed[0:1]), _core._p(removed[1:2]), _core._stream())
    return removed


def region_relabel(lab, class_mask, fill, limit, K=4, changed=None):
    """in place on the dense uint8 map `lab`: when the region (K, class_mask as in components3d) holds between 1 and limit - 1 voxels,
    each becomes `fill` -> changed: one int64 on the GPU, += their number.  The count is taken on the device (label_confusion of the map
    with itself) and the decision is made there.  changed: a zeroed (or partly filled) int64 element to add into"""
    _core.dense(lab, u8, 'region_relabel: lab')
    changed = _core.out_or_new(changed, (1,), i64, lab.device, 'region_relabel: changed', numel=1, zero=True)
    flat = lab.view(-1)
    conf = label_confusion(flat, flat, K)
    _core.lib().call('bts_region_relabel', _core._p(lab), lab.numel(), int(K), int(class_mask), int(fill), _core._p(conf), int(limit),
                     _core._p(changed), _core._stream())
    return changed


def dilate3d(lab, class_mask, K=4, connectivity=18, iterations=1, out=None, fuse=0):
    """lab: dense uint8 label map (D,H,W) on the GPU; the region is the set of classes min(label, K-1) whose bit is set in class_mask;
    connectivity 6 | 18 | 26 (scipy's generate_binary_structure(3, 1 | 2 | 3)); iterations >= 0
    -> uint8 (D,H,W): 1 where scipy.ndimage.binary_dilation(region, structure, iterations, border_value=0) is set, 0 elsewhere (the
    region itself for 0 iterations).  out: a dense uint8 tensor of lab's size to write into, not lab itself; fuse: iterations run per
    pass over the volume, 1..6 (0: the library's default)"""
    _core.dense(lab, u8, 'dilate3d: lab', rank=3)
    given, out = out is not None, _core.out_or_new(out, lab.shape, u8, lab.device, 'dilate3d: out', numel=lab.numel())
    if given and out.data_ptr() == lab.data_ptr():
        raise ValueError('dilate3d: out must not be lab (a tile reads its neighbours\' voxels)')
    d, h, w = lab.shape
    ws, nb = _core.scratch('bts_dilate3d_workspace', lab.device, d, h, w, int(iterations), int(fuse), optional=True)
    _core.lib().call('bts_dilate3d', _core._p(lab), _core._p(out), d, h, w, int(K), int(class_mask), int(connectivity), int(iterations), int(fuse),
                     _core._p(ws), _core._stream())
    return out


def lesion_pairs_capacity(n_td, n_pred):
    """slots of the pairing table for n_td dilated lesions and n_pred predicted components: a power of two, at least four times their
    sum (a component usually meets one lesion and a lesion a few components; a table that is too small is grown, not an error)"""
    need = 4 * (max(int(n_td), 0) + max(int(n_pred), 0))
    cap = 256
    while cap < need:
        cap *= 2
    return cap


def lesion_pairs(td_comp, truth, pred_comp, class_mask, K=4, counts=None, capacity=None, lesion_vox=None):
    """td_comp, pred_comp: the int32 maps components3d gives for the dilated truth and for the prediction; truth: the dense uint8 truth
    map of the same size, its region K / class_mask
    -> (rows: int64 numpy (pairs, 4), one row (lesion_root, pred_root, reach, overlap) per pair of a dilated component and a predicted
    component that share a voxel -- reach: the voxels they share, overlap: those of them that are truth -- in lexicographic order;
    lesion_vox: int32 (n,) on the GPU, lesion_vox[r] = the truth voxels inside the dilated component of root r, 0 elsewhere).
    counts: (dilated components, predicted components) as host integers, from which the table's capacity is derived; counted here (one
    more host read) when neither they nor `capacity` are given.  A table that proves too small is grown and the pass run again: the rows
    do not depend on the capacity.  One host read per pass.  lesion_vox: a dense int32 tensor of n values to write into"""
    _core.dense(td_comp, i32, 'lesion_pairs: td_comp')
    _core.dense(pred_comp, i32, 'lesion_pairs: pred_comp')
    _core.dense(truth, u8, 'lesion_pairs: truth')
    n = td_comp.numel()
    if pred_comp.numel() != n or truth.numel() != n:
        raise ValueError('lesion_pairs: td_comp holds %d voxels, truth %d, pred_comp %d' % (n, truth.numel(), pred_comp.numel()))
    lesion_vox = _core.out_or_new(lesion_vox, (n,), i32, td_comp.device, 'lesion_pairs: lesion_vox', numel=n)
    if capacity is None:
        if counts is None:
            both = torch.zeros(2, dtype=i64, device=td_comp.device)
            scratch = torch.empty(n, dtype=i32, device=td_comp.device)
            component_sizes(td_comp, out=scratch, count=both[0:1])
            component_sizes(pred_comp, out=scratch, count=both[1:2])
            counts = both.cpu().tolist()
        capacity = lesion_pairs_capacity(*counts)
    capacity = int(capacity)
    if capacity < 1:
        raise ValueError('lesion_pairs: the capacity must be positive, got %r' % (capacity,))
    while True:
        _core.lib().query('bts_lesion_pairs_table_bytes', capacity)
        buf = torch.empty(2 + 2 * capacity, dtype=i64, device=td_comp.device)               # status, keys, (reach, overlap) pairs
        _core.lib().call('bts_lesion_pairs', _core._p(td_comp), _core._p(truth), _core._p(pred_comp), n, int(K), int(class_mask),
                         _core._p(lesion_vox), _core._p(buf[2:]), capacity, _core._p(buf[0:2]), _core._stream())
        host = buf.cpu().numpy()                                                            # the one read of this pass
        stored, refused = int(host[0]), int(host[1])
        if refused == 0:
            break
        capacity = lesion_pairs_capacity(stored + refused, 0)                               # enough by construction: one rerun
    keys = host[2:2 + capacity]
    cnt = host[2 + capacity:].view(np.int32).reshape(capacity, 2)
    used = np.nonzero(keys)[0]
    rows = np.empty((len(used), 4), dtype=np.int64)
    rows[:, 0] = (keys[used] >> 32) - 1
    rows[:, 1] = (keys[used] & 0xFFFFFFFF) - 1
    rows[:, 2:] = cnt[used]
    if len(used) != stored:
        raise RuntimeError('lesion_pairs: the table holds %d pairs, its status word says %d' % (len(used), stored))
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))], lesion_vox


def _roots(roots, name, device):
    """-> (dense int32 tensor on the GPU or None, length); a host sequence is checked to ascend and uploaded"""
    if isinstance(roots, torch.Tensor):
        _core.dense(roots, i32, name)
        return (roots if roots.numel() else None), roots.numel()
    r = np.asarray(roots, dtype=np.int64).reshape(-1)
    if len(r) and (r[0] < 0 or r[-1] >= 2 ** 31 - 1 or (np.diff(r) <= 0).any()):
        raise ValueError('%s must ascend strictly inside [0, 2^31 - 1)' % name)
    return (torch.from_numpy(r.astype(np.int32)).to(device) if len(r) else None), len(r)


def component_boxes(comp, roots, out=None):
    """comp: the int32 map (D,H,W) of components3d; roots: ASCENDING roots, a dense int32 tensor on the GPU or a host sequence
    -> int32 (len(roots), 6) on the GPU: the half-open bounding box (d0,h0,w0,d1,h1,w1) of each root's component.  out: a dense int32
    tensor of that size to write into"""
    _core.dense(comp, i32, 'component_boxes: comp', rank=3)
    rt, m = _roots(roots, 'component_boxes: roots', comp.device)
    out = _core.out_or_new(out, (m, 6), i32, comp.device, 'component_boxes: out', numel=6 * m)
    d, h, w = comp.shape
    _core.lib().call('bts_component_boxes', _core._p(comp), d, h, w, _core._p(rt), m, _core._p(out), _core._stream())
    return out


def lesion_crop(td_comp, truth, pred_comp, class_mask, box, td_root, roots, K=4, out=None):
    """td_comp, truth, pred_comp as in lesion_pairs, shape (D,H,W); box: host (d0,h0,w0,d1,h1,w1), half-open and inside the volume;
    td_root: the root of one dilated component; roots: ASCENDING roots of predicted components (tensor or host sequence)
    -> (g, m): dense uint8 maps of the box's extent; g = 1 where the voxel is truth inside that dilated component, m = 1 where the
    voxel's predicted component is one of `roots`.  out: a pair of dense uint8 tensors of the box's size to write into"""
    _core.dense(td_comp, i32, 'lesion_crop: td_comp', rank=3)
    _core.dense(pred_comp, i32, 'lesion_crop: pred_comp', rank=3)
    _core.dense(truth, u8, 'lesion_crop: truth', rank=3)
    if tuple(td_comp.shape) != tuple(truth.shape) or tuple(pred_comp.shape) != tuple(truth.shape):
        raise ValueError('lesion_crop: the three maps differ in shape: %s, %s, %s' %
                         (tuple(td_comp.shape), tuple(truth.shape), tuple(pred_comp.shape)))
    d, h, w = truth.shape
    box = tuple(int(v) for v in box)
    if len(box) != 6 or min(box[:3]) < 0 or any(b1 <= b0 for b0, b1 in zip(box[:3], box[3:])) or any(b1 > s for b1, s in zip(box[3:], (d, h, w))):
        raise ValueError('lesion_crop: box must be a non-empty half-open (d0,h0,w0,d1,h1,w1) inside %s, got %r' % ((d, h, w), box))
    ext = tuple(b1 - b0 for b0, b1 in zip(box[:3], box[3:]))
    rt, m = _roots(roots, 'lesion_crop: roots', truth.device)
    g, pm = (None, None) if out is None else out
    g = _core.out_or_new(g, ext, u8, truth.device, 'lesion_crop: out g', numel=ext[0] * ext[1] * ext[2])
    pm = _core.out_or_new(pm, ext, u8, truth.device, 'lesion_crop: out m', numel=ext[0] * ext[1] * ext[2])
    _core.lib().call('bts_lesion_crop', _core._p(td_comp), _core._p(truth), _core._p(pred_comp), d, h, w, int(K), int(class_mask), *box, int(td_root),
                     _core._p(rt), m, _core._p(g), _core._p(pm), _core._stream())
    return (g, pm) if out is None else out
