"""SciPy / NumPy restatement of the lesion-wise score (csrc/lesion.hip, bts_amd.infer.lesionwise_scores), for
tests/test_lesion_host.py and tests/test_lesion_gpu.py (helper module, not collected).

  dilate            scipy.ndimage.binary_dilation with generate_binary_structure(3, 1 | 2 | 3), border_value = 0
  components        scipy.ndimage.label, renamed to 1 + the smallest linear index of each component (what bts_components3d writes)
  pairs             the rows (lesion_root, pred_root, reach, overlap) and the truth voxels per dilated component
  boxes, crop       half-open bounding boxes of components, and the two 0/1 maps of a box
  lesionwise_region the seven steps of the definition for one region, on whole volumes, with tests/surface_ref.py's HD95
  lesionwise_scores the same over the regions, the dict bts_amd.infer.lesionwise_scores returns
"""
import math

import numpy as np
from scipy import ndimage as ndi

import surface_ref as S

BRATS_REGIONS = (('wt', (1, 2, 3)), ('tc', (1, 3)), ('et', (3,)))
RANK = {6: 1, 18: 2, 26: 3}
KNOWN_SHAPE = (12, 16, 40)
ZERO = {'lesions': 0, 'false_negatives': 0, 'false_positives': 0, 'ignored': 0}


def region(lab, class_mask, k=4):
    return S.region(lab, k, class_mask)


def dilate(mask, connectivity=18, iterations=3):
    mask = np.asarray(mask, dtype=bool)
    if iterations == 0:
        return mask.copy()
    return ndi.binary_dilation(mask, ndi.generate_binary_structure(3, RANK[connectivity]), iterations, border_value=0)


def components(mask, connectivity=26):
    """-> int32 map: 0 outside the mask, 1 + the smallest linear index of the voxel's component inside"""
    mask = np.asarray(mask, dtype=bool)
    labels, n = ndi.label(mask, ndi.generate_binary_structure(3, RANK[connectivity]))
    if n == 0:
        return np.zeros(mask.shape, dtype=np.int32)
    first = ndi.minimum(np.arange(mask.size).reshape(mask.shape), labels, np.arange(1, n + 1)) + 1
    return np.concatenate([[0], first])[labels].astype(np.int32)


def roots_of(comp):
    return np.unique(comp[comp > 0]).astype(np.int64) - 1


def pairs(td_comp, truth_region, pred_comp):
    """-> (rows int64 (pairs, 4) in lexicographic order, lesion_vox int32 (n,))"""
    a, b, t = td_comp.reshape(-1).astype(np.int64), pred_comp.reshape(-1).astype(np.int64), np.asarray(truth_region).reshape(-1)
    lesion_vox = np.bincount(a[t & (a > 0)] - 1, minlength=a.size).astype(np.int32)
    both = (a > 0) & (b > 0)
    key = (a[both] - 1) * a.size + (b[both] - 1)
    uniq, inv = np.unique(key, return_inverse=True)
    rows = np.zeros((len(uniq), 4), dtype=np.int64)
    rows[:, 0], rows[:, 1] = uniq // a.size, uniq % a.size
    rows[:, 2] = np.bincount(inv, minlength=len(uniq))
    rows[:, 3] = np.bincount(inv, weights=t[both].astype(np.float64), minlength=len(uniq)).astype(np.int64)
    return rows, lesion_vox


def boxes(comp, roots):
    out = np.zeros((len(roots), 6), dtype=np.int32)
    for i, r in enumerate(roots):
        idx = np.argwhere(comp == r + 1)
        out[i] = np.concatenate([idx.min(axis=0), idx.max(axis=0) + 1]) if len(idx) else (2 ** 31 - 1,) * 3 + (0,) * 3
    return out


def crop(td_comp, truth_region, pred_comp, box, td_root, roots):
    sl = tuple(slice(box[i], box[i + 3]) for i in range(3))
    g = (td_comp[sl] == td_root + 1) & np.asarray(truth_region)[sl]
    m = np.isin(pred_comp[sl], np.asarray(roots, dtype=np.int64) + 1) & (pred_comp[sl] > 0)
    return g.astype(np.uint8), m.astype(np.uint8)


def lesionwise_region(t_mask, p_mask, spacing, dilation=3, dilation_connectivity=18, connectivity=26, min_lesion_voxels=50,
                      penalty_mm=374.0, percentile=95.0, hd95=None):
    """-> (lw_dice, lw_hd95, counts, lesions) of two boolean maps, by the seven steps.  hd95: a function (L, M, spacing, percentile)
    -> mm in place of tests/surface_ref.py's (scripts/lesionwise_measure.py times a full-size case with a faster one)"""
    t_mask, p_mask = np.asarray(t_mask, dtype=bool), np.asarray(p_mask, dtype=bool)
    counts = {'lesions': 0, 'false_negatives': 0, 'false_positives': 0, 'ignored': 0}
    if not t_mask.any() and not p_mask.any():                                                   # 1
        return 1.0, 0.0, counts, []
    structure = ndi.generate_binary_structure(3, RANK[connectivity])
    td_lab, n_les = ndi.label(dilate(t_mask, dilation_connectivity, dilation), structure)       # 2
    p_lab, n_comp = ndi.label(p_mask, structure)                                                # 3
    matched_any = set()
    lesions = []
    for i in range(1, n_les + 1):                                                               # scipy's label order
        halo = td_lab == i
        les = t_mask & halo
        comps = [int(c) for c in np.unique(p_lab[halo]) if c > 0]                               # 4
        matched_any.update(comps)
        if int(les.sum()) < min_lesion_voxels:                                                  # 5
            counts['ignored'] += 1
            continue
        m = np.isin(p_lab, comps) & p_mask
        row = {'voxels': int(les.sum()), 'matched_components': len(comps), 'matched_voxels': int(m.sum()),
               'overlap': int((les & m).sum()), 'dice': 0.0, 'hd95': float(penalty_mm)}
        if comps:                                                                               # 6
            row['dice'] = 2.0 * row['overlap'] / (row['voxels'] + row['matched_voxels'])
            row['hd95'] = hd95(les, m, spacing, percentile) if hd95 else S.hd95(les, m, spacing, percentile)['hd95']
        else:
            counts['false_negatives'] += 1
        lesions.append(row)
    counts['lesions'] = len(lesions)
    counts['false_positives'] = n_comp - len(matched_any)
    n = len(lesions) + counts['false_positives']                                                # 7
    if n == 0:
        return float('nan'), float('nan'), counts, lesions
    sum_dice = sum_hd = 0.0
    for row in lesions:
        sum_dice += row['dice']
        sum_hd += row['hd95']
    return sum_dice / n, (sum_hd + float(penalty_mm) * counts['false_positives']) / n, counts, lesions


def lesionwise_scores(truth, pred, spacing, n_classes=4, regions=None, **kw):
    k = int(n_classes)
    if regions is None:
        regions = BRATS_REGIONS if k == 4 else tuple(('class_%d' % c, (c,)) for c in range(1, k))
    out = {}
    for name, sel in regions:
        cm = sum(1 << c for c in set(sel))
        dice, hd, counts, lesions = lesionwise_region(region(truth, cm, k), region(pred, cm, k), spacing, **kw)
        out['lw_dice_' + name], out['lw_hd95_' + name], out['lw_counts_' + name], out['lw_lesions_' + name] = dice, hd, counts, lesions
    return out


def block(lab, lo, hi, value):
    lab[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = value


def multi_lesion_pair(shape=(24, 40, 72)):
    """a truth / prediction pair of labels {0,1,2,4} in which the whole tumour holds: two pieces 2 voxels apart (one lesion at dilation
    3) predicted by one component with a hole, a lesion below 50 voxels with a component of its own, a lesion nobody predicted, a
    predicted component far from every lesion, a component that reaches a lesion's halo but none of its voxels, one component that
    spans two lesions, and sets on every face of the volume; tc and et are sub-sets with fewer of these"""
    d, h, w = shape
    t, p = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    block(t, (0, 0, 0), (5, 6, 7), 2)                  # A: two pieces, the second starts 2 empty voxels after the first
    block(t, (1, 1, 1), (4, 5, 5), 4)
    block(t, (0, 0, 9), (5, 6, 14), 1)
    block(p, (0, 0, 2), (4, 6, 12), 2)                 # ... one component over both, shifted
    block(p, (1, 2, 3), (3, 4, 5), 4)
    block(t, (10, 20, 30), (13, 23, 33), 1)            # B: 27 voxels, ignored at 50
    block(p, (10, 20, 31), (13, 24, 35), 1)            # ... its component is no false positive
    block(t, (18, 30, 0), (24, 36, 5), 2)              # C: missed
    block(t, (19, 31, 1), (23, 35, 4), 4)
    block(p, (0, 33, 60), (4, 40, 72), 4)              # D: a false positive in a corner (enhancing: in every region)
    block(t, (8, 0, 50), (16, 6, 58), 1)              # E: matched through the halo only
    block(p, (8, 0, 60), (16, 6, 64), 2)
    block(t, (16, 14, 56), (24, 22, 62), 4)            # F and G: 7 voxels apart, one predicted component over both
    block(t, (16, 14, 69), (24, 22, 72), 4)
    block(p, (18, 16, 58), (22, 20, 72), 4)
    return t, p


def known_cases():
    """name -> (truth mask, predicted mask, keyword arguments, expected (dice, hd95, counts)); for tests/test_lesion_host.py (the restatement) and
    tests/test_lesion_gpu.py (the device).
    A cube of 4 x 4 x 4 = 64 voxels is a lesion at the default 50; one of 3 x 3 x 3 = 27 is ignored."""
    def empty():
        return np.zeros(KNOWN_SHAPE, bool)

    def cube(m, lo, side=4):
        m[lo[0]:lo[0] + side, lo[1]:lo[1] + side, lo[2]:lo[2] + side] = True
        return m

    out = {}
    out['both_empty'] = (empty(), empty(), {}, (1.0, 0.0, ZERO))
    out['truth_empty_two_components'] = (empty(), cube(cube(empty(), (0, 0, 0)), (6, 8, 30)), {},
                                         (0.0, 374.0, dict(ZERO, false_positives=2)))
    out['one_lesion_exact'] = (cube(empty(), (2, 3, 5)), cube(empty(), (2, 3, 5)), {}, (1.0, 0.0, dict(ZERO, lesions=1)))
    two = cube(cube(empty(), (2, 3, 5)), (2, 3, 11))                     # w 5..8 and 11..14: two empty voxels between them
    out['two_pieces_one_lesion'] = (two, two.copy(), {}, (1.0, 0.0, dict(ZERO, lesions=1)))
    out['two_pieces_two_lesions'] = (two, two.copy(), {'dilation': 0}, (1.0, 0.0, dict(ZERO, lesions=2)))
    # the component starts 2 voxels after the lesion: inside its halo of 3, on none of its voxels
    out['halo_only'] = (cube(empty(), (2, 3, 5)), cube(empty(), (2, 3, 11)), {}, (0.0, None, dict(ZERO, lesions=1)))
    # two lesions 8 voxels apart, one bar through both: it counts for each
    far = cube(cube(empty(), (2, 3, 5)), (2, 3, 17))
    bar = empty()
    bar[3:5, 4:6, 5:21] = True
    d = 2.0 * 16 / (64 + 64)
    out['one_component_two_lesions'] = (far, bar, {}, (d, None, dict(ZERO, lesions=2)))
    out['all_ignored_nothing_predicted'] = (cube(empty(), (2, 3, 5), 3), empty(), {}, (math.nan, math.nan, dict(ZERO, ignored=1)))
    out['component_on_an_ignored_lesion'] = (cube(empty(), (2, 3, 5), 3), cube(empty(), (2, 3, 6), 3), {},
                                             (math.nan, math.nan, dict(ZERO, ignored=1)))
    return out
