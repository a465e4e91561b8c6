"""Pure-NumPy restatement of csrc/components.hip and of infer.remove_components / postprocess_labels (no SciPy: the GPU tests use it).

Labelling: every voxel of the region starts as its own linear index + 1 and takes the minimum over its neighbourhood (6 | 18 | 26
neighbours inside the region) until nothing changes.  A label always names a voxel of the same component, so between two sweeps the
voxel a label named also takes what the sweep found (hooking), and every voxel the label of the voxel its label names until that is
stable too (pointer jumping): the fixed point is the same, the smallest index + 1 of the component, and a serpentine component of 10^5
voxels takes a few sweeps instead of 10^5."""
import numpy as np

MAXD = {6: 1, 18: 2, 26: 3}


def region_of(lab, class_mask, K=4):
    """bool map: bit min(label, K-1) of class_mask is set"""
    cls = np.minimum(np.asarray(lab).astype(np.int64), K - 1)
    return ((int(class_mask) >> cls) & 1).astype(bool)


def offsets(connectivity):
    m = MAXD[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < abs(dz) + abs(dy) + abs(dx) <= m]


def label_region(region, connectivity):
    """bool (D,H,W) -> int32 (D,H,W): 0 outside, 1 + the smallest linear index of the component inside"""
    region = np.asarray(region, dtype=bool)
    d, h, w = region.shape
    n = region.size
    big = n + 1
    cur = np.where(region, np.arange(1, n + 1, dtype=np.int64).reshape(region.shape), 0)
    offs = offsets(connectivity)
    while True:
        padded = np.full((d + 2, h + 2, w + 2), big, dtype=np.int64)
        padded[1:-1, 1:-1, 1:-1] = np.where(region, cur, big)
        new = padded[1:-1, 1:-1, 1:-1].copy()
        for dz, dy, dx in offs:
            np.minimum(new, padded[1 + dz:1 + dz + d, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w], out=new)
        flat = np.where(region, new, 0).reshape(-1)
        inside = np.flatnonzero(flat)
        np.minimum.at(flat, cur.reshape(-1)[inside] - 1, flat[inside])   # ... and hands what it found to the voxel its label named
        while True:                                   # the label of the voxel my label names
            jumped = np.where(flat > 0, flat[np.maximum(flat - 1, 0)], 0)
            if np.array_equal(jumped, flat):
                break
            flat = jumped
        if np.array_equal(flat, cur.reshape(-1)):
            return flat.reshape(region.shape).astype(np.int32)
        cur = flat.reshape(region.shape)


def components3d(lab, class_mask, K=4, connectivity=26):
    return label_region(region_of(lab, class_mask, K), connectivity)


def sizes(comp):
    """-> (size int32 (n,): voxels per root, number of components)"""
    c = np.asarray(comp).reshape(-1)
    size = np.bincount(c[c > 0] - 1, minlength=c.size).astype(np.int32)
    return size, int((size > 0).sum())


def largest_key(size):
    """(size << 32) | (0xFFFFFFFF - root) of the largest component, the smallest root among equals; 0 when there is none"""
    size = np.asarray(size)
    if not (size > 0).any():
        return 0
    root = int(np.argmax(size))                       # argmax returns the FIRST maximum: the smallest root
    return (int(size[root]) << 32) | (0xFFFFFFFF - root)


def key_root(key):
    return 0xFFFFFFFF - (int(key) & 0xFFFFFFFF)


def apply(lab, comp, size, min_voxels=0, largest_only=False, fill=0):
    """-> (new label map, removed voxels, removed components); only voxels of failing components change"""
    lab = np.array(lab, copy=True)
    comp = np.asarray(comp)
    flat, c = lab.reshape(-1), comp.reshape(-1)
    root = np.maximum(c.astype(np.int64) - 1, 0)
    keep = np.asarray(size)[root] >= min_voxels
    if largest_only:
        keep &= root == key_root(largest_key(size))
    fail = (c > 0) & ~keep
    flat[fail] = fill
    is_root = c == np.arange(1, c.size + 1)
    return lab, int(fail.sum()), int((fail & is_root).sum())


def remove_components(lab, class_mask, K=4, connectivity=26, min_voxels=0, largest_only=False, fill=0):
    """-> (new label map, counts as infer.remove_components returns them)"""
    comp = components3d(lab, class_mask, K, connectivity)
    size, found = sizes(comp)
    out, vox, gone = apply(lab, comp, size, min_voxels, largest_only, fill)
    return out, {'components': found, 'removed_components': gone, 'removed_voxels': vox}


def postprocess_labels(lab, min_component_voxels=0, et_min_voxels=0, connectivity=26):
    """BraTS label maps (0, 1, 2, 4) -> (new label map, counts as infer.postprocess_labels returns them)"""
    out = np.array(lab, copy=True)
    counts = {'components': 0, 'removed_components': 0, 'removed_voxels': 0, 'et_relabelled': 0}
    if min_component_voxels > 0:
        out, c = remove_components(out, 14, 4, connectivity, min_voxels=min_component_voxels)
        counts.update(c)
    if et_min_voxels > 0:
        et = out >= 3
        if 0 < int(et.sum()) < et_min_voxels:
            counts['et_relabelled'] = int(et.sum())
            out[et] = 1
    return out, counts


# ---- inputs shared by the host and the device tests ------------------------------------------------------------------------------------
def random_labels(shape, density, seed):
    """labels from {1, 2, 4, 255} on a fraction `density` of the voxels, 0 elsewhere"""
    rng = np.random.default_rng(seed)
    vals = np.array([1, 2, 4, 255], dtype=np.uint8)
    lab = vals[rng.integers(0, 4, size=shape)]
    lab[rng.random(shape) >= density] = 0
    return lab


def checkerboard(shape):
    d, h, w = np.indices(shape)
    return (((d + h + w) & 1) == 0).astype(np.uint8)


def serpentine(shape):
    """one component through the volume whatever the connectivity: every other row of every other plane is full, joined to the next at
    alternating ends (W, then H), and the planes by one voxel at alternating ends: parent chains as deep as they get"""
    d, h, w = shape
    lab = np.zeros(shape, dtype=np.uint8)
    lab[::2, ::2, :] = 1
    for j, y in enumerate(range(1, h - 1, 2)):                       # between rows y - 1 and y + 1 (both exist)
        lab[::2, y, (w - 1) if j % 2 == 0 else 0] = 1
    last = len(range(0, h, 2)) - 1                                   # the path of a plane ends in row 2 * last, at the end that row's turn left
    end = (w - 1) if last % 2 == 0 else 0
    for i, z in enumerate(range(1, d - 1, 2)):                       # between planes z - 1 and z + 1: at the path's end, then at its start
        lab[z, 2 * last if i % 2 == 0 else 0, end if i % 2 == 0 else 0] = 1
    return lab
