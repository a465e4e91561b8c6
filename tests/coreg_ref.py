"""float64 / integer restatement of the co-registration passes (csrc/coreg.hip, bts_amd.coreg), shared by tests/test_coreg_host.py,
tests/test_coreg_gpu.py and scripts/bench_coreg.py: the quantiser, the partial-volume joint histogram (vectorised, one np.bincount per
corner), `ties`, an analytic two-contrast head phantom and the cases of the kernel tests.  Nothing here imports bts_amd: `joint_hist_pv` has the
arguments and the result of `bts_amd.ops.joint_hist_pv` and is what the tests hand to `coreg.coregister(evaluate=...)`.

The rule (Q = 32; include/bts_hip.h states it for bts_joint_hist_pv): lattice point f = o + l * s of the fixed grid, a = qf[f];
c_j = ((m[j][0] f0 + m[j][1] f1) + m[j][2] f2) + m[j][3] in float64, operation by operation; counted only if 0 <= c_j <= N_j - 1 on all
axes; i_j = floor(c_j), r_j = int(floor((c_j - i_j) Q + 0.5)); corner d in {0,1}^3 reads b = qm[min(i_j + d_j, N_j - 1)] and adds
prod_j (d_j ? r_j : Q - r_j) to hist[a][b]."""
import numpy as np

Q = 32


def quantize(x, lo, hi, bins):
    """clamp(floor((double(x) - lo) * bins / (hi - lo)), 0, bins - 1) in float64 -> uint8; a NaN gives 0"""
    with np.errstate(invalid='ignore'):
        t = np.floor((np.asarray(x, dtype=np.float32).astype(np.float64) - float(lo)) * float(bins) / (float(hi) - float(lo)))
        return np.where(t >= 0.0, np.minimum(t, bins - 1.0), 0.0).astype(np.uint8)


def _as_numpy(t):
    return t.cpu().numpy() if hasattr(t, 'cpu') else np.asarray(t)


def coordinates(m, origin, stride, counts):
    """the float64 moving-voxel coordinates of every lattice point, in the rule's order of operations -> (f (3, n), c (3, n))"""
    m = np.asarray(m, dtype=np.float64)
    grids = np.meshgrid(*[origin[a] + stride[a] * np.arange(counts[a]) for a in range(3)], indexing='ij')
    f = np.stack([g.reshape(-1) for g in grids])
    ff = f.astype(np.float64)
    c = np.stack([((m[j, 0] * ff[0] + m[j, 1] * ff[1]) + m[j, 2] * ff[2]) + m[j, 3] for j in range(3)])
    return f, c


def joint_hist_one(qf, qm, origin, stride, counts, m, bins):
    qf, qm = np.asarray(qf), np.asarray(qm)
    f, c = coordinates(m, origin, stride, counts)
    hi = np.array(qm.shape, dtype=np.float64).reshape(3, 1) - 1.0
    with np.errstate(invalid='ignore'):
        inside = np.all((c >= 0.0) & (c <= hi), axis=0)
    f, c = f[:, inside], c[:, inside]
    a = qf[f[0], f[1], f[2]].astype(np.int64)
    fl = np.floor(c)
    i = fl.astype(np.int64)
    r = np.floor((c - fl) * float(Q) + 0.5).astype(np.int64)
    hist = np.zeros(bins * bins, dtype=np.int64)
    for d0 in (0, 1):
        for d1 in (0, 1):
            for d2 in (0, 1):
                d = (d0, d1, d2)
                idx = [np.minimum(i[j] + d[j], qm.shape[j] - 1) for j in range(3)]
                w = np.ones(a.shape, dtype=np.int64)
                for j in range(3):
                    w = w * (r[j] if d[j] else Q - r[j])
                b = qm[idx[0], idx[1], idx[2]].astype(np.int64)
                hist += np.bincount(a * bins + b, weights=None if w.size == 0 else w.astype(np.float64),
                                    minlength=bins * bins).astype(np.int64)[:bins * bins]
    return hist.reshape(bins, bins)


def joint_hist_pv(qf, qm, origin, stride, counts, matrices, bins=32):
    """the arguments and result of bts_amd.ops.joint_hist_pv, in numpy: (K,bins,bins) int64.  A weighted np.bincount sums in float64: a
    bin's sum stays below 2^53 (at most 2^31 points of 2^15 each), so it is exact."""
    qf, qm = _as_numpy(qf), _as_numpy(qm)
    ms = np.asarray(matrices, dtype=np.float64)
    return np.stack([joint_hist_one(qf, qm, origin, stride, counts, m[:3], bins) for m in ms])


def ties(matrices, origin, stride, counts, tol=1e-9):
    """the number of lattice points, over all the matrices, where the last bit of the float64 coordinate could decide: c_j, or
    (c_j - floor(c_j)) Q + 0.5, lies within tol of an integer without being one exactly"""
    n = 0
    for m in np.asarray(matrices, dtype=np.float64):
        _, c = coordinates(m[:3], origin, stride, counts)
        t = (c - np.floor(c)) * float(Q) + 0.5
        bad = np.zeros(c.shape[1], dtype=bool)
        for v in (c, t):
            near = np.abs(v - np.round(v))
            bad |= np.any((near <= tol) & (near != 0.0), axis=0)
        n += int(bad.sum())
    return n


# ---- the phantom -------------------------------------------------------------------------------------------------------------------
def _blob(x, centre, radii, edge=0.08):
    """a smooth-edged ellipsoid: 1 inside, 0 outside, a logistic edge of `edge` of the radius"""
    d = (x - np.asarray(centre, dtype=np.float64).reshape(3, 1)) / np.asarray(radii, dtype=np.float64).reshape(3, 1)
    return 1.0 / (1.0 + np.exp((np.sqrt((d * d).sum(axis=0)) - 1.0) / edge))


def tissues(x):
    """x (3, n) world coordinates in mm -> the tissue maps in [0, 1]: head (a soft-edged ellipsoid about the origin), white matter,
    ventricles, an off-centre lesion, and a low-amplitude sinusoidal texture"""
    x = np.asarray(x, dtype=np.float64)
    rad = np.sqrt(((x / np.array([[58.0], [72.0], [52.0]])) ** 2).sum(axis=0))
    head = 1.0 / (1.0 + np.exp((rad - 1.0) * 25.0))
    wm = _blob(x, (4.0, -6.0, 5.0), (34.0, 44.0, 28.0))
    vent = _blob(x, (-9.0, 4.0, 6.0), (7.0, 17.0, 9.0)) + _blob(x, (11.0, 2.0, 4.0), (6.0, 15.0, 8.0))
    lesion = _blob(x, (24.0, -22.0, 13.0), (11.0, 9.0, 12.0))
    tex = np.sin(x[0] / 5.3) * np.sin(x[1] / 6.1 + 0.7) * np.sin(x[2] / 4.7 + 1.9)
    return head, wm, np.minimum(vent, 1.0), lesion, tex


def contrast(x, which):
    """'fixed': a T1-like mix; 'moving': a non-monotone remap of the same tissue maps (fluid and lesion bright, white matter dark)"""
    head, wm, vent, lesion, tex = tissues(x)
    if which == 'fixed':
        v = 0.30 + 0.45 * wm - 0.28 * vent + 0.22 * lesion + 0.03 * tex
    else:
        v = 0.42 - 0.20 * wm + 0.50 * vent + 0.40 * lesion * (1.0 - 0.6 * lesion) + 0.03 * tex
    return head * v


def grid_affine(shape, spacing, offset=(0.0, 0.0, 0.0)):
    """an axis-aligned voxel -> world matrix whose mid-point lies at `offset`"""
    a = np.eye(4)
    for j in range(3):
        a[j, j] = spacing[j]
        a[j, 3] = offset[j] - spacing[j] * (shape[j] - 1) / 2.0
    return a


def render(shape, affine, which, world_map=None, noise=0.02, seed=0):
    """the contrast sampled at the world positions world_map @ affine @ voxel (no interpolation), plus Gaussian noise of `noise` of full
    scale inside the head -> float32 (D,H,W)"""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    v = np.stack([g.reshape(-1) for g in grids] + [np.ones(int(np.prod(shape)))])
    m = np.asarray(affine, dtype=np.float64) if world_map is None else np.asarray(world_map, dtype=np.float64) @ np.asarray(affine, dtype=np.float64)
    x = (m @ v)[:3]
    out = contrast(x, which)
    head = tissues(x)[0]
    out = out + noise * np.random.default_rng(seed).standard_normal(out.shape) * (head > 0.5)
    return out.reshape(shape).astype(np.float32)


def phantom_pair(fixed_shape, fixed_spacing, moving_shape, moving_spacing, t_true, moving_offset=(1.3, -0.7, 2.1), seed=0):
    """-> (fixed, A_f, moving, A_m): the moving volume shows the tissue that the fixed world holds at x at its header-world position
    t_true @ x, i.e. voxel v of it is the moving contrast at inv(t_true) @ A_m @ v"""
    a_f = grid_affine(fixed_shape, fixed_spacing)
    a_m = grid_affine(moving_shape, moving_spacing, moving_offset)
    fixed = render(fixed_shape, a_f, 'fixed', seed=seed)
    moving = render(moving_shape, a_m, 'moving', world_map=np.linalg.inv(np.asarray(t_true, dtype=np.float64)), seed=seed + 1)
    return fixed, a_f, moving, a_m


def mean_tre(t, t_true, fixed_shape, a_f):
    """mean |T x - T_true x| over the fixed voxels inside the head, in units of the fixed voxel (the geometric mean of its sides)"""
    grids = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in fixed_shape], indexing='ij')
    v = np.stack([g.reshape(-1) for g in grids] + [np.ones(int(np.prod(fixed_shape)))])
    x = np.asarray(a_f, dtype=np.float64) @ v
    x = x[:, tissues(x[:3])[0] > 0.5]
    d = ((np.asarray(t) - np.asarray(t_true)) @ x)[:3]
    vox = np.sqrt((np.asarray(a_f)[:3, :3] ** 2).sum(axis=0))
    return float(np.sqrt((d * d).sum(axis=0)).mean() / vox.prod() ** (1.0 / 3.0))


# ---- the cases of the kernel tests (tests/test_coreg_gpu.py runs them, tests/test_coreg_host.py proves that none of them has a tie) ----
FIXED, MOVING = (19, 23, 37), (17, 29, 21)
LATTICES = (((0, 0, 0), (1, 1, 1), (19, 23, 37)), ((1, 1, 1), (2, 2, 2), (9, 11, 18)), ((0, 1, 0), (3, 2, 1), (7, 11, 37)),
            ((2, 5, 0), (1, 1, 1), (17, 1, 37)))


def rotation(rx, ry, rz):
    """Rz @ Ry @ Rx, degrees (bts_amd.coreg.rigid_matrix's order)"""
    cx, cy, cz = np.cos(np.radians([rx, ry, rz]))
    sx, sy, sz = np.sin(np.radians([rx, ry, rz]))
    return (np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
            @ np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]]))


def voxel_map(params, fixed_shape, fixed_spacing, moving_shape, moving_spacing):
    """fixed voxel -> moving voxel for a rigid motion about the world origin between two centred axis-aligned grids -> (3, 4)"""
    t = np.eye(4)
    t[:3, :3] = rotation(*params[3:])
    t[:3, 3] = params[:3]
    return (np.linalg.inv(grid_affine(moving_shape, moving_spacing)) @ t @ grid_affine(fixed_shape, fixed_spacing))[:3]


def shift(d0, d1, d2):
    return np.array([[1.0, 0, 0, d0], [0, 1.0, 0, d1], [0, 0, 1.0, d2]])


def thirteen():
    """thirteen different rigid maps FIXED -> MOVING at unequal spacings: a pose and +-step on each parameter, as a sweep offers them"""
    p0, out = (1.5, -2.25, 0.75, 3.0, -2.0, 4.0), []
    out.append(p0)
    for i in range(6):
        for sgn in (1.0, -1.0):
            q = list(p0)
            q[i] += sgn * (1.0 if i < 3 else 0.5)
            out.append(tuple(q))
    return np.stack([voxel_map(p, FIXED, (1.0, 0.9, 0.6), MOVING, (1.1, 0.7, 1.05)) for p in out])


def hist_cases():
    """-> [(name, fixed extent, moving extent, matrices (K,3,4))]"""
    flat = thirteen()[:3].copy()
    flat[:, 1, :] = 0.0                                          # every point at coordinate 0 of the axis of extent 1
    return [('identity', FIXED, FIXED, shift(0, 0, 0)[None]),
            ('integer shift, partly outside', FIXED, FIXED, shift(3, -4, 5)[None]),
            ('half-voxel shift', FIXED, FIXED, shift(0.5, 0.5, 0.5)[None]),
            ('general rigid', FIXED, MOVING, thirteen()[:2]),
            ('everything outside', FIXED, MOVING, shift(100, 0, 0)[None]),
            ('moving axis of extent 1', FIXED, (17, 1, 21), flat),
            ('thirteen candidates', FIXED, MOVING, thirteen())]


def binned_volume(shape, bins, seed):
    """a smooth-plus-noise volume of bin numbers with a large background of bin 0, as a skull-stripped scan has"""
    rng = np.random.default_rng(seed)
    grids = np.meshgrid(*[np.linspace(-1.0, 1.0, n) for n in shape], indexing='ij')
    rad = np.sqrt(sum(g * g for g in grids))
    v = np.where(rad < 0.9, 0.5 + 0.4 * np.sin(3.0 * grids[0] + seed) * np.cos(2.0 * grids[1]) + 0.1 * rng.standard_normal(shape), 0.0)
    return np.clip(np.floor(v * bins), 0, bins - 1).astype(np.uint8)
