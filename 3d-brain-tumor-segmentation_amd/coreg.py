"""Rigid co-registration of a scan's modalities to its first one by normalised mutual information.

The usual BraTS preparation is co-register, resample to 1 mm, skull-strip; the reference stacks its modalities voxel for voxel
(test.py:21-42) and so expects files that were registered beforehand.  `infer.Conformer` places every modality where its own header says
it is, which is only as good as the patient's stillness between two sequences.  Here one 6-parameter rigid motion per non-reference
modality is estimated and handed on as a CORRECTED AFFINE: `coregister_case` returns affines that go straight into
`Conformer.forward(vols, affines)`; nothing downstream changes.

Everything in this module runs on the host in float64.  The device does the two passes that touch voxels, `ops.quantize_bins` and
`ops.joint_hist_pv` (one launch evaluates all candidates of a sweep); the histograms, K x 8 KB, are read back, and the score is a pure
function of their integers, so a search is reproducible bit for bit and `search` neither knows nor cares where `evaluate` runs.

The search is local: it starts from the headers and is meant for motion within about +-30 mm / +-20 degrees, not for scans whose frames of
reference are unrelated."""
import collections
import math

import numpy as np

Q3 = 32 ** 3                      # what one counted lattice point adds to a histogram (bts_joint_hist_pv)
DEFAULT_BOUNDS = (30.0, 20.0)     # |translation| in mm, |rotation| in degrees, per parameter
# per level: lattice spacing (mm; the stride closest to it per axis of the fixed grid), first step (mm, degrees), smallest translation step
DEFAULT_LEVELS = ((4.0, 4.0, 4.0, 1.0), (2.0, 1.0, 1.0, 0.125))
N_PARAMS = 6

Level = collections.namedtuple('Level', 'step_mm step_deg min_mm points')
CoregResult = collections.namedtuple('CoregResult', 'params matrix affine nmi_before nmi_after evaluations overlap trace refined')


def rigid_matrix(params, centre):
    """params (tx, ty, tz in mm, rx, ry, rz in degrees), world coordinates -> the 4x4 matrix of x' = R (x - centre) + centre + t with
    R = Rz @ Ry @ Rx (the rotation about x first), right-handed"""
    p = [float(v) for v in params]
    c = np.asarray(centre, dtype=np.float64).reshape(3)
    if len(p) != N_PARAMS or not all(math.isfinite(v) for v in p):
        raise ValueError('rigid_matrix: six finite parameters (tx, ty, tz, rx, ry, rz), got %r' % (params,))
    cx, cy, cz = (math.cos(math.radians(v)) for v in p[3:])
    sx, sy, sz = (math.sin(math.radians(v)) for v in p[3:])
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    m = np.eye(4, dtype=np.float64)
    m[:3, :3] = rz @ ry @ rx
    m[:3, 3] = c + np.array(p[:3]) - m[:3, :3] @ c
    return m


def _entropy(counts, n):
    c = counts[counts > 0].astype(np.float64)
    return math.log(n) - float(np.sum(c * np.log(c))) / n


def nmi(hist):
    """Studholme's normalised mutual information (H(F) + H(M)) / H(F,M) of one integer joint histogram [fixed bin][moving bin]: natural
    logarithm, float64, 0 log 0 = 0.  In [1, 2]; 0.0 for an empty histogram, 1.0 where all mass lies in one bin (no entropy at all)."""
    h = np.asarray(hist)
    if h.ndim != 2:
        raise ValueError('nmi: one two-dimensional histogram, got shape %s' % (h.shape,))
    h = h.astype(np.int64)
    n = int(h.sum())
    if n <= 0:
        return 0.0
    joint = _entropy(h.reshape(-1), float(n))
    if joint <= 0.0:
        return 1.0
    return (_entropy(h.sum(axis=1), float(n)) + _entropy(h.sum(axis=0), float(n))) / joint


def score(hist, points, min_overlap=0.5):
    """the search's objective: nmi(hist), or -inf where fewer than min_overlap * points lattice points were counted"""
    h = np.asarray(hist).astype(np.int64)
    return nmi(h) if int(h.sum()) >= min_overlap * points * Q3 else -math.inf


def _bounds(bounds):
    try:
        mm, deg = (float(v) for v in bounds)
    except (TypeError, ValueError):
        mm = deg = -1.0
    if not (0.0 < mm < math.inf and 0.0 < deg <= 180.0):
        raise ValueError('bounds must be (mm > 0, 0 < degrees <= 180), got %r' % (bounds,))
    return mm, deg


def search(evaluate, levels, bounds=DEFAULT_BOUNDS, min_overlap=0.5, max_sweeps=200, start=None):
    """deterministic compass search for the parameters of the highest score, coarse level to fine.

    evaluate(level, params_list) -> one integer histogram per entry of params_list (any array-like (K,bins,bins)); levels: one
    Level(step_mm, step_deg, min_mm, points) each, points = the size of that level's lattice.  Per sweep ONE evaluate call: the current
    point, then +step and -step on each of the six parameters in order, 13 candidates; those outside `bounds` (|t| <= mm, |r| <= degrees)
    are not offered.  A candidate counted on fewer than min_overlap * points lattice points scores -inf.  The search moves to the best
    candidate only if it is strictly better than the current point (ties: the lowest index), else halves both steps; a level ends when
    its translation step falls below min_mm, or after max_sweeps sweeps.
    -> (params, trace); trace holds one (level, params before the sweep, step_mm, step_deg, candidates, score of the current point, best
    score, moved) per sweep"""
    mm, deg = _bounds(bounds)
    p = tuple(float(v) for v in (start if start is not None else (0.0,) * N_PARAMS))
    if len(p) != N_PARAMS:
        raise ValueError('search: start must hold six parameters')
    trace = []
    for li, lv in enumerate(levels):
        lv = Level(*lv)
        step_mm, step_deg = float(lv.step_mm), float(lv.step_deg)
        if not (step_mm > 0 and step_deg > 0 and lv.min_mm > 0):
            raise ValueError('search: steps must be positive, got %r' % (lv,))
        sweeps = 0
        while step_mm >= lv.min_mm and sweeps < max_sweeps:
            cands = [p]
            for i in range(N_PARAMS):
                for sign in (1.0, -1.0):
                    q = list(p)
                    q[i] += sign * (step_mm if i < 3 else step_deg)
                    if abs(q[i]) <= (mm if i < 3 else deg):
                        cands.append(tuple(q))
            hists = evaluate(li, cands)
            if len(hists) != len(cands):
                raise ValueError('search: evaluate returned %d histograms for %d candidates' % (len(hists), len(cands)))
            scores = [score(h, lv.points, min_overlap) for h in hists]
            best = max(range(len(cands)), key=lambda k: (scores[k], -k))
            moved = scores[best] > scores[0]
            trace.append((li, p, step_mm, step_deg, len(cands), scores[0], scores[best], moved))
            if moved:
                p = cands[best]
            else:
                step_mm, step_deg = 0.5 * step_mm, 0.5 * step_deg
            sweeps += 1
    return p, trace


def lattice(shape, affine, spacing_mm):
    """-> (origin, stride, counts): per axis of the grid the stride closest to spacing_mm (at least 1, at most the extent), origin
    stride // 2, and as many points as lie inside the extent"""
    a = np.asarray(affine, dtype=np.float64)
    vox = np.sqrt((a[:3, :3] ** 2).sum(axis=0))
    stride = tuple(min(int(n), max(1, int(math.floor(float(spacing_mm) / v + 0.5)))) for n, v in zip(shape, vox))
    origin = tuple(s // 2 for s in stride)
    counts = tuple((int(n) - 1 - o) // s + 1 for n, o, s in zip(shape, origin, stride))
    return origin, stride, counts


def grid_aligned(voxel_map, tol=1e-6):
    """does the 3x4 fixed voxel -> moving voxel map send grid points onto grid points: a signed permutation and an integer translation?"""
    m = np.asarray(voxel_map, dtype=np.float64)[:3]
    lin = np.round(m[:, :3])
    return bool(np.abs(m - np.round(m)).max() <= tol and np.array_equal(np.abs(lin).sum(axis=0), np.ones(3))
                and np.array_equal(np.abs(lin).sum(axis=1), np.ones(3)))


def parabola_vertex(s_minus, s_0, s_plus):
    """the abscissa in [-0.5, 0.5] of the vertex of the parabola through (-1, s_minus), (0, s_0), (1, s_plus); 0.0 unless s_0 is finite
    and at least as large as both neighbours and the three are not on a line"""
    if not (math.isfinite(s_minus) and math.isfinite(s_0) and math.isfinite(s_plus)) or s_0 < s_minus or s_0 < s_plus:
        return 0.0
    den = s_minus - 2.0 * s_0 + s_plus
    return 0.5 * (s_minus - s_plus) / den if den < 0.0 else 0.0


def percentile_bounds(sorted_values, p_lo=0.5, p_hi=99.5):
    """the two percentiles by ops.case_norm's rule, s[k] + f (s[min(k+1,n-1)] - s[k]) with h = (n-1) p / 100, k = floor(h), f = h - k"""
    s = np.asarray(sorted_values, dtype=np.float64)
    out = []
    for p in (p_lo, p_hi):
        h = (s.size - 1) * p / 100.0
        k = int(math.floor(h))
        out.append(float(s[k] + (h - k) * (s[min(k + 1, s.size - 1)] - s[k])))
    return tuple(out)


def quantize_host(x, lo, hi, bins):
    """numpy restatement of ops.quantize_bins"""
    t = np.floor((np.asarray(x, dtype=np.float32).astype(np.float64) - lo) * float(bins) / (hi - lo))
    return np.where(t >= 0.0, np.minimum(t, bins - 1.0), 0.0).astype(np.uint8)


def _binned(vol, bins, who):
    """one (D,H,W) volume -> its bin numbers (uint8, dense) between its exact 0.5 / 99.5 percentiles: on the device for a device tensor
    (ops.case_norm's order statistics, ops.quantize_bins), in numpy for an array"""
    if isinstance(vol, np.ndarray):
        if vol.ndim != 3 or vol.size < 1:
            raise ValueError('coregister: %s must be a non-empty (D,H,W) volume, got shape %s' % (who, vol.shape))
        v = np.ascontiguousarray(vol, dtype=np.float32)
        lo, hi = percentile_bounds(np.sort(v, axis=None))
        if not hi > lo:
            raise ValueError('coregister: %s is constant between its 0.5 and 99.5 percentiles (%g)' % (who, lo))
        return quantize_host(v, lo, hi, bins)
    import torch
    from . import ops
    if not isinstance(vol, torch.Tensor) or vol.dim() != 3 or vol.numel() < 1:
        raise ValueError('coregister: %s must be a non-empty (D,H,W) volume' % who)
    if not vol.is_cuda:
        raise RuntimeError('coregister: %s must live on the GPU, or be a numpy array with a numpy `evaluate`' % who)
    v = vol.to(torch.float32).contiguous()
    _, stats = ops.case_norm(v.unsqueeze(-1), mask=torch.ones_like(v), clip=(0.5, 99.5))
    lo, hi = (float(t) for t in stats[3:5].cpu())             # one host round trip per volume, once per case
    if not hi > lo:
        raise ValueError('coregister: %s is constant between its 0.5 and 99.5 percentiles (%g)' % (who, lo))
    return ops.quantize_bins(v, lo, hi, bins)


def _to_numpy(h):
    return h.cpu().numpy() if hasattr(h, 'cpu') else np.asarray(h)


def coregister(fixed, fixed_affine, moving, moving_affine, bins=32, levels=None, bounds=DEFAULT_BOUNDS, evaluate=None, min_overlap=0.5):
    """estimate the rigid motion T (fixed world -> moving header world) that brings `moving` onto `fixed`.

    fixed, moving: (D,H,W) volumes on their own grids, device tensors (or numpy arrays, with a numpy `evaluate`); the affines: their 4x4
    voxel -> world matrices.  levels: (lattice spacing mm, first step mm, first step degrees, smallest step mm) each, default
    DEFAULT_LEVELS; bounds: (mm, degrees).  evaluate: the histogram backend, a callable with the arguments and result of
    `ops.joint_hist_pv` (the default); it is handed the binned volumes as they are.
    Both volumes are binned between their own 0.5 / 99.5 percentiles; the centre of rotation is the world position of the fixed volume's
    mid-voxel; candidate p is evaluated through the voxel map inv(A_m) @ rigid_matrix(p, centre) @ A_f.  The search starts at the
    identity; its result is kept only if it scores strictly higher than the identity on the finest lattice, so nmi_after >= nmi_before.
    Where the search ends ON the grid (`grid_aligned`: two volumes on one grid, no rotation found -- the regime in which partial-volume
    interpolation cannot see below a voxel), the translation is refined per moving axis by the vertex of the parabola
    through the scores of the end point and of its two grid-aligned neighbours, seven more histograms in one launch, none of them
    interpolated (an end point at the identity is left alone: headers that nothing moved stay exact); `refined` says so, and nmi_after stays the score of the search's end point.
    -> CoregResult: params, matrix (T), affine = inv(T) @ moving_affine (the corrected affine), nmi_before and nmi_after on the finest
    lattice, evaluations (candidate histograms computed), overlap (the fraction of the finest lattice that the search's end point maps
    inside `moving`), trace, refined"""
    a_f, a_m = np.asarray(fixed_affine, dtype=np.float64), np.asarray(moving_affine, dtype=np.float64)
    if a_f.shape != (4, 4) or a_m.shape != (4, 4) or not (np.all(np.isfinite(a_f)) and np.all(np.isfinite(a_m))):
        raise ValueError('coregister: the affines must be finite 4x4 matrices')
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= 64:
        raise ValueError('coregister: bins must be an integer in 2..64, got %r' % (bins,))
    bins = int(bins)
    bounds = _bounds(bounds)
    levels = DEFAULT_LEVELS if levels is None else tuple(tuple(float(v) for v in lv) for lv in levels)
    if not levels or any(len(lv) != 4 or min(lv) <= 0 for lv in levels):
        raise ValueError('coregister: levels must be (lattice spacing mm, step mm, step degrees, smallest step mm) each, got %r' % (levels,))
    if evaluate is None:
        if isinstance(fixed, np.ndarray) or isinstance(moving, np.ndarray):
            raise RuntimeError('coregister: numpy volumes need a numpy `evaluate`; the default runs on the GPU')
        from . import ops
        evaluate = ops.joint_hist_pv
    qf, qm = _binned(fixed, bins, 'fixed'), _binned(moving, bins, 'moving')
    shape = tuple(int(v) for v in qf.shape)
    lattices = [lattice(shape, a_f, lv[0]) for lv in levels]
    centre = (a_f @ np.array([(n - 1) // 2 for n in shape] + [1], dtype=np.float64))[:3]
    inv_m = np.linalg.inv(a_m)
    count = [0]

    def voxel_map(p):
        return (inv_m @ rigid_matrix(p, centre) @ a_f)[:3]

    def run(level, params_list):
        o, s, n = lattices[level]
        count[0] += len(params_list)
        return _to_numpy(evaluate(qf, qm, o, s, n, np.stack([voxel_map(p) for p in params_list]), bins))

    points = [int(np.prod(lt[2])) for lt in lattices]
    params, trace = search(run, [Level(lv[1], lv[2], lv[3], pts) for lv, pts in zip(levels, points)], bounds, min_overlap)
    zero = (0.0,) * N_PARAMS
    last = len(levels) - 1
    h0, h1 = run(last, [zero, params])
    before, after = nmi(h0), score(h1, points[last], min_overlap)
    if not after > before:                                     # never worse than the headers by the finest lattice's own measure
        params, h1, after = zero, h0, before
    refined = False
    end = voxel_map(params)
    if tuple(params) != zero and grid_aligned(end):          # headers that the search did not move are kept exactly
        o, s, n = lattices[last]
        shifted = [end] + [end + np.outer(sign * np.eye(3)[j], [0.0, 0.0, 0.0, 1.0]) for j in range(3) for sign in (-1.0, 1.0)]
        count[0] += len(shifted)
        sc = [score(h, points[last], min_overlap) for h in _to_numpy(evaluate(qf, qm, o, s, n, np.stack(shifted), bins))]
        delta = np.array([parabola_vertex(sc[1 + 2 * j], sc[0], sc[2 + 2 * j]) for j in range(3)])
        moved = tuple(float(v) for v in np.asarray(params[:3]) + a_m[:3, :3] @ delta) + tuple(params[3:])
        if np.any(delta != 0.0) and all(abs(v) <= bounds[0] for v in moved[:3]):
            params, refined = moved, True
    t = rigid_matrix(params, centre)
    return CoregResult(refined=refined, params=tuple(params), matrix=t, affine=np.linalg.inv(t) @ a_m, nmi_before=before, nmi_after=after,
                       evaluations=count[0], overlap=float(int(np.asarray(h1).astype(np.int64).sum()) // Q3) / points[last], trace=trace)


def coregister_case(vols, affines, **kw):
    """register every modality of a case to its first one -> (corrected affines, [None, CoregResult, ...]).  Modality 0 keeps its affine;
    modality c > 0 gets inv(T_c) @ A_c, through which `infer.Conformer.plan` reads it at inv(A_c) @ T_c @ target_affine.  The corrected
    list goes straight into `Conformer.forward(vols, affines)`.  **kw: as `coregister`."""
    if len(vols) != len(affines) or not len(vols):
        raise ValueError('coregister_case: one affine per modality, got %d and %d' % (len(vols), len(affines)))
    out, results = [np.asarray(affines[0], dtype=np.float64)], [None]
    for c in range(1, len(vols)):
        r = coregister(vols[0], affines[0], vols[c], affines[c], **kw)
        out.append(r.affine)
        results.append(r)
    return out, results


def format_result(name, r):
    """the one line the command line prints per registered modality"""
    return '%s: t = (%.3f, %.3f, %.3f) mm, r = (%.3f, %.3f, %.3f) deg, NMI %.6f -> %.6f, %d evaluations' % (
        (name,) + tuple(r.params) + (r.nmi_before, r.nmi_after, r.evaluations))
