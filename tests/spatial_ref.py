"""float64 numpy restatement of the spatial training augmentation (bts_augment_spatial_batch), and the cases, draws
and tolerances that tests/test_spatial_host.py (no GPU) and tests/test_spatial_gpu.py share.

For an output voxel t of a crop of extent T, from a source volume of extent S at window origin o:
  t~_k = flip_k ? T_k-1-t_k : t_k,  q = t~ - (T-1)/2,  s = o + (T-1)/2 + M q + u(t~),
  u(t~) = sum_{a,b,c=0..3} B_a(f0) B_b(f1) B_c(f2) phi[i0+a, i1+b, i2+c, :],  g = t~/spacing, i = floor(g), f = g - i,
  image: trilinear at s, corners outside the volume contribute fill[c] (scipy.ndimage mode='grid-constant'), then
  (v + shift sqrt(var)) scale with var the population variance of the whole volume; labels: voxel floor(s + 0.5), 0 outside,
  one-hot without the background.
"""
import numpy as np

# volume -> crop, C, out_ch
SHAPES = [((9, 10, 11), (8, 8, 8), 2, 3),
          ((16, 12, 20), (16, 8, 16), 4, 1),
          ((5, 5, 5), (5, 5, 5), 1, 3),
          ((20, 18, 24), (12, 10, 15), 2, 3)]        # odd T2: no four-voxel store path could serve it
MODES = ('affine', 'elastic4', 'elastic8', 'both')
# Shapes at which the kernel takes another path than at the four above, as (volume, crop, C, out_ch, spacing), mode 'both':
EXTRA = [((6, 15, 16), (4, 14, 14), 2, 3, 1),        # 17 x 17 control nodes per plane: too many for the LDS stage, the field is read from memory
         ((4, 5, 72), (3, 4, 70), 2, 3, 8),          # a row longer than a wave: a lane takes more than one voxel
         ((66, 33, 9), (64, 32, 8), 2, 2, 8)]        # 384 planes: six rows per work unit, all four waves busy, two rounds of rows
DRAWS = 6
TIE_EPS = 1e-4          # labels are compared away from float64 coordinates this close to a rounding tie ...
TIE_CAP = 0.02          # ... which may be at most this share of a case


def bspline(f):
    """the four uniform cubic B-spline basis values at fraction f"""
    return [(1 - f) ** 3 / 6, (3 * f ** 3 - 6 * f ** 2 + 4) / 6, (-3 * f ** 3 + 3 * f ** 2 + 3 * f + 1) / 6, f ** 3 / 6]


def rotation(axis, a):
    i, j = (axis + 1) % 3, (axis + 2) % 3
    r = np.eye(3)
    r[i, i], r[i, j], r[j, i], r[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
    return r


def matrix(angles, zoom):
    """M = R0 R1 R2 / z"""
    return rotation(0, angles[0]).dot(rotation(1, angles[1])).dot(rotation(2, angles[2])) / zoom


def grid(crop, spacing):
    return tuple((t - 1) // spacing + 4 for t in crop)


def field(phi, crop, spacing, dtype=np.float64):
    """u(t~) on the whole crop -> (T0,T1,T2,3); dtype float32 follows the kernel's order: the two outer axes are reduced first (a outer,
    b inner, weight B_a B_b), then the four taps along axis 2"""
    phi = np.asarray(phi, dtype)
    idx, w = [], []
    for k in range(3):
        t = np.arange(crop[k])
        i = t // spacing
        f = ((t - i * spacing).astype(dtype) / dtype(spacing)).astype(dtype)
        idx.append(i)
        w.append([b.astype(dtype) for b in bspline(f)] if dtype is np.float64 else _bspline32(f))
    red = np.zeros((crop[0], crop[1]) + phi.shape[2:], dtype)
    for a in range(4):
        for b in range(4):
            wab = (w[0][a][:, None] * w[1][b][None, :]).astype(dtype)
            red = (red + wab[:, :, None, None] * phi[idx[0] + a][:, idx[1] + b]).astype(dtype)
    u = np.zeros(tuple(crop) + (3,), dtype)
    for c in range(4):
        u = (u + w[2][c][None, None, :, None] * red[:, :, idx[2] + c]).astype(dtype)
    return u


def _bspline32(f):
    f = f.astype(np.float32)
    one, six = np.float32(1), np.float32(1.0) / np.float32(6.0)
    g, f2 = one - f, f * f
    f3 = f2 * f
    return [g * g * g * six, (np.float32(3) * f3 - np.float32(6) * f2 + np.float32(4)) * six,
            (np.float32(-3) * f3 + np.float32(3) * f2 + np.float32(3) * f + one) * six, f3 * six]


def coordinates(crop, offsets, M, phi=None, spacing=1, dtype=np.float64):
    """s for every unflipped crop voxel t~ -> (T0,T1,T2,3).  dtype float32 restates the kernel's documented arithmetic in numpy float32
    (without its fused multiply-adds): m_k = (M_k0 q0 + M_k1 q1) + M_k2 q2, s_k = ((o_k + h_k) + m_k) + u_k"""
    M = np.asarray(M, np.float64).reshape(3, 3).astype(dtype)      # (the kernel gets 9 floats: their rounding is part of delta)
    q = [(np.arange(crop[k]).astype(dtype) - dtype((crop[k] - 1) * 0.5)) for k in range(3)]
    q0, q1, q2 = q[0][:, None, None], q[1][None, :, None], q[2][None, None, :]
    s = np.empty(tuple(crop) + (3,), dtype)
    for k in range(3):
        m = ((M[k, 0] * q0 + M[k, 1] * q1).astype(dtype) + M[k, 2] * q2).astype(dtype)
        s[..., k] = dtype(offsets[k]) + dtype((crop[k] - 1) * 0.5) + m
    if phi is not None:
        s = (s + field(phi, crop, spacing, dtype)).astype(dtype)
    return s


def sample_linear(x, s, fill):
    """trilinear, grid-constant: x (S0,S1,S2,C) float64, s (...,3), fill (C,) -> (...,C)"""
    S = x.shape[:3]
    j = np.floor(s).astype(np.int64)
    w = s - j
    out = np.zeros(s.shape[:-1] + (x.shape[3],))
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                jj = [j[..., 0] + a, j[..., 1] + b, j[..., 2] + c]
                inside = np.ones(s.shape[:-1], bool)
                for k in range(3):
                    inside &= (jj[k] >= 0) & (jj[k] < S[k])
                v = x[np.clip(jj[0], 0, S[0] - 1), np.clip(jj[1], 0, S[1] - 1), np.clip(jj[2], 0, S[2] - 1)]
                v = np.where(inside[..., None], v, np.asarray(fill, np.float64))
                wt = ((w[..., 0] if a else 1 - w[..., 0]) * (w[..., 1] if b else 1 - w[..., 1]) * (w[..., 2] if c else 1 - w[..., 2]))
                out += wt[..., None] * v
    return out


def sample_nearest(y, s):
    """labels y (S0,S1,S2) at floor(s + 0.5); 0 outside"""
    S = y.shape
    j = np.floor(s + 0.5).astype(np.int64)
    inside = np.ones(s.shape[:-1], bool)
    for k in range(3):
        inside &= (j[..., k] >= 0) & (j[..., k] < S[k])
    v = y[np.clip(j[..., 0], 0, S[0] - 1), np.clip(j[..., 1], 0, S[1] - 1), np.clip(j[..., 2], 0, S[2] - 1)]
    return np.where(inside, v, 0)


def ties(s, eps=TIE_EPS):
    """voxels whose coordinate is within eps of a rounding tie (k + 1/2) on some axis"""
    r = s + 0.5
    return (np.abs(r - np.round(r)) < eps).any(axis=-1)


def _flip(a, flips):
    for k in range(3):
        if flips[k]:
            a = np.flip(a, axis=k)
    return a


def augment(x, y, crop, offsets, flips, shift, scale, out_ch, M, phi=None, spacing=1, fill=None):
    """x (S0,S1,S2,C), y (S0,S1,S2) arrays -> (x_out (T,C) float64, one-hot (T,out_ch), tie mask (T)), all indexed by the output voxel"""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64).reshape(x.shape[:3])
    C = x.shape[3]
    fill = np.zeros(C) if fill is None else np.asarray(fill, np.float64)
    s = coordinates(crop, offsets, M, phi, spacing)
    v = sample_linear(x, s, fill)
    sd = np.sqrt(x.reshape(-1, C).var(axis=0))
    v = (v + np.asarray(shift, np.float64) * sd) * np.asarray(scale, np.float64)
    lbl = sample_nearest(y, s).astype(np.int64)
    onehot = np.stack([(lbl == k + 1) for k in range(out_ch)], axis=-1).astype(np.float64)
    return (np.ascontiguousarray(_flip(v, flips)), np.ascontiguousarray(_flip(onehot, flips)), np.ascontiguousarray(_flip(ties(s), flips)))


# ---- the shared cases -------------------------------------------------------------------------------------------------------------
def volumes(n, vol, c, out_ch, seed):
    """n seeded volumes (float32 (S,C)) with integer labels (float32 (S,1))"""
    rs = np.random.RandomState(seed)
    xs = [(rs.randn(*(vol + (c,))) * 30 + 20).astype(np.float32) for _ in range(n)]
    ys = [rs.randint(0, out_ch + 1, vol + (1,)).astype(np.float32) for _ in range(n)]
    return xs, ys


def lipschitz(x, fill=0.0):
    """(L of the volume: the largest |difference| of two adjacent voxels, the same with the fill border included)"""
    x = np.asarray(x, np.float64)
    inner = max(float(np.abs(np.diff(x, axis=k)).max()) for k in range(3) if x.shape[k] > 1)
    pad = np.pad(x, ((1, 1), (1, 1), (1, 1), (0, 0)), constant_values=fill)
    return inner, max(float(np.abs(np.diff(pad, axis=k)).max()) for k in range(3))


class Case(object):
    """the six draws of one (shape, mode): offsets, flips (mask (6 shape + d) % 8: every mask thrice over the shapes), shift, scale,
    angles up to 30 degrees and zoom in 0.7..1.4 (M = I in the elastic-only modes), N(0, 2^2) control nodes at spacing 4 or 8"""

    def __init__(self, shape_index, mode, extra=False):
        spacing = None
        if extra:
            self.vol, self.crop, self.c, self.out_ch, spacing = EXTRA[shape_index]
            shape_index += len(SHAPES)
        else:
            self.vol, self.crop, self.c, self.out_ch = SHAPES[shape_index]
        self.mode = mode
        self.xs, self.ys = volumes(DRAWS, self.vol, self.c, self.out_ch, seed=100 + shape_index)
        rs = np.random.RandomState(1000 + 10 * shape_index + MODES.index(mode))
        self.draws = []
        for d in range(DRAWS):
            mask = (DRAWS * shape_index + d) % 8
            dr = {'offsets': [int(rs.randint(0, self.vol[k] - self.crop[k] + 1)) for k in range(3)],
                  'flips': [bool(mask & 4), bool(mask & 2), bool(mask & 1)], 'mask': mask,
                  'shift': rs.uniform(-0.1, 0.1, self.c).tolist(), 'scale': rs.uniform(0.9, 1.1, self.c).tolist()}
            angles, zoom = np.deg2rad(rs.uniform(-30, 30, 3)), rs.uniform(0.7, 1.4)
            dr['M'] = matrix(angles, zoom) if mode in ('affine', 'both') else np.eye(3)
            dr['spacing'] = spacing or {'affine': 4, 'elastic4': 4, 'elastic8': 8, 'both': (4, 8)[d % 2]}[mode]
            g = grid(self.crop, dr['spacing'])
            dr['phi'] = None if mode == 'affine' else (rs.randn(*(g + (3,))) * 2.0).astype(np.float32)
            self.draws.append(dr)

    def reference(self, d):
        dr = self.draws[d]
        return augment(self.xs[d], self.ys[d], self.crop, dr['offsets'], dr['flips'], dr['shift'], dr['scale'], self.out_ch, dr['M'],
                       dr['phi'], dr['spacing'])


    def delta(self):
        """4 x the largest |float32 restatement of the kernel's coordinate arithmetic - float64 reference| over this case's draws"""
        worst = 0.0
        for dr in self.draws:
            s64 = coordinates(self.crop, dr['offsets'], dr['M'], dr['phi'], dr['spacing'])
            s32 = coordinates(self.crop, dr['offsets'], dr['M'], dr['phi'], dr['spacing'], dtype=np.float32)
            worst = max(worst, float(np.abs(s32.astype(np.float64) - s64).max()))
        return 4.0 * worst


_CASES = {}


def case(shape_index, mode, extra=False):
    """built once, shared and left unchanged"""
    key = (shape_index, mode, extra)
    if key not in _CASES:
        _CASES[key] = Case(shape_index, mode, extra)
    return _CASES[key]


_DELTA = []


def coordinate_delta():
    """delta of the intensity tolerance: 4 x the largest |float32 restatement of the kernel's coordinate arithmetic - float64 reference|
    over every draw of every case (the factor covers fused multiply-adds and ordering)"""
    if not _DELTA:
        _DELTA.append(max(case(si, mode).delta() for si in range(len(SHAPES)) for mode in MODES))
    return _DELTA[0]


def intensity_bound(x, xref, delta=None):
    """|d| <= 3 delta L + 1e-5 max|x|; delta: coordinate_delta() of the four shapes, or an extra case's own"""
    return 3.0 * (coordinate_delta() if delta is None else delta) * lipschitz(x)[0] + 1e-5 * float(np.abs(xref).max())
