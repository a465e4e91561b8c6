"""float64 restatement of bts_intensity_batch (include/bts_hip.h) in numpy, a float32 restatement in the kernel's documented order of
operations (csrc/intensity.hip), and the cases the host and device tests share.

A parameter entry is (flags, s, sigma, m, f, gamma) for one (example, channel) volume; flags is a sum of NOISE .. INVERT.  Every
parameter of a case is a float32 value, as the device receives it."""
import functools

import numpy as np

NOISE, BLUR, BRIGHT, CONTRAST, GAMMA, INVERT = 1, 2, 4, 8, 16, 32
F32, F64 = np.float32, np.float64
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)


# ---- noise ---------------------------------------------------------------------------------------------------------------------------
def philox(counter, key):
    """Philox4x32-10: counter = four uint32 arrays (or ints), key = (k0, k1) -> four uint32 arrays"""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in counter]
    k0, k1 = np.uint64(key[0] & 0xffffffff), np.uint64(key[1] & 0xffffffff)
    for _ in range(10):
        a, b = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(b >> np.uint64(32)) ^ c[1] ^ k0, b & MASK, (a >> np.uint64(32)) ^ c[3] ^ k1, a & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return [v.astype(np.uint32) for v in c]


def _words(key, n):
    """the words (w_a, w_b) of elements 0..n-1 and whether an element is the sine of its pair"""
    e = np.arange(n, dtype=np.uint64)
    q = e >> np.uint64(2)
    nq = int(q[-1]) + 1
    cnt = np.arange(nq, dtype=np.uint64)
    o = philox((cnt & MASK, cnt >> np.uint64(32), np.zeros(nq, np.uint64), np.zeros(nq, np.uint64)), key)
    k = (e & np.uint64(3)).astype(np.int64)
    qi = q.astype(np.int64)
    hi = (k & 2) != 0
    wa = np.where(hi, o[2][qi], o[0][qi])
    wb = np.where(hi, o[3][qi], o[1][qi])
    return wa, wb, (k & 1) != 0


def normals(key, n):
    """z[e], e = 0..n-1, in float64"""
    wa, wb, sine = _words(key, n)
    u1 = ((wa >> np.uint32(8)).astype(F64) + 1.0) * 2.0 ** -24
    u2 = (wb >> np.uint32(8)).astype(F64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return np.where(sine, r * np.sin(2.0 * np.pi * u2), r * np.cos(2.0 * np.pi * u2))


def normals32(key, n):
    """z[e] as the kernel computes it: every operation rounded to float32"""
    wa, wb, sine = _words(key, n)
    u1 = ((wa >> np.uint32(8)) + np.uint32(1)).astype(F32) * F32(2.0 ** -24)
    u2 = (wb >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    r = np.sqrt(F32(-2.0) * np.log(u1))
    ang = F32(6.283185307179586) * u2
    assert r.dtype == F32 and ang.dtype == F32
    return np.where(sine, r * np.sin(ang), r * np.cos(ang)).astype(F32)


# ---- blur ----------------------------------------------------------------------------------------------------------------------------
def blur_weights(sigma):
    """(r, w[0..r]) in float64: scipy.ndimage's kernel, exp(-j^2 / (2 sigma^2)) over j = -r..r divided by its sum"""
    sigma = float(sigma)
    r = int(4.0 * sigma + 0.5)
    j = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * j ** 2)
    phi = phi / phi.sum()
    return r, phi[r:]


def reflect(i, n):
    """scipy's mode='reflect' (d c b a | a b c d | d c b a), of period 2n"""
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def fma32(a, b, c):
    """fmaf on float32 operands: the product is exact in float64, the sum is rounded once more than fmaf's (to float64 first), which
    changes a float32 result only when the float64 sum lands within 2^-29 relative of a float32 tie"""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def blur(v, sigma, single=False):
    """the separable blur, axes 2, 1, 0, taps j = -r..r accumulated from 0 in that order; single: float32 weights and fmaf per tap"""
    r, w = blur_weights(sigma)
    v = np.asarray(v, F32 if single else F64)
    if single:
        w = w.astype(F32)
    for axis in (2, 1, 0):
        idx = np.arange(v.shape[axis])
        acc = np.zeros(v.shape, v.dtype)
        for j in range(-r, r + 1):
            tap = np.take(v, reflect(idx + j, v.shape[axis]), axis=axis)
            acc = fma32(w[abs(j)], tap, acc) if single else acc + w[abs(j)] * tap
        v = acc
    return v


# ---- the chain of one (n, c) volume -----------------------------------------------------------------------------------------------------
def chain(v, entry, z):
    """float64: v (T0,T1,T2), entry = (flags, s, sigma, m, f, gamma), z = this volume's normals (float64, (T0,T1,T2))"""
    flags, s, sigma, m, f, g = entry
    v = np.asarray(v, F64).copy()
    if flags & NOISE:
        v = v + s * z
    if flags & BLUR:
        v = blur(v, sigma)
    if flags & BRIGHT:
        v = v * m
    if flags & CONTRAST:
        mu, lo, hi = v.mean(), v.min(), v.max()
        v = np.clip((v - mu) * f + mu, lo, hi)
    if flags & GAMMA:
        if flags & INVERT:
            v = -v
        mu, sd, lo = v.mean(), v.std(), v.min()
        R = v.max() - lo
        v = np.power((v - lo) / (R + 1e-7), g) * R + lo
        v = (v - v.mean()) / (v.std() + 1e-8) * sd + mu
        if flags & INVERT:
            v = -v
    return v


def chain32(v, entry, z32):
    """the same in the kernel's order with every operation rounded to float32; the statistics are float64 sums over the float32 values,
    rounded to float32, as the kernel's are"""
    flags = entry[0]
    s, sigma, m, f, g = (F32(a) for a in entry[1:])
    v = np.asarray(v, F32).copy()
    mean = lambda a: F32(a.astype(F64).mean())      # noqa: E731
    std = lambda a: F32(a.astype(F64).std())        # noqa: E731
    if flags & NOISE:
        v = fma32(s, z32, v)
    if flags & BLUR:
        v = blur(v, float(sigma), single=True)
    if flags & BRIGHT:
        v = v * m
    if flags & CONTRAST:
        mu, lo, hi = mean(v), v.min(), v.max()
        v = np.minimum(np.maximum(fma32(v - mu, f, mu), lo), hi)
    if flags & GAMMA:
        y = -v if flags & INVERT else v
        mu, sd, lo = mean(y), std(y), y.min()
        R = F32(y.max() - lo)
        p = np.power((y - lo) / (R + F32(1e-7)), g)
        assert p.dtype == F32
        y = fma32(p, R, lo)
        mu2, sd2 = mean(y), std(y)
        o = fma32((y - mu2) / (sd2 + F32(1e-8)), sd, mu)
        v = -o if flags & INVERT else o
    assert v.dtype == F32
    return v


def apply_batch(x, params, keys, single=False):
    """x: (N,T0,T1,T2,C) float32, channels last -> the float64 (or float32, with single) result of bts_intensity_batch"""
    n, t0, t1, t2, c = x.shape
    out = np.empty(x.shape, F32 if single else F64)
    for i in range(n):
        z = None
        if any(e[0] & NOISE for e in params[i]):
            z = (normals32 if single else normals)(keys[i], t0 * t1 * t2 * c).reshape(t0, t1, t2, c)
        for j in range(c):
            zz = None if z is None else z[..., j]
            out[i, ..., j] = (chain32 if single else chain)(x[i, ..., j], params[i][j], zz)
    return out


# ---- the shared cases ------------------------------------------------------------------------------------------------------------------
# (5,4,3): every extent below the blur radius; (12,10,15) C3: no vector-width alignment; (3,4,70): a row longer than a wave;
# (26,27,25): 17550 voxels > 64 blocks x 256 threads, so the statistics take all 64 blocks and a second round of the grid-stride loop
SHAPES = [((5, 4, 3), 1), ((9, 10, 11), 2), ((12, 10, 15), 3), ((3, 4, 70), 4), ((26, 27, 25), 2)]
KINDS = ('noise', 'blur', 'bright', 'contrast', 'gamma', 'chain')
_ALONE = {'noise': NOISE, 'blur': BLUR, 'bright': BRIGHT, 'contrast': CONTRAST, 'gamma': GAMMA}
_MIXED = (BLUR | CONTRAST, NOISE | BRIGHT | GAMMA, BLUR | GAMMA | INVERT, 0)
NDRAWS = 3


def volumes(si, n=NDRAWS):
    """N(0,1) with a constant background region (two slabs along the longest axis), like normalised skull-stripped scans"""
    crop, c = SHAPES[si]
    rs = np.random.RandomState(100 + si)
    x = rs.randn(n, *crop, c).astype(F32)
    axis = int(np.argmax(crop))
    edge = max(1, crop[axis] // 5)
    sl = [slice(None)] * 5
    for part in (slice(0, edge), slice(crop[axis] - edge, None)):
        sl[1 + axis] = part
        x[tuple(sl)] = 0.0
    return x


class Case(object):
    def __init__(self, si, kind):
        crop, c = SHAPES[si]
        self.si, self.kind, self.crop, self.c = si, kind, crop, c
        self.x = volumes(si)
        rs = np.random.RandomState(1000 * KINDS.index(kind) + si)
        f32 = lambda v: float(F32(v))      # noqa: E731
        self.params, self.keys = [], []
        for d in range(NDRAWS):
            row = []
            for j in range(c):
                side = d % 2 if kind == 'chain' else (d + j) % 2
                f = rs.uniform(0.65, 1.0) if side == 0 else rs.uniform(1.0, 1.5)
                g = rs.uniform(0.5, 1.0) if side == 0 else rs.uniform(1.0, 2.0)
                sigma = rs.uniform(1.4, 3.0) if si == 0 else rs.uniform(0.6, 2.5)
                s, m = rs.uniform(0.02, 0.3), rs.uniform(0.7, 1.3)
                if kind == 'chain':
                    flags = (31, 63, _MIXED[j % 4])[d]
                else:
                    flags = _ALONE[kind] | (INVERT if kind == 'gamma' and (d + j) % 3 == 1 else 0)
                row.append((flags, f32(s), f32(sigma), f32(m), f32(f), f32(g)))
            self.params.append(row)
            self.keys.append((int(rs.randint(0, 2 ** 32, dtype=np.uint64)), int(rs.randint(0, 2 ** 32, dtype=np.uint64))))
        self._ref = self._ref32 = None

    def ref(self):
        if self._ref is None:
            self._ref = apply_batch(self.x, self.params, self.keys)
            self._ref.setflags(write=False)
        return self._ref

    def ref32(self):
        if self._ref32 is None:
            self._ref32 = apply_batch(self.x, self.params, self.keys, single=True)
            self._ref32.setflags(write=False)
        return self._ref32

    def restatement_gap(self):
        """the largest |float32 restatement - float64 restatement| of the case"""
        return float(np.abs(self.ref32().astype(F64) - self.ref()).max())

    def ranges(self):
        """(N, C): max - min of every result volume"""
        r = self.ref()
        return r.max(axis=(1, 2, 3)) - r.min(axis=(1, 2, 3))

    def bound(self):
        """(N, C) absolute tolerance of the device result against ref(), per (example, channel) volume"""
        r = self.ref()
        peak = np.abs(r).max(axis=(1, 2, 3))
        if self.kind == 'noise':
            s = np.array([[e[1] for e in row] for row in self.params])
            return 2e-5 * s + 2.0 ** -23 * peak
        if self.kind == 'blur':
            rad = np.array([[blur_weights(e[2])[0] for e in row] for row in self.params])
            return 6.0 * (2 * rad + 3) * 2.0 ** -24 * np.abs(self.x.astype(F64)).max(axis=(1, 2, 3))
        if self.kind == 'bright':
            return 2.0 ** -24 * peak          # (the device test asks for bit equality with the float32 product as well)
        gamma = np.array([[1.0 if e[0] & GAMMA else 0.0 for e in row] for row in self.params])
        return 4.0 * self.restatement_gap() + gamma * 4.0 * 2.0 ** -24 * self.ranges()


@functools.lru_cache(maxsize=None)
def case(si, kind):
    return Case(si, kind)
