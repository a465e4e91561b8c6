"""Input pipeline with the augmentation on the device (reference train.py:12-64).

`prepare_dataset` keeps the reference's signature and per-example transformation (`parse_example`, train.py:14-49):
intensity shift/scale by per-channel sigma, random crop of the concatenated (x, y), independent flips of the three
axes with p = 0.5, one-hot labels minus the background channel -- note the reference applies it to the validation set
too (the same map function serves both, train.py:74-89).  Differences:
  * storage: TFRecord protos (train.py:51-58, preprocess.py:88-96) need TensorFlow; examples are read from `.npz` files
    holding the same two arrays (`x`: (h,w,d,c) float32, `y`: (h,w,d,1) float32);
  * the transformation runs on the GPU (bts_channel_moments + bts_augment_crop / bts_augment_batch: one pass over the crop),
    the host only draws the 2c + 6 random numbers -- at ~70 ms per step a tf.data-style host pipeline would otherwise be the bottleneck;
  * the draws come from a seeded torch generator in a documented order (shift[c], scale[c], 3 crop offsets, 3 flips), so
    an epoch is reproducible; TF's stream cannot be.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import ops


def synthetic_batch(n, crop, in_ch=2, out_ch=3, seed=1234, dropout_rate=0.2, latent=128):
    """Synthetic BraTS-like batch of SURVEY 8(d), host tensors (x, y, dropout keep-mask, eps):
    x ~ N(0,1) zeroed outside a centred ellipsoid of semi-axes (56,60,52)/128 of the crop (skull-stripped, unit-variance
    channels: preprocess.py:116-124), labels = three nested spheres at a jittered centre -> one-hot minus background
    (train.py:41-43, preprocess.py:36), mask ~ Bernoulli(keep 1-rate) (encoder.py:39,71), eps ~ N(0,1) (vae.py:12).
    All draws from numpy.random.Generator(PCG64(seed)) in that order, so bench.py, the tests and the CPU baseline see the
    same volumes (the oracle carries an identical generator; tests/test_host_logic.py checks they agree)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    D, H, W = crop
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing='ij')
    semi = np.array([56.0, 60.0, 52.0]) * np.array(crop) / 128.0
    inside = (((zz - D / 2) / semi[0]) ** 2 + ((yy - H / 2) / semi[1]) ** 2 + ((xx - W / 2) / semi[2]) ** 2) <= 1.0
    x = rng.standard_normal((n, D, H, W, in_ch)).astype(np.float32) * inside[None, ..., None]
    y = np.zeros((n, D, H, W, out_ch), np.float32)
    radii = np.array([36.0, 24.0, 12.0]) * min(crop) / 128.0
    for b in range(n):
        centre = np.array([D / 2, H / 2, W / 2]) + rng.uniform(-0.15, 0.15, 3) * np.array(crop)
        r2 = (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2
        lab = np.zeros((D, H, W), np.int64)
        for k, r in enumerate(radii[:out_ch]):
            lab[r2 <= r * r] = k + 1
        for k in range(out_ch):
            y[b, ..., k] = (lab == k + 1)
    mask = (rng.random((n, D, H, W, in_ch)) >= dropout_rate).astype(np.float32)
    eps = rng.standard_normal((n, latent)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(mask), torch.from_numpy(eps)


class Draws(object):
    """the random numbers of one example (train.py:19-20,26,30-33)"""
    __slots__ = ('shift', 'scale', 'offsets', 'flips')

    def __init__(self, shift, scale, offsets, flips):
        self.shift, self.scale, self.offsets, self.flips = list(shift), list(scale), list(offsets), list(flips)

    @property
    def flip_mask(self):
        return (4 if self.flips[0] else 0) | (2 if self.flips[1] else 0) | (1 if self.flips[2] else 0)


def draw(gen, c, vol_size, crop_size):
    """shift ~ U(-0.1, 0.1)^c, scale ~ U(0.9, 1.1)^c, crop origin uniform over the valid range, flip_k = (u_k > 0.5)"""
    u = torch.rand(2 * c + 6, generator=gen, dtype=torch.float64).tolist()
    shift = [-0.1 + 0.2 * v for v in u[:c]]
    scale = [0.9 + 0.2 * v for v in u[c:2 * c]]
    offs = [min(int(u[2 * c + k] * (vol_size[k] - crop_size[k] + 1)), vol_size[k] - crop_size[k]) for k in range(3)]
    flips = [u[2 * c + 3 + k] > 0.5 for k in range(3)]
    return Draws(shift, scale, offs, flips)


def augment_example(x, y, crop_size, out_ch, draws):
    """device tensors x (h,w,d,c), y (h,w,d,1) -> (x_aug (crop,c), y_onehot (crop,out_ch)) per train.py:17-41"""
    _, var = ops.channel_moments(x)
    return ops.augment_crop(x, y, var, crop_size, draws.offsets, draws.flip_mask, draws.shift, draws.scale, out_ch)


class SpatialConfig(object):
    """spatial augmentation of a training example (bts_augment_spatial_batch): with probability `prob` the crop is rotated about
    axes 0, 1, 2 by angles uniform in +-rotate_deg[k] degrees (one number: the same bound for all three), zoomed by z uniform in
    zoom = (lo, hi) (z > 1 magnifies) and, with elastic_sigma > 0, deformed by a cubic B-spline free-form field whose control
    nodes, elastic_spacing voxels apart, are N(0, elastic_sigma^2) displacements in voxels.  Voxels from outside the volume carry
    `fill` (one number or one per channel) before the intensity shift / scale; labels there are background."""

    def __init__(self, prob, rotate_deg=(15.0, 15.0, 15.0), zoom=(0.9, 1.1), elastic_sigma=0.0, elastic_spacing=32, fill=0.0):
        deg = [float(rotate_deg)] * 3 if np.isscalar(rotate_deg) else [float(a) for a in rotate_deg]
        self.prob, self.rotate_deg, self.zoom = float(prob), tuple(deg), (float(zoom[0]), float(zoom[1]))
        self.elastic_sigma, self.elastic_spacing = float(elastic_sigma), int(elastic_spacing)
        self.fill = float(fill) if np.isscalar(fill) else [float(v) for v in fill]
        if not 0.0 <= self.prob <= 1.0 or len(deg) != 3 or self.elastic_sigma < 0 or self.elastic_spacing < 1:
            raise ValueError('SpatialConfig: prob in [0,1], three angles, elastic_sigma >= 0 and elastic_spacing >= 1 are needed')
        if not 0.0 < self.zoom[0] <= self.zoom[1]:
            raise ValueError('SpatialConfig: zoom must be 0 < lo <= hi, got %r' % (self.zoom,))

    def fill_of(self, c):
        return [self.fill] * c if isinstance(self.fill, float) else list(self.fill)


class SpatialDraw(object):
    """the spatial draws of one example: `on` (False: the plain copy), the 3x3 float64 `matrix` M, the control field `phi`
    (host float32 (G0,G1,G2,3), or None) and its `spacing`"""
    __slots__ = ('on', 'matrix', 'phi', 'spacing', 'angles', 'zoom')

    def __init__(self, on, matrix, phi, spacing, angles, zoom):
        self.on, self.matrix, self.phi, self.spacing, self.angles, self.zoom = bool(on), matrix, phi, int(spacing), angles, zoom


def spatial_matrix(angles, zoom):
    """M = R0(a0) R1(a1) R2(a2) / zoom in float64; R_k rotates about axis k by a_k radians (counter-clockwise in the plane of the two
    other axes taken in cyclic order)"""
    def rot(axis, a):
        i, j = (axis + 1) % 3, (axis + 2) % 3
        r = np.eye(3)
        r[i, i], r[i, j], r[j, i], r[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        return r
    return rot(0, angles[0]).dot(rot(1, angles[1])).dot(rot(2, angles[2])) / float(zoom)


def control_grid(crop_size, spacing):
    """nodes per axis of the free-form field of a crop: G_k = (T_k - 1) // spacing + 4"""
    return tuple((int(t) - 1) // int(spacing) + 4 for t in crop_size)


def draw_spatial(gen, cfg, crop_size):
    """The spatial draws of one example, taken right after draw().  For a given config the same number of values is consumed whatever
    they turn out to be (an example that stays untransformed still draws its angles, zoom and field), so the position in the stream
    never depends on a draw.  Order: torch.rand(5, float64) = [u_prob, u_a0, u_a1, u_a2, u_z] with on = (u_prob < prob),
    angle_k = (2 u_ak - 1) rotate_deg[k], z = lo + u_z (hi - lo); then, only if elastic_sigma > 0, torch.randn(G0, G1, G2, 3, float32)
    scaled by elastic_sigma (3 G0 G1 G2 standard normals, node-major, component last)."""
    u = torch.rand(5, generator=gen, dtype=torch.float64).tolist()
    phi = None
    if cfg.elastic_sigma > 0:
        phi = torch.randn(control_grid(crop_size, cfg.elastic_spacing) + (3,), generator=gen, dtype=torch.float32) * cfg.elastic_sigma
    on = u[0] < cfg.prob
    angles = [np.deg2rad((2.0 * u[1 + k] - 1.0) * cfg.rotate_deg[k]) for k in range(3)]
    zoom = cfg.zoom[0] + u[4] * (cfg.zoom[1] - cfg.zoom[0])
    if not on:
        return SpatialDraw(False, np.eye(3), None, cfg.elastic_spacing, angles, zoom)
    return SpatialDraw(True, spatial_matrix(angles, zoom), phi, cfg.elastic_spacing, angles, zoom)


class IntensityConfig(object):
    """intensity augmentation of a training example (bts_intensity_batch), the nnU-Net / batchgenerators set with its defaults:
    Gaussian noise of standard deviation s ~ U(noise_sigma) with probability noise_prob; Gaussian blur with probability blur_prob,
    then per channel with probability blur_channel_prob and sigma ~ U(blur_sigma); a brightness factor m ~ U(brightness) with
    probability brightness_prob; a contrast factor f from `contrast` with probability contrast_prob; a gamma from `gamma` with
    probability gamma_prob, applied to the negated image with probability gamma_invert_prob.  f and gamma follow batchgenerators'
    rule for a range (lo, hi): with lo < 1 and a side draw < 0.5 the value is U(lo, 1), otherwise U(max(lo, 1), hi).  s, sigma, m, f
    and gamma are drawn per channel."""

    def __init__(self, noise_prob=0.1, noise_sigma=(0.0, 0.1), blur_prob=0.2, blur_sigma=(0.5, 1.0), blur_channel_prob=0.5,
                 brightness_prob=0.15, brightness=(0.75, 1.25), contrast_prob=0.15, contrast=(0.75, 1.25), gamma_prob=0.3,
                 gamma=(0.7, 1.5), gamma_invert_prob=0.1):
        def pair(v, name, positive):
            try:
                lo, hi = (float(a) for a in v)
            except (TypeError, ValueError):
                raise ValueError('IntensityConfig: %s must be a pair (lo, hi), got %r' % (name, v))
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi and (lo > 0.0 if positive else lo >= 0.0)):
                raise ValueError('IntensityConfig: %s must be finite with %s lo <= hi, got %r' % (name, '0 <' if positive else '0 <=', v))
            return lo, hi
        self.noise_sigma = pair(noise_sigma, 'noise_sigma', False)
        self.blur_sigma = pair(blur_sigma, 'blur_sigma', True)
        self.brightness = pair(brightness, 'brightness', True)
        self.contrast = pair(contrast, 'contrast', True)
        self.gamma = pair(gamma, 'gamma', True)
        if int(4.0 * float(np.float32(self.blur_sigma[1])) + 0.5) > 16:
            raise ValueError('IntensityConfig: blur_sigma %r needs a radius int(4 sigma + 0.5) above 16' % (blur_sigma,))
        for name, v in (('noise_prob', noise_prob), ('blur_prob', blur_prob), ('blur_channel_prob', blur_channel_prob),
                        ('brightness_prob', brightness_prob), ('contrast_prob', contrast_prob), ('gamma_prob', gamma_prob),
                        ('gamma_invert_prob', gamma_invert_prob)):
            try:
                v = float(v)
            except (TypeError, ValueError):
                v = float('nan')
            if not 0.0 <= v <= 1.0:
                raise ValueError('IntensityConfig: %s must be a probability in [0, 1]' % name)
            setattr(self, name, v)


class IntensityDraw(object):
    """the intensity draws of one example: `params`, one (flags, s, sigma, m, f, gamma) per channel as ops.intensity_batch takes
    them (every number is kept, whatever its flag), and the Philox `key` (k0, k1) of its noise"""
    __slots__ = ('params', 'key')

    def __init__(self, params, key):
        self.params, self.key = params, key


def _two_sided(rng, side, u):
    """batchgenerators' draw of a contrast factor or gamma from rng = (lo, hi)"""
    lo, hi = rng
    if side < 0.5 and lo < 1.0:
        return lo + u * (1.0 - lo)
    lo = max(lo, 1.0)
    return lo + u * (hi - lo)


def draw_intensity(gen, cfg, c):
    """The intensity draws of one example of c channels, taken after draw() (and after draw_spatial() when there is one) on the same
    generator.  For a given config the same number of values is consumed whatever they turn out to be.  Order:
    torch.rand(6 + 8c, float64) = [u_noise, u_blur, u_brightness, u_contrast, u_gamma, u_invert], then for each channel
    [noise s, blur-channel, blur sigma, brightness m, contrast side, contrast value, gamma side, gamma value];
    then torch.randint(0, 2**32, (2,), int64) = the noise key (k0, k1).
    A stage is on when its u < its probability (blur: and the channel's u < blur_channel_prob; invert: u_invert <
    gamma_invert_prob, with gamma on); a range draw is lo + u (hi - lo), f and gamma by the two-sided rule of IntensityConfig."""
    u = torch.rand(6 + 8 * c, generator=gen, dtype=torch.float64).tolist()
    key = torch.randint(0, 2 ** 32, (2,), generator=gen, dtype=torch.int64).tolist()
    lin = lambda rng, v: rng[0] + v * (rng[1] - rng[0])      # noqa: E731
    noise, blur, bright = u[0] < cfg.noise_prob, u[1] < cfg.blur_prob, u[2] < cfg.brightness_prob
    contrast, gamma = u[3] < cfg.contrast_prob, u[4] < cfg.gamma_prob
    invert = gamma and u[5] < cfg.gamma_invert_prob
    params = []
    for j in range(c):
        v = u[6 + 8 * j:14 + 8 * j]
        flags = ((ops.INTENSITY_NOISE if noise else 0) | (ops.INTENSITY_BLUR if blur and v[1] < cfg.blur_channel_prob else 0) |
                 (ops.INTENSITY_BRIGHT if bright else 0) | (ops.INTENSITY_CONTRAST if contrast else 0) |
                 (ops.INTENSITY_GAMMA if gamma else 0) | (ops.INTENSITY_INVERT if invert else 0))
        params.append((flags, lin(cfg.noise_sigma, v[0]), lin(cfg.blur_sigma, v[2]), lin(cfg.brightness, v[3]),
                       _two_sided(cfg.contrast, v[4], v[5]), _two_sided(cfg.gamma, v[6], v[7])))
    return IntensityDraw(params, (int(key[0]), int(key[1])))


class ForegroundConfig(object):
    """foreground oversampling of the training crops (the nnU-Net / batchgenerators recipe): with probability `prob`, in (0, 1], an
    example's crop is centred on a voxel drawn from its class-location table (ops.class_locations: at most `samples` evenly spaced
    voxels per class, built on the device once per file) instead of being placed uniformly.  classes: the classes c (label c + 1) to
    choose from, a subset of range(out_ch); None: all.  A class without a voxel in the example is never chosen, and an example without
    any voxel of the allowed classes keeps its uniform crop."""

    def __init__(self, prob, samples=10000, classes=None):
        try:
            self.prob = float(prob)
        except (TypeError, ValueError):
            self.prob = float('nan')
        if not 0.0 < self.prob <= 1.0:
            raise ValueError('ForegroundConfig: prob must be in (0, 1], got %r' % (prob,))
        if isinstance(samples, bool) or not isinstance(samples, (int, np.integer)) or not 1 <= int(samples) < 2 ** 31:
            raise ValueError('ForegroundConfig: samples must be an integer >= 1, got %r' % (samples,))
        self.samples = int(samples)
        if classes is not None:
            try:
                cl = [int(c) for c in classes]
                ok = len(cl) > 0 and all(float(c) == int(c) for c in classes)
            except (TypeError, ValueError):
                cl, ok = [], False
            if not ok or len(set(cl)) != len(cl) or min(cl) < 0 or max(cl) >= ops.CLASS_LOCATIONS_MAX_CLASSES:
                raise ValueError('ForegroundConfig: classes must be distinct integers in range(out_ch), got %r' % (classes,))
            classes = tuple(sorted(cl))
        self.classes = classes

    def allowed(self, out_ch):
        """the ascending classes to choose from for `out_ch` output classes; ValueError for a class outside range(out_ch)"""
        if self.classes is None:
            return list(range(int(out_ch)))
        if self.classes[-1] >= int(out_ch):
            raise ValueError('ForegroundConfig: classes %r must lie in range(out_ch) = range(%d)' % (self.classes, int(out_ch)))
        return list(self.classes)


def draw_foreground(gen, cfg, counts, loc, vol_size, crop_size, offsets):
    """The foreground draw of one example, taken right after draw() (and before draw_spatial()) on the same generator -> its three crop
    offsets.  counts: the out_ch voxel counts n_c, loc: the (out_ch, K) table of ops.class_locations, both on the host; offsets: what
    draw() placed.  The same three values are consumed in every branch, so the position in the stream never depends on a draw.  Order:
    torch.rand(3, float64) = [u_on, u_class, u_voxel] with on = (u_on < prob).  present = the ascending allowed classes with n_c > 0; if
    on and present is not empty: c = present[min(int(u_class len(present)), len(present) - 1)], j = min(int(u_voxel m_c), m_c - 1) with
    m_c = ceil(n_c / max(1, ceil(n_c / K))) the entries the table holds for c, p = the voxel of linear index loc[c][j], and
    offset_k = min(max(p_k - crop_k // 2, 0), vol_k - crop_k).  Otherwise `offsets` is returned as it came.

    Where the voxel ends up: p sits at index crop_k // 2 of the crop unless an offset was clamped at a face of the volume, and then it
    sits nearer that face.  Flips act on the crop's own index and keep it inside.  The spatial transform (bts_augment_spatial_batch) fixes
    the crop's geometric centre (crop_k - 1) / 2, so an unclamped p lies half a voxel (even crop_k) or no distance (odd crop_k) from the
    fixed point and a rotation or zoom moves it by a fraction of a voxel; a clamped p can lie up to crop_k / 2 from the fixed point, and a
    rotation, a zoom above 1 or the elastic field can then move it out of the crop."""
    u = torch.rand(3, generator=gen, dtype=torch.float64).tolist()
    k = len(loc[0])
    present = [c for c in cfg.allowed(len(counts)) if int(counts[c]) > 0]
    if not (u[0] < cfg.prob and present):
        return list(offsets)
    c = present[min(int(u[1] * len(present)), len(present) - 1)]
    n = int(counts[c])
    stride = max(1, -(-n // k))
    m = -(-n // stride)
    p = int(loc[c][min(int(u[2] * m), m - 1)])
    pk = (p // (vol_size[1] * vol_size[2]), (p // vol_size[2]) % vol_size[1], p % vol_size[2])
    return [min(max(pk[a] - crop_size[a] // 2, 0), vol_size[a] - crop_size[a]) for a in range(3)]


TARGETS = ('labels', 'regions')


class _Dataset(object):
    """re-iterable epoch of (x, y) device batches.  Data parallel: every rank draws the SAME permutation from
    the shared shuffle generator and keeps positions rank, rank+world, ... of it, truncated to len // world examples so
    that all ranks run the same number of steps (the per-step exchanges would deadlock otherwise); the augmentation draws
    come from a second, per-rank generator.

    resident_bytes / workers (both 0: the per-example path as it always was).  Otherwise a batch is one bts_augment_batch launch
    over the examples' device tensors, and
      * an example whose x + y bytes still fit under `resident_bytes` stays on the device once read, with its per-channel variance (a
        property of the file: the same fixed-order fp64 result every time); the others are streamed -- read, uploaded, moments, used,
        dropped.  An epoch whose examples are all resident reads no file and uploads no volume: only the draws and the pointer /
        offset tables leave the host.  A rank keeps what it visits;
      * with workers > 0 host threads read the epoch's next non-resident examples ahead, consumed in visiting order.
    All draws stay on the iterating thread in visiting order, so for a given seed the batches are bit-identical whatever the two
    arguments are; residency is not state (state_dict is the two generators).

    spatial (a SpatialConfig, or None: nothing below happens and not one extra value is drawn): draw_spatial() follows every draw(), on
    the same generator, and both paths go through bts_augment_spatial_batch (the per-example path with N = 1), so the batches are
    still the same on either path and the state is still the two generators.

    intensity (an IntensityConfig, or None: nothing below happens and not one extra value is drawn): draw_intensity() follows draw()
    and draw_spatial(), on the same generator, and both paths run bts_intensity_batch on what the augment launch returned (the
    per-example path with N = 1, channels last).  Its result depends neither on N nor on the layout, so the batches are again the
    same on either path.

    targets ('labels': nothing below happens): with 'regions' the label batch goes through bts_region_targets right after the augment
    launch (before the intensity stage, which does not touch y), so y holds the nested BraTS regions (WT, TC, ET) in place of the
    disjoint one-hot labels.  No value is drawn for it: x and the generator states are those of 'labels'.

    foreground (a ForegroundConfig, or None: nothing below happens and not one extra value is drawn): draw_foreground() follows every
    draw(), before draw_spatial(), on the same generator, and replaces the crop offsets; nothing else of the draws changes, so spatial,
    intensity and targets compose as they are.  It reads the example's class-location table (ops.class_locations on the labels, copied to
    the host once), which is built where the variance is and kept next to (x, y, var): a property of the file, never rebuilt for a
    resident example, rebuilt per read for a streamed one.  The host tables do not count against resident_bytes."""

    channels_first = False

    def __init__(self, files, batch_size, prepro_size, crop_size, out_ch, shuffle, seed, device, rank=0, world=1,
                 resident_bytes=0, workers=0, spatial=None, intensity=None, targets='labels', foreground=None):
        if targets not in TARGETS:
            raise ValueError('unknown targets %r: one of %s' % (targets, TARGETS))
        if targets == 'regions' and int(out_ch) != 3:
            raise ValueError("targets='regions' are the three BraTS regions WT, TC, ET: out_ch must be 3, got %r" % (out_ch,))
        self.targets = targets
        self.files, self.batch_size, self.prepro_size = files, int(batch_size), tuple(prepro_size)
        self.crop_size, self.out_ch, self.shuffle = tuple(crop_size), int(out_ch), shuffle
        self.rank, self.world = int(rank), max(1, int(world))
        self.order_gen = torch.Generator().manual_seed(seed)
        self.gen = torch.Generator().manual_seed(seed + 7919 * (self.rank + 1))
        self.device = device
        self.resident_bytes, self.workers = max(0, int(resident_bytes)), max(0, int(workers))
        # file index -> (x, y, var) on the device and the host class-location table (None without foreground); bytes of their x + y
        self._resident, self._resident_used = {}, 0
        self.spatial = spatial
        self.intensity = intensity
        self.foreground = foreground
        if foreground is not None:
            foreground.allowed(self.out_ch)                     # (a class outside range(out_ch) is refused here, not at the first batch)

    def _per_rank(self):
        return len(self.files) // self.world if self.world > 1 else len(self.files)

    def __len__(self):
        return (self._per_rank() + self.batch_size - 1) // self.batch_size

    def state_dict(self):
        """generator states (uint8 tensors): persisted by train.save_checkpoint so a resumed run draws what the
        uninterrupted one would have"""
        return {'order_gen': self.order_gen.get_state().clone(), 'gen': self.gen.get_state().clone()}

    def load_state_dict(self, st):
        self.order_gen.set_state(st['order_gen'].to(torch.uint8).cpu())
        self.gen.set_state(st['gen'].to(torch.uint8).cpu())

    def _order(self):
        order = list(range(len(self.files)))
        if self.shuffle:                                                   # train.py:60-61 (buffer = whole file list)
            order = torch.randperm(len(order), generator=self.order_gen).tolist()
        if self.world > 1:
            order = order[self.rank::self.world][:self._per_rank()]
        return order

    def _read(self, i):
        """host side of one example -> (x (h,w,d,c), y (h,w,d,1)) float32 arrays"""
        h, w, d, c = self.prepro_size
        z = np.load(self.files[i])
        return (np.ascontiguousarray(z['x'], dtype=np.float32).reshape(h, w, d, c),
                np.ascontiguousarray(z['y'], dtype=np.float32).reshape(h, w, d, 1))

    def _table(self, y):
        """the class-location table of an example's device labels, copied to the host: (counts, loc); None without foreground oversampling"""
        if self.foreground is None:
            return None
        counts, loc = ops.class_locations(y, self.out_ch, self.foreground.samples)
        return counts.cpu().tolist(), loc.cpu().numpy()

    def _draw(self, table):
        """draw() of one example, its crop moved by draw_foreground() where that is on"""
        h, w, d, c = self.prepro_size
        dr = draw(self.gen, c, (h, w, d), self.crop_size)
        if self.foreground is not None:
            dr.offsets = draw_foreground(self.gen, self.foreground, table[0], table[1], (h, w, d), self.crop_size, dr.offsets)
        return dr

    def __iter__(self):
        if self.resident_bytes == 0 and self.workers == 0:
            return self._iter_per_example()
        return self._iter_batched()

    def _iter_per_example(self):
        order = self._order()
        h, w, d, c = self.prepro_size
        xs, ys = [], []
        for i in order:
            xh, yh = self._read(i)
            x, y = torch.from_numpy(xh).to(self.device), torch.from_numpy(yh).to(self.device)
            dr = self._draw(self._table(y))
            if self.spatial is None:
                xa, ya = augment_example(x, y, self.crop_size, self.out_ch, dr)
            else:
                sd = draw_spatial(self.gen, self.spatial, self.crop_size)
                xa, ya = self._augment_spatial([(x, y, ops.channel_moments(x)[1])], [dr], [sd], False)
                xa, ya = xa[0], ya[0]
            if self.targets == 'regions':
                ops.region_targets(ya)
            if self.intensity is not None:
                idr = draw_intensity(self.gen, self.intensity, c)
                ops.intensity_batch(xa.unsqueeze(0), [idr.params], [idr.key], False)
            xs.append(xa)
            ys.append(ya)
            if len(xs) == self.batch_size:
                yield self._emit(xs, ys)
                xs, ys = [], []
        if xs:
            yield self._emit(xs, ys)

    def _emit(self, xs, ys):
        return torch.stack(xs), torch.stack(ys)

    def _host_examples(self, todo):
        """the examples of `todo` in order; with workers > 0 a bounded number of them is read ahead by host threads"""
        if self.workers <= 0:
            for i in todo:
                yield self._read(i)
            return
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            pending, nxt = [], 0
            for _ in todo:
                while nxt < len(todo) and len(pending) < self.workers + 1:
                    pending.append(pool.submit(self._read, todo[nxt]))
                    nxt += 1
                yield pending.pop(0).result()

    def _iter_batched(self):
        order = self._order()
        h, w, d, c = self.prepro_size
        # an index occurs once per epoch and the resident set only grows: what this epoch has to read is known now
        host = self._host_examples([i for i in order if i not in self._resident])
        batch, draws, sdraws, idraws = [], [], [], []
        for i in order:
            ex = self._resident.get(i)
            if ex is None:
                xh, yh = next(host)
                # (uploads run on the current stream, like everything that reads them: a yielded batch is ordered behind them)
                x, y = torch.from_numpy(xh).to(self.device), torch.from_numpy(yh).to(self.device)
                ex = (x, y, ops.channel_moments(x)[1], self._table(y))
                nbytes = (x.numel() + y.numel()) * 4
                if self._resident_used + nbytes <= self.resident_bytes:
                    self._resident[i] = ex
                    self._resident_used += nbytes
            batch.append(ex)
            draws.append(self._draw(ex[3]))
            if self.spatial is not None:
                sdraws.append(draw_spatial(self.gen, self.spatial, self.crop_size))
            if self.intensity is not None:
                idraws.append(draw_intensity(self.gen, self.intensity, c))
            if len(batch) == self.batch_size:
                yield self._intensity(self._augment(batch, draws, sdraws), idraws)
                batch, draws, sdraws, idraws = [], [], [], []
        if batch:
            yield self._intensity(self._augment(batch, draws, sdraws), idraws)

    def _intensity(self, xy, idraws):
        if self.intensity is not None:
            ops.intensity_batch(xy[0], [d.params for d in idraws], [d.key for d in idraws], self.channels_first)
        return xy

    def _augment_spatial(self, batch, draws, sdraws, channels_first):
        # (the fields are uploaded on the current stream, ahead of the launch that reads them)
        phis = [None if sd.phi is None else sd.phi.to(self.device) for sd in sdraws]
        c = self.prepro_size[3]
        return ops.augment_spatial_batch([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], self.crop_size,
                                         [dr.offsets for dr in draws], [dr.flip_mask for dr in draws], [dr.shift for dr in draws],
                                         [dr.scale for dr in draws], self.out_ch, [sd.on for sd in sdraws],
                                         [sd.matrix.reshape(-1).tolist() for sd in sdraws], phis, [sd.spacing for sd in sdraws],
                                         [self.spatial.fill_of(c)] * len(batch), channels_first)

    def _augment(self, batch, draws, sdraws=()):
        if self.spatial is not None:
            xy = self._augment_spatial(batch, draws, sdraws, self.channels_first)
        else:
            xy = ops.augment_batch([b[0] for b in batch], [b[1] for b in batch], [b[2] for b in batch], self.crop_size,
                                   [dr.offsets for dr in draws], [dr.flip_mask for dr in draws], [dr.shift for dr in draws],
                                   [dr.scale for dr in draws], self.out_ch, self.channels_first)
        if self.targets == 'regions':
            ops.region_targets(xy[1], self.channels_first)
        return xy


class _ChannelsFirstDataset(_Dataset):
    """public NCDHW batches (train.py:45-47 transposes each example); the engine's layers re-lay them out on entry"""

    channels_first = True

    def _emit(self, xs, ys):
        return torch.stack(xs).permute(0, 4, 1, 2, 3).contiguous(), torch.stack(ys).permute(0, 4, 1, 2, 3).contiguous()


def prepare_dataset(loc, batch_size, prepro_size, crop_size, out_ch, shuffle=True, data_format='channels_last', seed=0,
                    device=None, rank=None, world=None, resident_bytes=0, workers=0, spatial=None, intensity=None,
                    targets='labels', foreground=None):
    """-> (re-iterable dataset of (x, y) device batches, number of examples)   [train.py:12-64]
    rank / world default to the process group's (one shard of the examples per rank, see _Dataset).
    resident_bytes: budget of example bytes kept on the device after their first read; workers: host threads reading ahead
    (see _Dataset; the batches do not depend on either).  spatial: a SpatialConfig (rotation, zoom and elastic deformation of the
    crops, on the device in the same launch) or None, which leaves every draw and every batch as it was.  intensity: an
    IntensityConfig (noise, blur, brightness, contrast and gamma on the augmented batch, on the device) or None, likewise.
    targets: 'labels' (y = one-hot labels minus the background, as the reference trains) or 'regions' (y = the nested BraTS regions
    WT, TC, ET: bts_region_targets on the label batch; out_ch must be 3); x and every draw are the same in both.  foreground: a
    ForegroundConfig (a share of the crops centred on a foreground voxel of the example, from a class-location table built on the device
    once per file) or None, which leaves every draw and every batch as it was."""
    if data_format not in ('channels_last', 'channels_first'):
        raise ValueError('unknown data_format %r' % (data_format,))
    from . import parallel
    rank = parallel.rank() if rank is None else rank
    world = parallel.world() if world is None else world
    files = sorted(os.path.join(loc, f) for f in os.listdir(loc) if f.endswith('.npz'))
    dev = device if device is not None else torch.device('cuda', torch.cuda.current_device())
    cls = _Dataset if data_format == 'channels_last' else _ChannelsFirstDataset
    return cls(files, batch_size, prepro_size, crop_size, out_ch, shuffle, seed, dev, rank, world, resident_bytes, workers, spatial,
               intensity, targets, foreground), len(files)
