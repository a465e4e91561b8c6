"""-m gpu: csrc/casenorm.hip (bts_case_norm) against the numpy float64 restatement tests/casenorm_ref.py, and the per-case normalisation
through bts_amd.preprocess, bts_amd.infer and `python -m bts_amd.test`.  No tolerance is taken from the kernels under test:

  n, lo, hi                             equal (==): integer counts; the order statistics are exact and the interpolation is three fp64
                                        operations, each rounded once on both sides
  mean where every clamped value is     bit-equal: integer terms whose total stays below 2^53 add exactly in any order, and the
  an integer                            division is rounded once
  mean elsewhere                        |sum_dev - sum_ref| <= n 2^-53 sum|v| (a reordered fp64 sum).  The device returns the quotient,
                                        so the bound is carried to it: divided by n, plus one rounding (2^-53 |mean|) per side
  std                                   likewise on the centred squares with 2n: |q_dev - q_ref| <= 2n 2^-53 q, q_dev = n std_dev^2; the
                                        division, the square root and squaring it again here add 4 roundings of q
  output                                bit-equal to float32((clamp(x) - mean) / std) in numpy float64 with the statistics the DEVICE
                                        returned, +0.0 outside the mask
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import casenorm_ref as CR  # noqa: E402
import guard_alloc  # noqa: E402
import segment_ref as S  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
CLIPS = [None, (0.5, 99.5), (0.0, 100.0), (25.0, 75.0), (50.0, 50.0)]
SHAPES = [(5, 7, 9), (6, 10, 33), (9, 17, 21), (16, 16, 16), 'big']


def dev():
    return torch.device('cuda', 0)


def big_shape():
    """about 2 10^5 voxels, from the implementation's own grid cap: a sweep of the capped grid covers cap x 256 voxels, so the
    grid-stride loop runs a second time for some workgroups and the finalize adds `cap` (> 64) partials"""
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    cap = lib()._bts_case_norm_blocks()
    assert cap > 64
    t2 = (cap * 256) // (64 * 64) + 8
    t2 -= t2 % 8
    assert 64 * 64 * t2 > cap * 256
    return (64, 64, t2)


def make_volume(shape, c, values, seed):
    """values 'int': integer-valued gamma intensities >= 1; 'frac': fractional values of both signs.  40 % of the voxels are zero in
    every channel (background), and single channels are zero here and there"""
    rng = np.random.default_rng(seed)
    if values == 'int':
        x = np.floor(rng.gamma(2.0, 150.0, size=shape + (c,))) + 1.0
    else:
        x = rng.standard_normal(shape + (c,)) * 50.0 + 20.0
    x[rng.random(shape + (c,)) < 0.05] = 0.0
    x[rng.random(shape) < 0.4] = 0.0
    return x.astype(np.float32)


def explicit_mask(shape, seed):
    """leaves out about half of the voxels, positive ones among them, and takes in background; 'non-zero' has several values"""
    rng = np.random.default_rng(seed + 1000)
    return (rng.random(shape) < 0.5).astype(np.float32) * rng.choice(np.array([1.0, 2.0, -1.0, 0.25], dtype=np.float32), size=shape)


def run(x, mask=None, clip=None, y=None):
    from bts_amd import ops
    xg = x if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(dev())
    mg = None if mask is None else (mask if isinstance(mask, torch.Tensor) else torch.from_numpy(mask).to(dev()))
    got = ops.case_norm(xg, mg, clip, y=y)
    return [g.cpu().numpy() for g in got]


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def check_against_reference(x, mask, clip, who):
    out, st = run(x, mask, clip)
    ref_out, ref_st, sums = CR.case_norm(x, mask, clip)
    inside = CR.inside_mask(x, mask)
    c = x.shape[-1]
    n = int(ref_st[0])
    print('%s: n %d of %d' % (who, n, inside.size))
    assert st[0] == n, who
    for ch in range(c):
        mean, std, lo, hi = st[1 + 4 * ch:5 + 4 * ch]
        rmean, rstd, rlo, rhi = ref_st[1 + 4 * ch:5 + 4 * ch]
        assert lo == rlo and hi == rhi, (who, ch, lo, rlo, hi, rhi)
        if n == 0:
            assert mean == 0 and std == 0
            continue
        v = CR.clamp(x[..., ch][inside].astype(np.float64), rlo, rhi)
        total, sq, sabs = sums[ch]
        if np.array_equal(v, np.floor(v)) and sabs < 2.0 ** 53:
            assert mean == rmean, (who, ch, mean, rmean)
        else:
            err, bound = abs(mean - rmean), U * sabs + 2 * U * abs(rmean)
            print('  channel %d: |mean - ref| %.3e, bound %.3e' % (ch, err, bound))
            assert err <= bound, (who, ch)
        q, bound = std * std * n, 2 * n * U * sq + 4 * U * sq
        print('  channel %d: |q - ref| %.3e, bound %.3e' % (ch, abs(q - sq), bound))
        assert abs(q - sq) <= bound, (who, ch, std, rstd)
    want = CR.apply_stats(x, inside, st)
    assert out.dtype == np.float32 and bits(out) == bits(want), who
    assert bits(out[~inside]) == bytes(out[~inside].nbytes), who
    return out, st


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('values', ['int', 'frac'])
@pytest.mark.parametrize('clip', CLIPS, ids=lambda c: 'none' if c is None else '%g-%g' % c)
@pytest.mark.parametrize('c', [1, 2, 3, 4, 16])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: s if isinstance(s, str) else 'x'.join(map(str, s)))
def test_against_the_reference(shape, c, clip, values):
    shape = big_shape() if shape == 'big' else shape
    x = make_volume(shape, c, values, 7 * c + shape[2])
    for masked in (False, True):
        mask = explicit_mask(shape, c + shape[1]) if masked else None
        out, st = check_against_reference(x, mask, clip, '%s C=%d %s %s clip %s' % (shape, c, values, 'mask' if masked else 'derived', clip))
        if clip == (50.0, 50.0):
            # lo == hi = w: n copies of w, 25 significant bits, add exactly (n < 2^28), so mean == w and the deviation is 0
            assert not out.any()


# ---- edges -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('clip', [None, (0.5, 99.5)])
def test_empty_mask_and_tiny_counts(clip):
    x = make_volume((5, 7, 9), 3, 'frac', 3)
    out, st = check_against_reference(x, np.zeros((5, 7, 9), dtype=np.float32), clip, 'all-zero mask')
    assert st.tolist() == [0.0] * 13 and bits(out) == bytes(out.nbytes)
    out, st = check_against_reference(np.zeros((4, 4, 4, 2), dtype=np.float32), None, clip, 'all-zero volume')
    assert st.tolist() == [0.0] * 9 and bits(out) == bytes(out.nbytes)
    for n in (1, 2):
        m = np.zeros((5, 7, 9), dtype=np.float32)
        m.reshape(-1)[[17, 200][:n]] = 1.0
        out, st = check_against_reference(x, m, clip, 'n = %d' % n)
        assert st[0] == n
        if n == 1:
            assert not out.any()


@pytest.mark.parametrize('clip', [None, (0.0, 100.0), (10.0, 90.0)])
def test_constant_channel_ties_and_signed_zeros(clip):
    rng = np.random.default_rng(5)
    x = make_volume((6, 10, 33), 3, 'int', 9)
    inside = CR.inside_mask(x)
    x[..., 1] = np.where(inside, np.float32(37.0), np.float32(0.0))               # constant inside: zeros in this channel only
    out, st = check_against_reference(x, None, clip, 'constant channel')
    assert st[1 + 4 + 1] == 0 and not out[..., 1].any() and out[..., 0].any() and out[..., 2].any()
    t = rng.choice(np.array([1.0, 2.0, 2.0, 2.0, 5.0], dtype=np.float32), size=(9, 17, 21, 2))        # heavy ties
    check_against_reference(t, None, clip, 'ties')
    z = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.5, -2.5], dtype=np.float32), size=(9, 17, 21, 2))  # -0.0 next to +0.0
    z[..., 1] += np.float32(1.0)                                                   # a mean of exactly 0 would leave the sign of 0 open
    m = (rng.random((9, 17, 21)) < 0.8).astype(np.float32)
    check_against_reference(z, m, clip, 'signed zeros')


def test_clip_0_100_is_clip_none():
    for c in (1, 2, 3, 4):
        x = make_volume((9, 17, 21), c, 'frac', 40 + c)
        a, sa = run(x, None, None)
        b, sb = run(x, None, (0.0, 100.0))
        assert bits(a) == bits(b)
        assert bits(sa.reshape(-1)[[0] + [i for ch in range(c) for i in (1 + 4 * ch, 2 + 4 * ch)]]) == \
            bits(sb.reshape(-1)[[0] + [i for ch in range(c) for i in (1 + 4 * ch, 2 + 4 * ch)]])
        inside = CR.inside_mask(x)
        for ch in range(c):
            assert sb[3 + 4 * ch] == x[..., ch][inside].min() and sb[4 + 4 * ch] == x[..., ch][inside].max()


@pytest.mark.parametrize('clip', [(0.5, 99.5), (10.0, 90.0), (37.0, 63.0), (50.0, 50.0)])
def test_every_digit_pass_decides_a_selection(clip):
    """eight channels: in channel (byte b, sign s) the values differ from one base pattern in byte b of the key alone, so the pass of
    that digit alone separates them (the other three passes see one occupied bin)"""
    rng = np.random.default_rng(17)
    shape = (5, 7, 9)
    nv = int(np.prod(shape))
    base = np.uint32(0x42F6E979)                                   # 123.456...
    chans = []
    for sign in (0, 1):
        for byte in range(4):
            digit = rng.integers(0, 0x7F if byte == 3 else 256, size=nv).astype(np.uint32)       # the top byte: finite exponents only
            keep = np.uint32(~(0xFF << (8 * byte)) & 0xFFFFFFFF) if byte < 3 else np.uint32(0x00FFFFFF)
            u = (base & keep) | (digit << np.uint32(8 * byte)) | np.uint32(sign << 31)
            chans.append(u.view(np.float32))
    x = np.stack(chans, axis=-1).reshape(shape + (8,)).astype(np.float32)
    assert np.isfinite(x).all() and (x[..., :4] > 0).all() and (x[..., 4:] < 0).all()
    for ch in range(8):
        u = x[..., ch].reshape(-1).view(np.uint32)
        assert len(np.unique(u)) > 40 and len(np.unique(u & ~np.uint32(0xFF << (8 * (ch % 4))))) == 1
    check_against_reference(x, None, clip, 'digit passes')


# ---- windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', [2, 3, 4])
@pytest.mark.parametrize('clip', [None, (0.5, 99.5)])
def test_a_strided_window_equals_its_contiguous_copy(c, clip):
    from bts_amd import ops
    rng = np.random.default_rng(c)
    parent = torch.from_numpy(make_volume((9, 12, 11), c, 'frac', 60 + c)).to(dev())
    labels = torch.from_numpy(rng.integers(0, 6, size=(9, 12, 11, 1)).astype(np.float32)).to(dev())
    pm = torch.from_numpy(explicit_mask((9, 12, 11), 61)).to(dev())
    cut = (slice(1, 8), slice(3, 12), slice(3, 10))                # an odd origin; T2 = 7: T2 C is 14, 21, 28
    xw, yw, mw = parent[cut], labels[cut], pm[cut]
    assert not xw.is_contiguous() and ((7 * c) % 4 != 0 or c == 4)
    for mask_w, mask_c in ((None, None), (mw, mw.contiguous())):
        a, ya, sa = ops.case_norm(xw, mask_w, clip, y=yw)
        b, yb, sb = ops.case_norm(xw.contiguous(), mask_c, clip, y=yw.contiguous())
        assert a.is_contiguous() and tuple(a.shape) == (7, 9, 7, c) and tuple(ya.shape) == (7, 9, 7, 1)
        assert torch.equal(a, b) and bits(a.cpu().numpy()) == bits(b.cpu().numpy())
        assert bits(sa.cpu().numpy()) == bits(sb.cpu().numpy()) and torch.equal(ya, yb)
        lab = yw.cpu().numpy()
        assert np.array_equal(ya.cpu().numpy(), np.where(lab >= 4, np.float32(3.0), lab)) and ya.max() == 3.0
        check_against_reference(xw.cpu().numpy(), None if mask_w is None else mask_w.cpu().numpy(), clip, 'window C=%d' % c)
    out = torch.full((7, 9, 7, c), -777.0, device=dev())
    got = ops.case_norm(xw, None, clip, out=out)
    assert got[0] is out and torch.equal(out, ops.case_norm(xw, None, clip)[0])
    with pytest.raises(ValueError):
        ops.case_norm(parent.permute(1, 0, 2, 3))                  # no spatial slice
    with pytest.raises(ValueError):
        ops.case_norm(parent[..., :1])                             # a channel slice
    with pytest.raises(ValueError):
        ops.case_norm(parent, pm[:8])


# ---- guard bands, poison, determinism -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c,clip,masked', [(2, (0.5, 99.5), False), (3, (25.0, 75.0), True), (4, None, False), (16, (0.5, 99.5), True)])
def test_guard_bands_poison_and_repeatability(monkeypatch, c, clip, masked):
    """outputs, statistics and the workspace, sized EXACTLY by bts_case_norm_workspace, between guard bands: the bands stay intact, two
    runs give the same bits, and a buffer pre-filled with 0x00 gives the bits of one pre-filled with 0xFF (nothing unwritten is read)"""
    import bts_amd  # noqa: F401
    from bts_amd import ops
    x = torch.from_numpy(make_volume((9, 17, 21), c, 'frac', 80 + c)).to(dev())
    y = torch.from_numpy(np.random.default_rng(c).integers(0, 6, size=(9, 17, 21, 1)).astype(np.float32)).to(dev())
    m = torch.from_numpy(explicit_mask((9, 17, 21), 81)).to(dev()) if masked else None
    results = {}
    for fill in (0x00, 0xFF, guard_alloc.FILL):
        with monkeypatch.context() as mp:
            g = guard_alloc.install(mp, fill)
            runs = [[t.cpu().numpy().copy() for t in ops.case_norm(x, m, clip, y=y)] for _ in range(2)]
            assert g.check() >= 8
        for a, b in zip(*runs):
            assert bits(a) == bits(b)
        results[fill] = runs[0]
    for other in (0xFF, guard_alloc.FILL):
        for a, b in zip(results[0x00], results[other]):
            assert bits(a) == bits(b)
    assert np.isfinite(results[0x00][0]).all() and results[0x00][0].any()


@pytest.mark.parametrize('clip', [None, (0.5, 99.5), (0.0, 100.0), (25.0, 75.0)])
def test_scaling_the_scan_by_four_leaves_the_output(clip):
    for shape, c in (((5, 7, 9), 1), ((6, 10, 33), 2), ((9, 17, 21), 4), ((3, 5, 7), 3)):
        for values in ('int', 'frac'):
            x = make_volume(shape, c, values, 90 + c)
            a, sa = run(x, None, clip)
            b, sb = run(4.0 * x, None, clip)
            assert bits(a) == bits(b) and a.any()
            assert sa[0] == sb[0] and np.array_equal(sb[1:], 4.0 * sa[1:])


# ---- bts_amd.preprocess --------------------------------------------------------------------------------------------------------------
def write_cases(folder, count, vol, seed):
    from bts_amd import nifti
    for k in range(count):
        case = os.path.join(folder, 'case%d' % k)
        os.makedirs(case)
        x = S.scan_like(vol, seed + k) * np.float32(1.0 + 2.0 * k)               # every case on its own intensity scale
        lab = np.array([0, 1, 2, 4], dtype=np.int16)[np.random.default_rng(seed + k).integers(0, 4, size=vol)]
        nifti.save(os.path.join(case, 'c_t1ce.nii.gz'), x[..., 0], np.eye(4))
        nifti.save(os.path.join(case, 'c_flair.nii'), x[..., 1], np.eye(4))
        nifti.save(os.path.join(case, 'c_seg.nii.gz'), lab, np.eye(4))


@pytest.mark.parametrize('clip', [None, (0.5, 99.5)])
def test_preprocess_in_case_mode(tmp_path, clip):
    import bts_amd  # noqa: F401
    from bts_amd import ops, preprocess
    src, out = str(tmp_path / 'in'), str(tmp_path / 'out')
    write_cases(src, 3, (12, 14, 10), 31)
    r = preprocess.preprocess([src], ['t1ce', 'flair'], 'seg', out, norm='case', clip=clip)
    assert r['n_train'] == 3 and r['n_val'] == 0 and r['mean'].reshape(-1).tolist() == [0.0, 0.0] and r['std'].reshape(-1).tolist() == [1.0, 1.0]
    spec = preprocess.load_norm(os.path.join(out, 'prepro.npy'))
    assert spec.mode == 'case' and spec.clip == clip
    size, mean, std = preprocess.load_prepro(os.path.join(out, 'prepro.npy'))
    assert mean.tolist() == [0.0, 0.0] and std.tolist() == [1.0, 1.0]
    xs, ys, size2 = preprocess.create_dataset([src], ['t1ce', 'flair'], 'seg')
    assert size == (size2['h'], size2['w'], size2['d'], 2) and not xs[0].is_contiguous()
    for i, (xv, yv) in enumerate(zip(xs, ys), 1):
        z = np.load(os.path.join(out, 'train', '%d.npz' % i))
        xn, yn, st = ops.case_norm(xv, None, clip, y=yv)
        assert bits(z['x']) == bits(xn.cpu().numpy()) and bits(z['y']) == bits(yn.cpu().numpy())
        assert z['x'].shape == size and set(np.unique(z['y']).tolist()) == {0.0, 1.0, 2.0, 3.0}
        inside = CR.inside_mask(xv.cpu().numpy())
        assert bits(z['x']) == bits(CR.apply_stats(xv.cpu().numpy(), inside, st.cpu().numpy()))
        if clip is None:
            assert abs(z['x'][inside].astype(np.float64).mean(axis=0)).max() < 1e-6
            assert abs(z['x'][inside].astype(np.float64).std(axis=0) - 1.0).max() < 1e-6
    a, b = np.load(os.path.join(out, 'train', '1.npz'))['x'], np.load(os.path.join(out, 'train', '3.npz'))['x']
    assert abs(a).max() < 20 and abs(b).max() < 20                # five times the intensity, the same scale after normalisation


# ---- bts_amd.infer -------------------------------------------------------------------------------------------------------------------
KW = dict(base_filters=4, groups=2, reduction=2, depth=2)
SKULL_KW = dict(base_filters=4, groups=2, reduction=2, depth=2, out_ch=1)
VOL = (9, 10, 13)


def case_spec(clip):
    from bts_amd import preprocess
    return preprocess.NormSpec('case', clip, np.zeros(2), np.ones(2))


def small_model(kw, build, seed):
    from bts_amd.model import Model
    m = Model(**kw)
    m.build((1,) + tuple(build) + (2,))
    m.set_weights_from(S.randomised_params(R.default_config(**kw), tuple(build), seed))
    return m


@pytest.fixture(scope='module')
def padded_scan():
    import bts_amd  # noqa: F401
    from bts_amd import infer
    x = torch.from_numpy(S.scan_like(VOL, 5)).to(dev())
    mask = (x > 0).any(dim=-1, keepdim=True).float()
    xp, mp, _ = infer.pad_to_spatial_res(4, x, mask)
    return xp, mp


@pytest.mark.parametrize('how', ['whole', 'windowed', 'float16', 'channel_tta'])
def test_augmentor_in_case_mode_is_the_identity_augmentor_on_the_normalised_volume(padded_scan, how):
    from bts_amd import infer, ops
    xp, mp = padded_scan
    clip = (0.5, 99.5)
    kw = dict(KW)
    args = {}
    if how == 'windowed':
        args = dict(window=infer.WindowSpec((8, 8, 8)))
    if how == 'float16':
        kw, args = dict(base_filters=16, groups=8, reduction=2, depth=3), dict(compute_dtype='float16')
    if how == 'channel_tta':
        args = dict(channel_tta=1)
    m = small_model(kw, (8, 8, 8) if how == 'windowed' else tuple(xp.shape[:3]), 31)
    before = xp.clone()
    case = infer.TestTimeAugmentor(None, None, m, norm=case_spec(clip), **args)
    y = case(xp, mp)
    lab = case.labels()
    assert torch.equal(xp, before)                                 # normalised into a new tensor
    xn = ops.case_norm(xp, mp, clip)[0]
    plain = infer.TestTimeAugmentor(torch.zeros(2), torch.ones(2), m, **args)
    y2 = plain(xn, mp)
    assert torch.equal(y, y2) and torch.equal(lab, plain.labels()) and float(y.max()) > 0
    other = infer.TestTimeAugmentor(torch.zeros(2), torch.ones(2), m, norm=None, **args)(xp, mp)
    assert not torch.equal(other, y)                               # ... and norm=None is what it was: the raw volume with these statistics
    with pytest.raises(ValueError, match='NormSpec'):
        infer.TestTimeAugmentor(None, None, m, norm='case')


def test_segment_functions_take_norm():
    from bts_amd import infer
    x = torch.from_numpy(S.scan_like(VOL, 5)).to(dev())
    mask = (x > 0).any(dim=-1, keepdim=True).float()
    m = small_model(KW, S.padded(VOL, 4), 31)
    spec = case_spec((0.5, 99.5))
    y1, l1 = infer.segment_volume(m, x, mask, None, None, 4, norm=spec)
    y2, l2 = infer.segment_scan(m, x, (1.0, 1.0, 1.0), None, None, 4, norm=spec)
    stage = infer.StageSpec(m, None, None, 4, norm=spec)
    y3, l3 = infer.segment_case(stage, x, (1.0, 1.0, 1.0))
    ds = infer.StageSpec(m, torch.tensor([60.0, 70.0]), torch.tensor([30.0, 40.0]), 4)
    y4, l4 = infer.segment_case(ds, x, (1.0, 1.0, 1.0), norm=spec)                # the argument takes the place of the stage's own
    assert torch.equal(y1, y2) and torch.equal(y1, y3) and torch.equal(y1, y4) and torch.equal(l1, l2) and torch.equal(l1, l3) and torch.equal(l1, l4)
    y5, l5 = infer.segment_case(ds, x, (1.0, 1.0, 1.0))                            # ... for that call only
    y6, l6 = infer.segment_scan(m, x, (1.0, 1.0, 1.0), ds.mean, ds.std, 4)
    assert torch.equal(y5, y6) and torch.equal(l5, l6) and not torch.equal(y5, y1)


def test_two_stages_in_case_mode():
    """the skull stage normalises a copy: ops.skull_strip multiplies the raw scan.  And a scan of four times the intensity gets the
    same labels (x 4 is exact in every step: the normalised inputs are the same bits, the stripped scan is four times the other)"""
    from bts_amd import infer
    x = S.scan_like(VOL, 5)
    spec = case_spec((0.5, 99.5))
    skull = infer.StageSpec(small_model(SKULL_KW, S.padded(VOL, 4), 15), None, None, 4, norm=spec)
    tumor = infer.StageSpec(small_model(KW, S.padded(VOL, 4), 25), None, None, 4, norm=spec)
    y, lab, st = infer.segment_case(tumor, x, (1.0, 1.0, 1.0), skull=skull, return_stages=True)
    xp, mp, _ = infer.pad_to_spatial_res(4, torch.from_numpy(x).to(dev()), (torch.from_numpy(x).to(dev()) > 0).any(dim=-1, keepdim=True).float())
    assert torch.equal(st['x1mm'], xp) and torch.equal(st['mask'], mp)
    xo, mo = S.strip(st['x1mm'].cpu().numpy(), st['skull_prob'].cpu().numpy(), st['mask'].cpu().numpy(), VOL, S.padded(VOL, 4))
    assert bits(st['x_stripped'].cpu().numpy()) == bits(xo) and bits(st['mask_repadded'].cpu().numpy()) == bits(mo)
    y4, lab4, st4 = infer.segment_case(tumor, 4.0 * x, (1.0, 1.0, 1.0), skull=skull, return_stages=True)
    assert torch.equal(st4['skull_prob'], st['skull_prob']) and torch.equal(st4['x_stripped'], 4.0 * st['x_stripped'])
    assert torch.equal(lab4, lab) and torch.equal(y4, y)
    y1, lab1 = infer.segment_case(tumor, x, (1.0, 1.0, 1.0))
    y1b, lab1b = infer.segment_case(tumor, 4.0 * x, (1.0, 1.0, 1.0))
    assert torch.equal(lab1, lab1b) and torch.equal(y1, y1b)


# ---- the command ---------------------------------------------------------------------------------------------------------------------
def test_command_follows_the_prepro_file(tmp_path, capsys):
    import bts_amd  # noqa: F401
    from bts_amd import infer, nifti, preprocess
    from bts_amd import test as T
    from bts_amd.train import save_checkpoint, save_train_args
    data = tmp_path / 'data'
    os.makedirs(str(data / 'a'))
    x = S.scan_like(VOL, 5)
    nifti.save(str(data / 'a' / 'c_t1ce.nii.gz'), x[..., 0], np.eye(4))
    nifti.save(str(data / 'a' / 'c_flair.nii'), x[..., 1], np.eye(4))
    build = S.padded(VOL, 4)
    save_checkpoint(str(tmp_path / 'tumor'), small_model(KW, build, 31))
    save_train_args(str(tmp_path / 'tumor'), {'model_args': dict(KW), 'crop_size': list(build)})
    clip = (0.5, 99.5)
    np.save(str(tmp_path / 'tp.npy'), {'size': {'h': 16, 'w': 16, 'd': 16, 'c': 2},
                                      'norm': {'mode': 'case', 'clip': clip, 'mean': np.zeros((1, 1, 1, 2)), 'std': np.ones((1, 1, 1, 2))}})
    base = ['--in_locs', str(data), '--modalities', 't1ce,flair', '--gpu', '--tumor_model', str(tmp_path / 'tumor'),
            '--tumor_prepro', str(tmp_path / 'tp.npy'), '--workers', '0']
    assert T.main(base + ['--out_loc', str(tmp_path / 'out')]) == 0
    text = capsys.readouterr().out
    assert 'normalisation case, clipped to the percentiles 0.5, 99.5' in text and '1 cases segmented' in text
    args = T.parse_args(base)
    stage = T.load_stage(str(tmp_path / 'tumor'), str(tmp_path / 'tp.npy'), args, VOL)
    assert stage.norm.mode == 'case' and stage.norm.clip == clip
    xg, _ = T.upload_case(T.decode_case(str(data / 'a'), ['t1ce', 'flair'], ''), dev())
    plain = infer.StageSpec(stage.model, stage.mean, stage.std, stage.spatial_res)
    _, lab = infer.segment_case(plain, xg, (1.0, 1.0, 1.0), norm=preprocess.load_norm(str(tmp_path / 'tp.npy')))
    got = nifti.load(str(tmp_path / 'out' / 'a' / 'mask.nii'))[0]
    print('labels: %d of %d voxels are tumour' % (int((got > 0).sum()), got.size))
    assert got.shape == VOL and np.array_equal(got, lab.cpu().numpy()) and lab.any()
