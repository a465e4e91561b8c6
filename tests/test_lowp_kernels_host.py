"""CPU: the tolerances tests/test_lowp_kernels_gpu.py applies to the 16-bit non-conv kernels are honest, the reductions' inputs make
every seam count, storage_interval does what it says, and the entry points turn bad arguments away before any HIP call.

Every fp32 restatement of tests/lowp_ref.py must stay within K/4 of the bound its kernel is held to with K.  Bounds that are sums of
several terms with a K each (the gate, the epilogue's output, the heads) come back absolute: there K = 1 stands for the whole bound
and the restatement is held to a quarter of it.  Each test prints the ratio it measured (pytest -s)."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lowp_ref as L  # noqa: E402
from oracle import torch_ref as R  # noqa: E402

TDTS = [torch.float16, torch.bfloat16]
MODES = {L.SLAB: 'slab', L.CHANNEL: 'channel'}


def held(what, got, ref, unit, k, limit=None):
    limit = k / 4 if limit is None else limit
    r = L.ratio(got, ref, unit)
    print('%-58s %.3f (limit %g, K = %g)' % (what, r, limit, k))
    assert r <= limit, '%s: the fp32 restatement is %.3f x eps32*B from the reference, limit %g' % (what, r, limit)
    return r


# ---------------------------------------------------------------------------------------------------------------
# the references are the oracle's GroupNormalization
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,mode', [((2, 384, 32, 8), L.SLAB), ((1, 10, 24, 3), L.SLAB), ((2, 300, 32, 8), L.CHANNEL)])
def test_stats_and_apply_references_compose_to_the_oracle(shape, mode):
    n, v, c, g = shape
    x = L.randn_storage((n, v, c), torch.float16, 1, 4.0, 1.0)
    gamma, beta, _, _ = L.gn_params(n, c, g, 1)
    mean, rstd, _, _ = L.gn_stats_ref(x, g, mode, 1e-5)
    y, _ = L.gn_apply_ref(x, gamma.double(), beta.double(), mean, rstd, g, mode, False)
    x5 = x.double().reshape(n, v, 1, 1, c)
    if mode == L.SLAB:
        want = R.group_norm(x5, gamma.double(), beta.double(), g, -1, L.f32(1e-5)).reshape(n, v, c)
    else:
        want = R.group_norm(x5.permute(0, 4, 1, 2, 3), gamma.double(), beta.double(), g, 1, L.f32(1e-5)).permute(0, 2, 3, 4, 1).reshape(n, v, c)
    assert float((y - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_maxpool_reference_takes_the_values_of_torch_max_pool3d():
    for shape in L.MAXPOOL_SHAPES:
        x = L.maxpool_inputs(shape, torch.float16)
        y, idx = L.maxpool_ref(x)
        want = torch.nn.functional.max_pool3d(x.float().permute(0, 4, 1, 2, 3), 2).permute(0, 2, 3, 4, 1)
        assert torch.equal(y.float(), want)         # (== holds between -0.0 and +0.0: the sign of a zero is pinned below)
        wn = L.windows(x).reshape(-1, 8)
        yf, ix = y.reshape(-1), idx.reshape(-1)
        assert ix[0] == 0 and ix[1] == 0 and ix[4] == 7
        assert ix[2] == 3 and torch.signbit(yf[2])              # -0.0 came first: it stays
        assert ix[3] == 2 and not torch.signbit(yf[3])
        assert torch.equal(torch.gather(wn, 1, ix.long()[:, None])[:, 0].view(torch.int16), yf.view(torch.int16))
        dy = L.randn_storage(y.shape, torch.float16, 3)
        dx = L.maxpool_bwd_ref(dy, idx)
        assert torch.equal(L.windows(dx).sum(-1), dy) and int((dx != 0).sum()) <= dy.numel()


# ---------------------------------------------------------------------------------------------------------------
# restatement against reference, K/4
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape,mode', [(s, L.SLAB) for s in L.GN_STATS_SLAB] + [(s, L.CHANNEL) for s in L.GN_STATS_CHANNEL])
def test_gn_stats_restatement(shape, mode, tdt):
    x = L.gn_stats_inputs(shape, mode, tdt)
    m, r, bm, br = L.gn_stats_ref(x, shape[3], mode, 1e-5)
    m32, r32 = L.gn_stats_f32(x, shape[3], mode, 1e-5)
    held('gn_stats mean %s %s %s' % (shape, MODES[mode], tdt), m32, m, bm, L.K_RUN)
    held('gn_stats rstd %s %s %s' % (shape, MODES[mode], tdt), r32, r, br, L.K_RUN)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.GN_APPLY_CHUNKED + L.GN_APPLY_STRIDE)
def test_gn_apply_restatement(shape, tdt):
    n, v, c, g, mode = shape
    x = L.randn_storage((n, v, c), tdt, 2)
    gamma, beta, mean, rstd = L.gn_params(n, c, g, 2)
    for relu in (0, 1):
        ref, unit = L.gn_apply_ref(x, gamma, beta, mean, rstd, g, mode, relu)
        for fused in (True, False):
            held('gn_apply %s relu %d fused %d %s' % (shape, relu, fused, tdt), L.gn_apply_f32(x, gamma, beta, mean, rstd, g, mode, relu, fused),
                 ref, unit, L.K_LP)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.COLSUM_SHAPES)
def test_colsum_restatement(shape, tdt):
    x = L.colsum_inputs(shape, tdt)
    for scale in (1.0, 1.0 / shape[1]):
        ref, unit = L.lp_colsum_ref(x, scale)
        held('colsum %s scale %g %s' % (shape, scale, tdt), L.lp_colsum_f32(x, scale), ref, unit, L.K_RUN)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.EPILOGUE_CHUNKED + L.EPILOGUE_STRIDE)
def test_block_epilogue_restatement(shape, tdt):
    n, v, c, g, mode = shape
    p = L.epilogue_inputs(shape, tdt)
    sp, bsp, out, bout = L.epilogue_ref(p, g, mode)
    for fused in (True, False):
        sp32, out32 = L.epilogue_f32(p, g, mode, fused)
        held('epilogue gate %s fused %d %s' % (shape, fused, tdt), sp32, sp, bsp, 1.0)
        held('epilogue out  %s fused %d %s' % (shape, fused, tdt), out32, out, bout, 1.0)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.EPILOGUE_HEAD)
def test_block_epilogue_head_restatement(shape, tdt):
    n, v, c, g, mode = shape
    for k in (1, 2, 3, 4):
        p = L.epilogue_inputs(shape, tdt, k=k)
        for bias, sig in ((True, 1), (False, 1), (True, 0)):
            ref, bound = L.epilogue_head_ref(p, g, mode, bias, sig)
            held('epilogue_head %s K %d bias %d sigmoid %d %s' % (shape, k, bias, sig, tdt), L.epilogue_head_f32(p, g, mode, bias, sig), ref,
                 bound, 1.0)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape,oct_form', [(s, False) for s in L.HEAD_PER_VOXEL] + [(s, True) for s in L.HEAD_OCT])
def test_head_restatement(shape, oct_form, tdt):
    x, w, b = L.head_inputs(shape, tdt)
    for bias, sig in ((b, 1), (None, 1), (b, 0)):
        ref, bound = L.head_ref(x, w, bias, sig)
        long_chain = not oct_form and shape[1] >= 24          # one fma chain over all channels: lowp_ref's finding
        held('head %s bias %d sigmoid %d %s' % (shape, bias is not None, sig, tdt), L.head_f32(x, w, bias, sig, oct_form), ref, bound, 1.0,
             L.LONG_CHAIN_HOST_LIMIT if long_chain else None)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.HEAD_BWD)
def test_head_bwd_restatement(shape, tdt):
    x, dpre, w = L.head_bwd_inputs(shape, tdt)
    old_dw, old_db = L.randn32(w.shape, 11), L.randn32((shape[2],), 12)
    for ow, ob in ((None, None), (old_dw, old_db)):
        (dx, dw, db), (bx, bw, bb) = L.head_bwd_ref(x, dpre, w, ow, ob)
        dx32, dw32, db32 = L.head_bwd_f32(x, dpre, w, ow, ob)
        tag = '%s accumulate %d %s' % (shape, ow is not None, tdt)
        held('head_bwd dx ' + tag, dx32, dx, bx, L.K_LP)
        held('head_bwd dw ' + tag, dw32, dw, bw, L.K_RUN)
        held('head_bwd db ' + tag, db32, db, bb, L.K_RUN)


@pytest.mark.parametrize('tdt', TDTS)
@pytest.mark.parametrize('shape', L.UPSAMPLE_SHAPES)
def test_upsample_bwd_restatement(shape, tdt):
    n, d, h, w, c = shape
    dy = L.randn_storage((n, 2 * d, 2 * h, 2 * w, c), tdt, 4)
    old = L.randn_storage(shape, tdt, 5)
    for o in (None, old):
        ref, unit = L.upsample_bwd_ref(dy, o)
        held('upsample2_bwd %s accumulate %d %s' % (shape, o is not None, tdt), L.upsample_bwd_f32(dy, o), ref, unit, L.K_LP)
    assert torch.equal(L.windows(L.upsample_ref(old))[..., 3], old)


# ---------------------------------------------------------------------------------------------------------------
# every seam counts: on the reference alone, dropping or double-counting one seam item moves an output by >= 8 bounds
# ---------------------------------------------------------------------------------------------------------------
SEAM_MOVES = 8.0


@pytest.mark.parametrize('shape,mode', [(s, L.SLAB) for s in L.GN_STATS_SLAB + [L.GN_STATS_SLAB_PAST_CAP, L.GN_STATS_SLAB_OVER_CAP]] +
                         [(s, L.CHANNEL) for s in L.GN_STATS_CHANNEL])
def test_gn_stats_seams_count(shape, mode):
    n, v, c, g = shape
    for tdt in TDTS[:1] if shape == L.GN_STATS_SLAB_PAST_CAP else TDTS[1:] if shape == L.GN_STATS_SLAB_OVER_CAP else TDTS:
        x = L.gn_stats_inputs(shape, mode, tdt)
        _, _, bm, br = L.gn_stats_ref(x, g, mode, 1e-5)
        bm, br = (L.K_RUN * bm + L.TINY).reshape(n, g, 1), (L.K_RUN * br + L.TINY).reshape(n, g, 1)
        u = L._units(x.double(), g, mode)
        cnt = float(v * c // g)
        s, q = u.sum((2, 3))[..., None], (u * u).sum((2, 3))[..., None]
        m0, r0 = L.gn_stats_from_sums(s, q, cnt, L.f32(1e-5))
        it = u[:, :, torch.tensor(L.gn_stats_seams(v, c, g, mode))]
        si, qi = it.sum(-1), (it * it).sum(-1)
        worst = float('inf')
        for sign in (-1.0, 1.0):
            m1, r1 = L.gn_stats_from_sums(s + sign * si, q + sign * qi, cnt, L.f32(1e-5))
            moved = torch.maximum((m1 - m0).abs() / bm, (r1 - r0).abs() / br)
            worst = min(worst, float(moved.min()))
        print('gn_stats %s %s %s: %d seam items, the least visible moves an output by %.1f bounds' % (shape, MODES[mode], tdt, it.shape[2], worst))
        assert worst >= SEAM_MOVES


@pytest.mark.parametrize('shape', L.COLSUM_SHAPES + [L.COLSUM_PAST_CAP])
def test_colsum_seams_count(shape):
    n, v, c = shape
    x = L.colsum_inputs(shape, torch.float16)
    for scale in (1.0, 1.0 / v):
        _, unit = L.lp_colsum_ref(x, scale)
        bound = (L.K_RUN * unit + L.TINY)[:, None, :]
        it = x.double()[:, torch.tensor(L.colsum_seams(v, c))] * L.f32(scale)
        moved = (it.abs() / bound).reshape(n, -1, c // 8, 8).max(-1)[0]
        print('colsum %s scale %g: the least visible seam octet moves an output by %.1f bounds' % (shape, scale, float(moved.min())))
        assert float(moved.min()) >= SEAM_MOVES


@pytest.mark.parametrize('shape', L.HEAD_BWD + [L.HEAD_BWD_PAST_CAP])
def test_head_bwd_seams_count(shape):
    nvox, c, k = shape
    x, dpre, w = L.head_bwd_inputs(shape, torch.float16)
    old_dw, old_db = L.randn32(w.shape, 11), L.randn32((k,), 12)
    for ow, ob in ((None, None), (old_dw, old_db)):
        _, (_, bw, bb) = L.head_bwd_ref(x, dpre, w, ow, ob)
        idx = torch.tensor(L.head_bwd_seams(nvox, c))
        dw_i = x.double()[idx][:, :, None] * dpre.double()[idx][:, None, :]             # (seams, C, K): what the voxel adds to dw
        moved = (dw_i.abs() / (L.K_RUN * bw + L.TINY)).reshape(len(idx), c // 8, 8 * k).max(-1)[0]
        moved_b = (dpre.double()[idx].abs() / (L.K_RUN * bb + L.TINY)).max(-1)[0]
        print('head_bwd %s accumulate %d: %d seam voxels, least visible octet %.1f bounds (dw), %.1f (db)' % (
            shape, ow is not None, len(idx), float(moved.min()), float(moved_b.min())))
        assert float(moved.min()) >= SEAM_MOVES and float(moved_b.min()) >= SEAM_MOVES


# ---------------------------------------------------------------------------------------------------------------
# storage_interval on a hand table
# ---------------------------------------------------------------------------------------------------------------
H, B16 = torch.float16, torch.bfloat16
INTERVAL_TABLE = [
    # (type, ref, bound, lo, hi)
    (H, 1.0 + 2.0 ** -11, 0.0, 1.0, 1.0),                                   # a tie goes to the even neighbour ...
    (H, 1.0 + 3 * 2.0 ** -11, 0.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9),       # ... up as well as down
    (H, 1.0 + 2.0 ** -11, 2.0 ** -30, 1.0, 1.0 + 2.0 ** -10),               # a tie within the bound: both neighbours pass
    (H, 1.0 + 2.0 ** -12, 2.0 ** -30, 1.0, 1.0),                            # away from a tie: ONE value (truncation and RNE agree here)
    (H, 1.0 + 3 * 2.0 ** -12, 2.0 ** -30, 1.0 + 2.0 ** -10, 1.0 + 2.0 ** -10),   # ... and here truncation (1.0) fails
    (H, 65504.0, 1.0, 65504.0, 65504.0),
    (H, 65519.0, 0.5, 65504.0, 65504.0),
    (H, 65520.0, 0.0, float('inf'), float('inf')),                          # the tie at the top rounds to infinity
    (H, 65519.5, 1.0, 65504.0, float('inf')),
    (H, 2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -24),                           # the smallest subnormal
    (H, 2.0 ** -25, 0.0, 0.0, 0.0),                                         # half of it: tie to even = 0
    (H, 3 * 2.0 ** -25, 0.0, 2.0 ** -23, 2.0 ** -23),
    (H, 2.0 ** -25, 2.0 ** -40, 0.0, 2.0 ** -24),
    (H, 1023.5 * 2.0 ** -24, 0.0, 2.0 ** -14, 2.0 ** -14),                  # the largest subnormal's tie goes up to the smallest normal
    (H, 0.0, 2.0 ** -26, -0.0, 0.0),                                        # +-0: the interval [-0, +0] takes either zero
    (H, -2.0 ** -26, 2.0 ** -30, -0.0, -0.0),
    (B16, 1.0 + 2.0 ** -8, 0.0, 1.0, 1.0),
    (B16, 1.0 + 3 * 2.0 ** -8, 0.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -6),
    (B16, 1.0 + 2.0 ** -8, 2.0 ** -30, 1.0, 1.0 + 2.0 ** -7),
    (B16, 65520.0, 0.0, 65536.0, 65536.0),
    (B16, -(256.0 + 3.0), 0.0, -260.0, -260.0),
]


@pytest.mark.parametrize('tdt,ref,bound,lo,hi', INTERVAL_TABLE)
def test_storage_interval_hand_table(tdt, ref, bound, lo, hi):
    a, b = L.storage_interval(torch.tensor([ref], dtype=torch.float64), bound, tdt)
    assert a.dtype == tdt and b.dtype == tdt
    assert float(a) == lo and float(b) == hi, (float(a), float(b))
    if lo == 0.0 and hi == 0.0 and ref < 0:
        assert torch.signbit(a).item()
    # storage_ratio agrees: both ends sit at <= 1 bound from ref, the value beyond each end does not (where the bound is not 0)
    if bound > 0 and all(map(lambda t: abs(t) != float('inf'), (lo, hi))):
        for end in (a, b):
            assert L.storage_ratio(end, torch.tensor([ref], dtype=torch.float64), bound) <= 1.0


def test_check_storage_fails_truncation():
    g = torch.Generator().manual_seed(7)
    ref = torch.randn(4096, generator=g, dtype=torch.float64)
    unit = L.EPS32 * ref.abs()
    for tdt in TDTS:
        L.check_storage(ref.to(tdt), ref, unit, 16, 'RNE')
        sh = 13 if tdt == H else 16
        trunc = ((ref.float().view(torch.int32) >> sh) << sh).view(torch.float32).to(tdt)
        assert float((trunc != ref.to(tdt)).float().mean()) > 0.4
        with pytest.raises(AssertionError):
            L.check_storage(trunc, ref, unit, 16, 'truncation')
        assert L.storage_ratio(ref.to(tdt), ref, unit) == 0.0
        assert L.storage_ratio(trunc, ref, unit) > 1000


def test_cast_edge_table_reaches_what_it_names():
    e = L.cast_edge_values()
    h, b = e.to(H), e.to(B16)
    assert torch.isinf(h[e == 65520.0]).all() and float(h[e == 65504.0][0]) == 65504.0 and torch.isinf(h[e == 1e5]).all()
    assert float(h[e == 2.0 ** -25][0]) == 0.0 and float(h[e == 3 * 2.0 ** -25][0]) == 2.0 ** -23
    assert torch.isnan(h).sum() == 1 and torch.isnan(b).sum() == 1
    big = e[-4:].to(B16)       # bf16's largest value, the fp32 above it (rounds back down), +-FLT_MAX (past the last tie: infinite)
    assert big[0].float() == e[-4] and big[1] == big[0] and big[2] == float('inf') and big[3] == -float('inf')
    assert torch.signbit(h[1]) and float(h[1]) == 0.0


# ---------------------------------------------------------------------------------------------------------------
# argument statuses: every call returns before its first HIP call (read from csrc/lowp_norm.hip, lowp_block.hip and lowp_point.hip); nothing is launched
# ---------------------------------------------------------------------------------------------------------------
A = 4096        # a "pointer": 16-byte aligned, never dereferenced
OFF4 = 4100     # 4 bytes off a 16-byte boundary
OFF2 = 4098
BIG = 1 << 30
SHAPE, ALIGN, UNSUPPORTED, WORKSPACE = -1, -2, -3, -4


def _stats(x=A, ws=A, nb=BIG, n=1, v=64, c=8, g=1, mode=0):
    return (1, x, A, A, ws, nb, n, v, c, g, mode, 1e-5, None)


def _apply(x=A, y=A, n=1, v=64, c=8, ldy=8, g=1, mode=0):
    return (1, x, y, A, A, A, A, n, v, c, ldy, g, mode, 0, None)


def _colsum(x=A, nb=BIG, n=1, v=64, c=8):
    return (1, x, A, A, nb, n, v, c, 1.0, None)


def _epi(res=A, out=A, n=1, v=64, c=8, ldo=8, g=1, mode=0):
    return (1, res, A, out, None, A, A, A, A, A, A, n, v, c, ldo, g, mode, None)


def _epih(res=A, y=A, n=1, v=2048, c=8, g=1, mode=0, k=3):
    return (1, res, A, y, A, A, A, A, A, A, A, None, n, v, c, g, mode, k, 1, None)


def _head(x=A, nvox=64, c=8, ldx=8, k=3):
    return (1, x, A, None, A, nvox, c, ldx, k, 1, None)


def _headb(x=A, dx=A, ws=A, nb=BIG, nvox=64, c=16, ldx=16, lddx=16, k=3):
    return (1, x, A, A, dx, A, None, ws, nb, nvox, c, ldx, lddx, k, 0, None)


def _gnb(g=1):
    return (1, A, A, A, None, A, A, A, A, A, A, A, BIG, 1, 2048, 8, 8, g, 1, 1, None, None)


def _blkb(g=1):
    return (1, A, 8) + (A,) * 22 + (None, None, A, BIG, 1, 2048, 8, 2, g, None)


def _pool(x=A, y=A, idx=A, d=2, h=2, w=2, c=8, ldx=8, ldy=8):
    return (1, x, y, idx, 1, d, h, w, c, ldx, ldy, None)


def _poolb(idx=A, d=2, c=8, lddy=8, lddx=8):
    return (1, A, idx, A, 1, d, 2, 2, c, lddy, lddx, 0, None)


STATUS_CASES = [
    ('gn_stats G = 0', 'bts_lp_gn_stats', _stats(g=0), SHAPE),
    ('gn_stats G = -1', 'bts_lp_gn_stats', _stats(g=-1), SHAPE),
    ('gn_stats C % G', 'bts_lp_gn_stats', _stats(g=3), SHAPE),
    ('gn_stats slab L % 8', 'bts_lp_gn_stats', _stats(v=1, c=12), UNSUPPORTED),
    ('gn_stats misaligned x', 'bts_lp_gn_stats', _stats(x=OFF4), ALIGN),
    ('gn_stats misaligned workspace', 'bts_lp_gn_stats', _stats(ws=OFF4), ALIGN),
    ('gn_stats short workspace', 'bts_lp_gn_stats', _stats(nb=64), WORKSPACE),
    ('gn_apply G = 0', 'bts_lp_gn_apply', _apply(g=0), SHAPE),
    ('gn_apply C = 0', 'bts_lp_gn_apply', _apply(c=0, ldy=0), SHAPE),
    ('gn_apply C % 8', 'bts_lp_gn_apply', _apply(c=12, ldy=16), SHAPE),
    ('gn_apply ldy < C', 'bts_lp_gn_apply', _apply(c=16, ldy=8), SHAPE),
    ('gn_apply ldy % 8', 'bts_lp_gn_apply', _apply(ldy=12), SHAPE),
    ('gn_apply misaligned y', 'bts_lp_gn_apply', _apply(y=OFF4), ALIGN),
    ('colsum C = 0', 'bts_lp_colsum', _colsum(c=0), SHAPE),
    ('colsum C % 8', 'bts_lp_colsum', _colsum(c=12), SHAPE),
    ('colsum C = 264', 'bts_lp_colsum', _colsum(c=264), SHAPE),
    ('colsum C / 8 = 3', 'bts_lp_colsum', _colsum(c=24), SHAPE),
    ('colsum misaligned x', 'bts_lp_colsum', _colsum(x=OFF4), ALIGN),
    ('colsum short workspace', 'bts_lp_colsum', _colsum(nb=64), WORKSPACE),
    ('block_epilogue G = 0', 'bts_lp_block_epilogue', _epi(g=0), SHAPE),
    ('block_epilogue C = 0', 'bts_lp_block_epilogue', _epi(c=0, ldo=0), SHAPE),
    ('block_epilogue C % 8', 'bts_lp_block_epilogue', _epi(c=12, ldo=16), SHAPE),
    ('block_epilogue C / 8 = 3', 'bts_lp_block_epilogue', _epi(c=24, ldo=24), SHAPE),
    ('block_epilogue ldo < C', 'bts_lp_block_epilogue', _epi(c=16, ldo=8), SHAPE),
    ('block_epilogue misaligned out', 'bts_lp_block_epilogue', _epi(out=OFF4), ALIGN),
    ('block_epilogue_head G = 0', 'bts_lp_block_epilogue_head', _epih(g=0), SHAPE),
    ('block_epilogue_head C = 0', 'bts_lp_block_epilogue_head', _epih(c=0), SHAPE),
    ('block_epilogue_head K = 0', 'bts_lp_block_epilogue_head', _epih(k=0), SHAPE),
    ('block_epilogue_head C = 128', 'bts_lp_block_epilogue_head', _epih(c=128), UNSUPPORTED),
    ('block_epilogue_head K = 5', 'bts_lp_block_epilogue_head', _epih(k=5), UNSUPPORTED),
    ('block_epilogue_head ragged unit', 'bts_lp_block_epilogue_head', _epih(v=100), UNSUPPORTED),
    ('block_epilogue_head misaligned y', 'bts_lp_block_epilogue_head', _epih(y=OFF2), ALIGN),
    ('head C = 0', 'bts_lp_head', _head(c=0, ldx=0), SHAPE),
    ('head ldx < C', 'bts_lp_head', _head(c=16, ldx=8), SHAPE),
    ('head C % 8', 'bts_lp_head', _head(c=12, ldx=16), SHAPE),
    ('head K = 5', 'bts_lp_head', _head(k=5), SHAPE),
    ('head misaligned x', 'bts_lp_head', _head(x=OFF4), ALIGN),
    ('head_bwd C = 24', 'bts_lp_head_bwd', _headb(c=24, ldx=24, lddx=24), UNSUPPORTED),
    ('head_bwd C = 8', 'bts_lp_head_bwd', _headb(c=8), UNSUPPORTED),
    ('head_bwd K = 5', 'bts_lp_head_bwd', _headb(k=5), UNSUPPORTED),
    ('head_bwd ldx < C', 'bts_lp_head_bwd', _headb(ldx=8), SHAPE),
    ('head_bwd lddx < C', 'bts_lp_head_bwd', _headb(lddx=8), SHAPE),
    ('head_bwd misaligned dx', 'bts_lp_head_bwd', _headb(dx=OFF4), ALIGN),
    ('head_bwd short workspace', 'bts_lp_head_bwd', _headb(nb=64), WORKSPACE),
    ('gn_bwd G = 0', 'bts_lp_gn_bwd', _gnb(g=0), SHAPE),
    ('block_bwd G = 0', 'bts_lp_block_bwd', _blkb(g=0), SHAPE),
    ('maxpool2_fwd D odd', 'bts_lp_maxpool2_fwd', _pool(d=3), SHAPE),
    ('maxpool2_fwd W odd', 'bts_lp_maxpool2_fwd', _pool(w=5), SHAPE),
    ('maxpool2_fwd C % 8', 'bts_lp_maxpool2_fwd', _pool(c=4), SHAPE),
    ('maxpool2_fwd ldx < C', 'bts_lp_maxpool2_fwd', _pool(c=16, ldx=8, ldy=16), SHAPE),
    ('maxpool2_fwd misaligned y', 'bts_lp_maxpool2_fwd', _pool(y=OFF4), ALIGN),
    ('maxpool2_bwd idx == NULL', 'bts_lp_maxpool2_bwd', _poolb(idx=None), SHAPE),
    ('maxpool2_bwd D odd', 'bts_lp_maxpool2_bwd', _poolb(d=3), SHAPE),
    ('maxpool2_bwd lddx < C', 'bts_lp_maxpool2_bwd', _poolb(c=16, lddy=16, lddx=8), SHAPE),
    ('upsample2_fwd C % 8', 'bts_lp_upsample2_fwd', (1, A, A, 1, 1, 1, 1, 12, 16, 16, None), SHAPE),
    ('upsample2_fwd ldy < C', 'bts_lp_upsample2_fwd', (1, A, A, 1, 1, 1, 1, 16, 16, 8, None), SHAPE),
    ('upsample2_bwd misaligned dy', 'bts_lp_upsample2_bwd', (1, OFF4, A, 1, 1, 1, 1, 8, 8, 8, 0, None), ALIGN),
    ('upsample2_bwd dtype 3', 'bts_lp_upsample2_bwd', (3, A, A, 1, 1, 1, 1, 8, 8, 8, 0, None), UNSUPPORTED),
    ('cast rows = 0', 'bts_lp_cast', (1, A, 2, A, 2, 0, 2, None), SHAPE),
    ('cast dtype 0', 'bts_lp_cast', (0, A, 2, A, 2, 8, 2, None), UNSUPPORTED),
    ('uncast C = 0', 'bts_lp_uncast', (2, A, 0, A, 0, 8, 0, None), SHAPE),
    ('cast_pad16 C = 5', 'bts_lp_cast_pad16', (1, A, 5, A, 8, 5, None), SHAPE),
    ('cast_pad16 ld_src < C', 'bts_lp_cast_pad16', (1, A, 1, A, 8, 2, None), SHAPE),
    ('cast_pad16 misaligned dst', 'bts_lp_cast_pad16', (1, A, 2, OFF4, 8, 2, None), ALIGN),
    ('dropout_cast_pad16 rate = 1', 'bts_lp_dropout_cast_pad16', (1, A, A, 8, 2, 1.0, 5, None), SHAPE),
    ('dropout_cast_pad16 misaligned dst', 'bts_lp_dropout_cast_pad16', (1, A, OFF4, 8, 2, 0.2, 5, None), ALIGN),
]


@pytest.mark.parametrize('what,name,args,status', STATUS_CASES, ids=[c[0] for c in STATUS_CASES])
def test_argument_status(what, name, args, status):
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    lb = lib()
    assert len(args) == len(lb.protos[name][1]), 'argument list does not match the header'
    assert getattr(lb, '_' + name)(*args) == status
