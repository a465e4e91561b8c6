"""-m gpu: the 16-bit non-conv kernels of csrc/lowp_norm.hip, lowp_block.hip and lowp_point.hip against the fp64 references of tests/lowp_ref.py, at the shapes where their
two forms, their block spans, their unrolled loops and their grid caps part ways.  The Ks are lowp_ref's, unchanged; outputs in the
storage type are held to storage_interval (no u * |ref| of slack); selections and copies are compared bit for bit.  Every check
prints its ratio first (pytest -s); where a bound is a sum of terms with a K each (the gate, the epilogue's output, the heads) the
ratio is a fraction of the whole bound ("of K = 1").  Channel-slice outputs sit in a sentinel-filled slab whose other channels must come back intact;
no call passes a pointer or extent that lets a kernel touch memory outside its buffers.

Not reached by these shapes (see lowp_ref's docstring): gn_stats' `cnt == 64` flush (more than 3.3e7 elements per group), the
32768-block caps of both head kernels (2^26 elements or more: left to the full-size tests), the 16384-block caps of maxpool2
forward / backward and upsample2 backward (2.7e8-element tensors: not covered)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import lowp_ref as L  # noqa: E402

DEV = torch.device('cuda', 0)
BOTH = ['float16', 'bfloat16']
MODES = {L.SLAB: 'slab', L.CHANNEL: 'channel'}
PAD = 16        # extra channels of a slab around a channel-slice view


def _lp():
    import bts_amd  # noqa: F401
    from bts_amd import lowp, ops
    from bts_amd._lib import lib
    return lowp, ops, lib()


def v5(t):
    """(N, V, C) -> the (N, V, 1, 1, C) view the wrappers take"""
    return t.reshape(t.shape[0], t.shape[1], 1, 1, t.shape[2])


def dev(t):
    return t.to(DEV)


def slab(shape, c, ld, dtype):
    """a sentinel-filled dense (..., ld) buffer on the device and its [..., :c] view"""
    buf = torch.full(tuple(shape) + (ld,), L.SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[..., :c]


def intact(buf, c, what):
    assert bool((buf[..., c:] == L.SENTINEL).all()), '%s: wrote outside its channel slice' % what


def in_slab(t, pad=PAD):
    """t (N, D, H, W, C) on the CPU -> its copy on the device as the first C channels of a wider buffer"""
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + pad,), 3.0, dtype=t.dtype, device=DEV)
    buf[..., :t.shape[-1]] = dev(t)
    return buf[..., :t.shape[-1]]


# ---------------------------------------------------------------------------------------------------------------
# GroupNormalization statistics
# ---------------------------------------------------------------------------------------------------------------
STATS_CASES = [(s, L.SLAB, d) for s in L.GN_STATS_SLAB for d in BOTH] + [(L.GN_STATS_SLAB_PAST_CAP, L.SLAB, 'float16'), (L.GN_STATS_SLAB_OVER_CAP, L.SLAB, 'bfloat16')] + \
              [(s, L.CHANNEL, d) for s in L.GN_STATS_CHANNEL for d in BOTH]


@pytest.mark.parametrize('shape,mode,dtype', STATS_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_gn_stats(shape, mode, dtype):
    """slab (2,1,8,1): one octet per unit; (1,769,8,1): trips and a tail; (1,5121,8,1): B = 2 and `per` rounded up past the unit's
    end; (1,525289,8,1): 256 blocks, the cap's own value; (1,526337,8,1): the cap binds.  The `cnt == 64` flush needs > 3.3e7 elements per group and is not reached."""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    n, v, c, g = shape
    if shape == (1, 5121, 8, 1):
        assert L.gn_blocks(v * c // g) == 2 and (v * c // g // 8) % 2 == 1
    if shape == L.GN_STATS_SLAB_PAST_CAP:
        assert (v * c // g) // 16384 == 256 and L.gn_blocks(v * c // g) == 256
    if shape == L.GN_STATS_SLAB_OVER_CAP:
        assert (v * c // g) // 16384 > 256 and L.gn_blocks(v * c // g) == 256
    x = L.gn_stats_inputs(shape, mode, tdt)
    mean, rstd = lowp.gn_stats(code, v5(dev(x)), g, mode, 1e-5)
    m, r, bm, br = L.gn_stats_ref(x, g, mode, 1e-5)
    tag = '%s %s %s' % (shape, MODES[mode], dtype)
    L.check(mean, m, bm, L.K_RUN, 'gn_stats mean ' + tag)
    L.check(rstd, r, br, L.K_RUN, 'gn_stats rstd ' + tag)


# ---------------------------------------------------------------------------------------------------------------
# GroupNormalization application
# ---------------------------------------------------------------------------------------------------------------
APPLY_CASES = [(s, d) for s in L.GN_APPLY_CHUNKED + L.GN_APPLY_STRIDE for d in BOTH] + [(L.GN_APPLY_PAST_CAP, 'float16')]


@pytest.mark.parametrize('shape,dtype', APPLY_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_gn_apply(shape, dtype):
    """chunked form: 1 step; 7 steps = one unrolled trip of 4 + 3 of the remainder loop; 9 steps in chunks of 5 and 4; channel mode at
    C = 8 (one lane per voxel) and C = 256 (32 lanes).  Grid-stride form: C = 24 (2048 % C != 0), ragged units, and past its
    16384-block cap."""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    n, v, c, g, mode = shape
    past = shape == L.GN_APPLY_PAST_CAP
    assert L.takes_chunked(n, v, c, g, mode) == (shape in L.GN_APPLY_CHUNKED)
    if past:
        assert n * v * c // 8 > 16384 * 256
    x = L.randn_storage((n, v, c), tdt, 2)
    gamma, beta, mean, rstd = L.gn_params(n, c, g, 2)
    xd = v5(dev(x))
    dp = [dev(t) for t in (gamma, beta, mean, rstd)]
    if past:
        out = lowp.gn_apply(code, xd, dp[0], dp[1], dp[2], dp[3], g, mode, 1).reshape(n, v, c)
        for lo, hi in L.chunks(v):
            ref, unit = L.gn_apply_ref(x[:, lo:hi], gamma, beta, mean, rstd, g, mode, 1, lo, v)
            L.check_storage(out[:, lo:hi], ref, unit, L.K_LP, 'gn_apply %s relu 1 voxels [%d, %d) %s' % (shape, lo, hi, dtype))
        return
    for relu in (0, 1):
        ref, unit = L.gn_apply_ref(x, gamma, beta, mean, rstd, g, mode, relu)
        for ld in (c, c + PAD):
            buf, out = slab((n, v, 1, 1), c, ld, tdt)
            lowp.gn_apply(code, xd, dp[0], dp[1], dp[2], dp[3], g, mode, relu, out=out)
            what = 'gn_apply %s relu %d ldy %d %s' % (shape, relu, ld, dtype)
            L.check_storage(out.reshape(n, v, c), ref, unit, L.K_LP, what)
            intact(buf, c, what)


# ---------------------------------------------------------------------------------------------------------------
# column sums
# ---------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [(s, d) for s in L.COLSUM_SHAPES for d in BOTH] + [(L.COLSUM_PAST_CAP, 'bfloat16')]


@pytest.mark.parametrize('shape,dtype', COLSUM_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_colsum(shape, dtype):
    """one voxel; C = 256 (32 octets, 8 voxels per trip); 33 voxels on 32 lanes' rows; B = 2 with a ragged second span; the same at C = 256:
    257 trips per lane, past the `cnt == 256` flush to fp64; the 512-block cap"""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    n, v, c = shape
    if shape == (1, 4097, 32):
        assert L.colsum_blocks(v) == 2
    if shape == L.COLSUM_PAST_CAP:
        assert v // 2048 > 512
    x = L.colsum_inputs(shape, tdt)
    xd = v5(dev(x))
    for scale in (1.0, 1.0 / v):
        ref, unit = L.lp_colsum_ref(x, scale)
        L.check(lowp.colsum(code, xd, scale), ref, unit, L.K_RUN, 'colsum %s scale %g %s' % (shape, scale, dtype))


# ---------------------------------------------------------------------------------------------------------------
# block epilogue
# ---------------------------------------------------------------------------------------------------------------
EPI_CASES = [(s, d) for s in L.EPILOGUE_CHUNKED + L.EPILOGUE_STRIDE for d in BOTH] + [(L.EPILOGUE_PAST_CAP, 'float16')]


def _epi_dev(p):
    return {k: (v5(dev(t)) if k in ('res', 'c2') else dev(t)) for k, t in p.items()}


@pytest.mark.parametrize('shape,dtype', EPI_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_block_epilogue(shape, dtype):
    """chunked form: 1 step; 3 steps = one unrolled pair + 1 remainder; chunks of 5 and 4 steps; C = 256 in channel mode.  Grid-stride
    form: 3 voxels; ragged units; C = 256; past the 16384-block cap."""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    n, v, c, g, mode = shape
    past = shape == L.EPILOGUE_PAST_CAP
    assert L.takes_chunked(n, v, c, g, mode) == (shape in L.EPILOGUE_CHUNKED)
    if past:
        assert n * v * c // 8 > 16384 * 256
    p = L.epilogue_inputs(shape, tdt)
    d = _epi_dev(p)
    if past:
        out = torch.empty_like(d['res'])
        sp_out = torch.empty(n * v, dtype=torch.float32, device=DEV)
        lowp.block_epilogue(code, d['res'], d['c2'], out, d['wsp'], d['ch'], d['gamma'], d['beta'], d['mean'], d['rstd'], g, mode, sp_out=sp_out)
        out, sp_out = out.reshape(n, v, c), sp_out.reshape(n, v)
        for lo, hi in L.chunks(v):
            q = dict(p, res=p['res'][:, lo:hi], c2=p['c2'][:, lo:hi])
            sp, bsp, ref, bout = L.epilogue_ref(q, g, mode, lo, v)
            what = 'block_epilogue %s voxels [%d, %d) %s' % (shape, lo, hi, dtype)
            L.check(sp_out[:, lo:hi], sp, bsp, 1.0, what + ' gate')
            L.check_storage(out[:, lo:hi], ref, bout, 1.0, what + ' out')
        return
    sp, bsp, ref, bout = L.epilogue_ref(p, g, mode)
    for ld, with_sp in ((c, True), (c + PAD, False), (c + PAD, True)):
        buf, out = slab((n, v, 1, 1), c, ld, tdt)
        sp_out = torch.full((n * v + 8,), L.SENTINEL, dtype=torch.float32, device=DEV) if with_sp else None
        lowp.block_epilogue(code, d['res'], d['c2'], out, d['wsp'], d['ch'], d['gamma'], d['beta'], d['mean'], d['rstd'], g, mode,
                            sp_out=sp_out)
        what = 'block_epilogue %s ldo %d sp_out %d %s' % (shape, ld, with_sp, dtype)
        if with_sp:
            L.check(sp_out[:n * v].reshape(n, v), sp, bsp, 1.0, what + ' gate')
            assert bool((sp_out[n * v:] == L.SENTINEL).all())
        L.check_storage(out.reshape(n, v, c), ref, bout, 1.0, what + ' out')
        intact(buf, c, what)


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('shape', L.EPILOGUE_HEAD, ids=lambda v: str(v).replace(' ', ''))
def test_block_epilogue_head(shape, dtype):
    """against fp64 directly (the head sees the UNROUNDED block output), K = 1 .. 4, bias None, sigmoid 0 and 1"""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    n, v, c, g, mode = shape
    for k in (1, 2, 3, 4):
        p = L.epilogue_inputs(shape, tdt, k=k)
        d = _epi_dev(p)
        for bias, sig in ((True, 1), (False, 1), (True, 0)):
            ref, bound = L.epilogue_head_ref(p, g, mode, bias, sig)
            y = lowp.block_epilogue_head(code, d['res'], d['c2'], d['wsp'], d['ch'], d['gamma'], d['beta'], d['mean'], d['rstd'], g, mode,
                                         d['hw'], d['hb'] if bias else None, sigmoid=bool(sig))
            assert y is not None
            L.check(y.reshape(n, v, k), ref, bound, 1.0, 'epilogue_head %s K %d bias %d sigmoid %d %s' % (shape, k, bias, sig, dtype))


def test_block_epilogue_head_leaves_wide_blocks_to_the_two_kernels():
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES['float16']
    shape = (1, 144, 128, 8, L.CHANNEL)
    assert L.takes_chunked(*shape)
    d = _epi_dev(L.epilogue_inputs(shape, tdt, k=3))
    assert lowp.block_epilogue_head(code, d['res'], d['c2'], d['wsp'], d['ch'], d['gamma'], d['beta'], d['mean'], d['rstd'], 8, L.CHANNEL,
                                    d['hw'], d['hb']) is None


# ---------------------------------------------------------------------------------------------------------------
# output head, forward and backward
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('shape', L.HEAD_PER_VOXEL + L.HEAD_OCT, ids=lambda v: str(v).replace(' ', ''))
def test_head(shape, dtype):
    """per-voxel kernel below 4096 voxels (and at C = 24: three octets are no power of two), the oct kernel from 4096 on: the threshold
    itself, a last trip with dead lanes (4097, 5003, 4100), C = 256 (32 lanes per voxel).  The 32768-block caps of both kernels lie at
    2^26 elements or more: left to the full-size tests."""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    nvox, c, k = shape
    x, w, b = L.head_inputs(shape, tdt)
    dense = dev(x).reshape(1, nvox, 1, 1, c)
    view = in_slab(x.reshape(1, nvox, 1, 1, c))
    wd, bd = dev(w), dev(b)
    for xin, bias, sig in ((dense, b, 1), (view, b, 1), (dense, None, 1), (view, b, 0)):
        ref, bound = L.head_ref(x, w, bias, sig)
        y = torch.full((nvox * k + 8,), L.SENTINEL, dtype=torch.float32, device=DEV)
        _lp()[2].call('bts_lp_head', code, xin.data_ptr(), wd.data_ptr(), bd.data_ptr() if bias is not None else None, y.data_ptr(), nvox, c,
                      xin.stride(-2), k, sig, None)
        torch.cuda.synchronize()
        what = 'head %s ldx %d bias %d sigmoid %d %s' % (shape, xin.stride(-2), bias is not None, sig, dtype)
        L.check(y[:nvox * k].reshape(nvox, k), ref, bound, 1.0, what)
        assert bool((y[nvox * k:] == L.SENTINEL).all()), what + ': wrote past the last voxel'


HEAD_BWD_CASES = [(s, d) for s in L.HEAD_BWD for d in BOTH] + [(L.HEAD_BWD_PAST_CAP, 'bfloat16')]


@pytest.mark.parametrize('shape,dtype', HEAD_BWD_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_head_bwd(shape, dtype):
    """one voxel; less than a workgroup; several workgroups with a ragged last one; past the 2048-block cap (two trips of the loop)"""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    nvox, c, k = shape
    if shape == L.HEAD_BWD_PAST_CAP:
        assert (nvox * (c // 8) + 255) // 256 > 2048
    x, dpre, w = L.head_bwd_inputs(shape, tdt)
    old_dw, old_db = L.randn32(w.shape, 11), L.randn32((k,), 12)
    dense = dev(x).reshape(1, nvox, 1, 1, c)
    view = in_slab(x.reshape(1, nvox, 1, 1, c))
    dp, wd = dev(dpre).reshape(1, nvox, 1, 1, k), dev(w)
    for xin, acc, with_db in ((dense, 0, True), (view, 1, True), (dense, 1, False)):
        (dxr, dwr, dbr), (bx, bw, bb) = L.head_bwd_ref(x, dpre, w, old_dw if acc else None, old_db if acc else None)
        dw, db = dev(old_dw).clone(), dev(old_db).clone()
        dx = lowp.head_bwd(code, tdt, xin, dp, wd, dw, db if with_db else None, accumulate=bool(acc))
        what = 'head_bwd %s ldx %d accumulate %d db %d %s' % (shape, xin.stride(-2), acc, with_db, dtype)
        L.check_storage(dx.reshape(nvox, c), dxr, bx, L.K_LP, what + ' dx')
        L.check(dw, dwr, bw, L.K_RUN, what + ' dw')
        if with_db:
            L.check(db, dbr, bb, L.K_RUN, what + ' db')
        else:
            assert torch.equal(db.cpu(), old_db)


# ---------------------------------------------------------------------------------------------------------------
# samplers
# ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().cpu().view(torch.int16)


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('shape,views', [(L.MAXPOOL_SHAPES[0], False), (L.MAXPOOL_SHAPES[1], True)], ids=['2x2x2', 'slabs'])
def test_maxpool2(shape, views, dtype):
    """all-equal, all-negative and -0.0 / +0.0 windows: value and index bit for bit (the FIRST maximum); the gradient with accumulate 0, 1"""
    lowp, ops, lb = _lp()
    code, tdt = L.DTYPES[dtype]
    n, d, h, w, c = shape
    x = L.maxpool_inputs(shape, tdt)
    yr, ir = L.maxpool_ref(x)
    xd = in_slab(x) if views else dev(x)
    ybuf, y = slab((n, d // 2, h // 2, w // 2), c, c + PAD if views else c, tdt)
    idx = torch.full(yr.shape, 255, dtype=torch.uint8, device=DEV)
    lb.call('bts_lp_maxpool2_fwd', code, xd.data_ptr(), y.data_ptr(), idx.data_ptr(), n, d, h, w, c, xd.stride(-2), y.stride(-2), None)
    torch.cuda.synchronize()
    assert torch.equal(idx.cpu(), ir), 'maxpool2 %s %s: index' % (shape, dtype)
    assert torch.equal(_bits(y), _bits(yr)), 'maxpool2 %s %s: value bits' % (shape, dtype)
    intact(ybuf, c, 'maxpool2 fwd')
    dy = L.randn_storage(yr.shape, tdt, 21)
    old = L.randn_storage(shape, tdt, 22)
    dyd = in_slab(dy) if views else dev(dy)
    for acc in (0, 1):
        dbuf, dx = slab((n, d, h, w), c, c + PAD if views else c, tdt)
        dx.copy_(dev(old))
        lowp.maxpool2_bwd(code, dyd, idx, dx, acc)
        want = L.maxpool_bwd_ref(dy, ir, old if acc else None)
        assert torch.equal(_bits(dx), _bits(want)), 'maxpool2_bwd %s accumulate %d %s' % (shape, acc, dtype)
        intact(dbuf, c, 'maxpool2 bwd')


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('shape,views', [(L.UPSAMPLE_SHAPES[0], False), (L.UPSAMPLE_SHAPES[1], True)], ids=['1x1x1', 'slabs'])
def test_upsample2(shape, views, dtype):
    """the repeat bit for bit; its gradient (fp32 sums of 8, + the old value) by storage_interval.  The 16384-block caps of the
    backward and of the pool need 2.7e8-element tensors: not covered."""
    lowp, ops, lb = _lp()
    code, tdt = L.DTYPES[dtype]
    n, d, h, w, c = shape
    x = L.randn_storage(shape, tdt, 23)
    xd = in_slab(x) if views else dev(x)
    ybuf, y = slab((n, 2 * d, 2 * h, 2 * w), c, c + PAD if views else c, tdt)
    lowp.upsample2(code, xd, out=y)
    assert torch.equal(_bits(y), _bits(L.upsample_ref(x))), 'upsample2 %s %s' % (shape, dtype)
    intact(ybuf, c, 'upsample2 fwd')
    dy = L.randn_storage(y.shape, tdt, 24)
    old = L.randn_storage(shape, tdt, 25)
    dyd = in_slab(dy) if views else dev(dy)
    for acc in (0, 1):
        dbuf, dx = slab((n, d, h, w), c, c + PAD if views else c, tdt)
        dx.copy_(dev(old))
        lowp.upsample2_bwd(code, dyd, dx=dx, accumulate=bool(acc))
        ref, unit = L.upsample_bwd_ref(dy, old if acc else None)
        what = 'upsample2_bwd %s accumulate %d %s' % (shape, acc, dtype)
        L.check_storage(dx, ref, unit, L.K_LP, what)
        intact(dbuf, c, what)


def test_upsample2_forward_past_its_block_cap():
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES['bfloat16']
    n, d, h, w, c = L.UPSAMPLE_PAST_CAP
    assert 8 * n * d * h * w * (c // 8) > 16384 * 256
    x = L.randn_storage(L.UPSAMPLE_PAST_CAP, tdt, 26)
    y = lowp.upsample2(code, dev(x))
    assert torch.equal(_bits(y), _bits(L.upsample_ref(x)))


# ---------------------------------------------------------------------------------------------------------------
# casts
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', BOTH)
def test_casts_on_the_edge_table(dtype):
    """ties to even, fp16's 65504 / 65520 / 1e5, subnormals and 2^-25, +-0, +-inf, NaN, bf16's largest value and the fp32 above it -- through
    the generic kernel (C = 5; C = 2 into an odd ld_dst), the rows kernel (C = 1, 2, 3, 4), cast_pad16, dropout_cast_pad16 at rate 0 (its own
    store path), and back through uncast"""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES[dtype]
    rows = 96
    for c in (1, 2, 3, 4, 5):
        src = L.cast_table(rows, c)
        want = src.to(tdt)
        got = lowp.cast(code, tdt, dev(src))
        assert L.same_bits_or_nan(got.cpu(), want), 'cast C = %d %s' % (c, dtype)
        back = lowp.uncast(code, got)
        assert L.same_bits_or_nan(back.cpu(), want.float()), 'uncast C = %d %s' % (c, dtype)
        if c <= 4:
            pad = lowp.cast_pad16(code, tdt, dev(src)).cpu()
            assert L.same_bits_or_nan(pad[:, :c].contiguous(), want) and bool((pad[:, c:].view(torch.int16) == 0).all()), 'cast_pad16 C = %d' % c
            drop = lowp.dropout_cast_pad16(code, tdt, dev(src), 0.0, 5).cpu()       # rate 0: every element kept, scale 1 / (1 - 0) = 1
            assert L.same_bits_or_nan(drop[:, :c].contiguous(), want) and bool((drop[:, c:].view(torch.int16) == 0).all()), \
                'dropout_cast_pad16 at rate 0, C = %d' % c
    src = L.cast_table(rows, 2)
    buf, out = slab((rows,), 2, 3, tdt)             # odd row stride: the generic kernel, not the rows kernel's 4-byte stores
    lowp.cast(code, tdt, dev(src), out=out)
    assert L.same_bits_or_nan(out.contiguous().cpu(), src.to(tdt))
    intact(buf, 2, 'cast into an odd row stride')


def _tail_rows(rows, c, seed):
    """(rows, c) fp32 whose LAST 4096 rows hold the edge table and random values: the rows past a grid cap are the last ones"""
    src = torch.zeros((rows, c))
    src[-4096:] = L.randn32((4096, c), seed)
    src[-96:] = L.cast_table(96, c)
    src[:96] = L.cast_table(96, c)
    return src


def test_casts_past_their_grid_caps():
    """generic kernel and uncast (65536 blocks of 256 elements): 3355500 rows of 5; rows kernel (65536 blocks of 256 rows): 16778000 rows of
    1; cast_pad16 (16384 blocks of 256 rows): 4195000 rows of 2"""
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES['float16']
    for rows, c, cap in ((3355500, 5, 65536 * 256 // 5), (16778000, 1, 65536 * 256)):
        assert rows > cap
        src = _tail_rows(rows, c, 31)
        got = lowp.cast(code, tdt, dev(src))
        assert L.same_bits_or_nan(got.cpu(), src.to(tdt)), 'cast %d rows of %d' % (rows, c)
        if c == 5:
            assert L.same_bits_or_nan(lowp.uncast(code, got).cpu(), src.to(tdt).float())
        del got
    code, tdt = L.DTYPES['bfloat16']
    rows, c = 4195000, 2
    assert rows > 16384 * 256
    src = _tail_rows(rows, c, 32)
    pad = lowp.cast_pad16(code, tdt, dev(src)).cpu()
    assert L.same_bits_or_nan(pad[:, :c].contiguous(), src.to(tdt)) and bool((pad[:, c:].view(torch.int16) == 0).all())


def test_dropout_cast_pad16_equals_the_three_passes_past_its_grid_cap():
    lowp, ops, _ = _lp()
    code, tdt = L.DTYPES['float16']
    rows, c = 4195000, 2
    src = dev(L.randn32((rows, c), 33))
    one = lowp.dropout_cast_pad16(code, tdt, src, 0.2, 77)
    mask = ops.dropout_mask((rows, c), 0.2, 77, DEV)
    three = lowp.cast_pad16(code, tdt, ops.dropout_apply(src, mask, 0.2))
    assert torch.equal(one.view(torch.int16), three.view(torch.int16))
    kept = float(mask.float().mean())
    assert abs(kept - 0.8) < 1e-3 and bool((one[:, :c][mask == 0] == 0).all())
