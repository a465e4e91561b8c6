"""-m gpu: no result depends on bytes nobody wrote (the twin of tests/test_guard_gpu.py, which proves that nothing WRITES outside its
buffers).

The contract (include/bts_hip.h): a result is a function of the operand views and of nothing else -- not of the contents of a workspace,
of an output that is not accumulated into, of channels outside a view (ld > C), or of memory before or behind a tensor.

Every case runs twice in this process on the same seeds under the allocator of tests/guard_alloc.py: first with every `torch.empty`,
exact-size workspace, guard band, slab neighbour channel and non-accumulated output filled with the byte 0x00, then with 0xFF, which reads
NaN in fp16, bf16, fp32 and fp64 (and -1 in the integer types).  NaN survives a multiplication by a zero-padded weight, a sum and a
maximum, so a kernel that loads a lane it does not own and cancels it arithmetically, a finalize pass that sums a partial slot no workgroup
wrote, or a host path that hands `torch.empty` to an accumulating call shows as a non-finite or a different result.  Asserted, with no
tolerance (the engine's results are bitwise reproducible, which the zero-twice control below re-checks):
  * every defined result is finite in both runs;
  * every defined result is bit-identical between the two runs;
  * the guard bands, and the neighbour channels of every slab, still hold their fill byte for byte in both runs.
The 0xA5 of the guard test is nearly blind to reads: -2.9e-16 as fp32 / bf16, -0.022 as fp16."""
import pytest
import torch

from guard_alloc import POISON, install
from test_guard_gpu import FORMS, SHAPES, _fresh_model
from test_kernels_gpu import ROUTES, _route_env, rnd, wshape

pytestmark = pytest.mark.gpu

FILLS = (0x00, POISON)
INT_OF = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def dev():
    return torch.device('cuda', 0)


def keep(v):
    """a result, copied out of the guarded memory (engine Tensor, torch tensor or number)"""
    t = getattr(v, 't', None)
    if torch.is_tensor(t):
        v = t
    if not torch.is_tensor(v):
        return torch.tensor(float(v), dtype=torch.float64)
    return v.detach().to('cpu', copy=True).contiguous()


def bits(t):
    return t.contiguous().view(INT_OF[t.element_size()])


def assert_identical(a, b, tags=('0x00', '0xFF')):
    """every result finite in both runs and the same bits in both"""
    assert list(a) == list(b), (list(a), list(b))
    problems = []
    for k in a:
        x, y = a[k], b[k]
        if x.dtype != y.dtype or x.shape != y.shape:
            problems.append('%s: %s %s against %s %s' % (k, x.dtype, tuple(x.shape), y.dtype, tuple(y.shape)))
            continue
        if x.is_floating_point():
            for tag, t in zip(tags, (x, y)):
                bad = int((~torch.isfinite(t)).sum())
                if bad:
                    problems.append('%s: %d of %d elements are not finite with fill %s' % (k, bad, t.numel(), tag))
        diff = (bits(x) != bits(y)).reshape(-1)
        if bool(diff.any()):
            i = int(diff.nonzero()[0])
            problems.append('%s: %d of %d elements differ between the fills, first at flat index %d: %r against %r' % (
                k, int(diff.sum()), diff.numel(), i, x.reshape(-1)[i].item(), y.reshape(-1)[i].item()))
    assert not problems, '%d results depend on unowned bytes:\n  ' % len(problems) + '\n  '.join(problems)


def twin(case, fills=FILLS, buffers=1):
    """run case(guard, monkeypatch) -> {name: result} once per fill; the guard bands must be intact after each run, and the run must
    have drawn at least `buffers` buffers from the filled allocator"""
    out = []
    for fill in fills:
        with pytest.MonkeyPatch.context() as mp:
            g = install(mp, fill)
            res = case(g, mp)
            n = g.check()
            assert n >= buffers, (n, buffers)
        out.append(res)
    return out


def recorded(fn):
    from bts_amd import ops
    ops.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ops.profile_enable(False)
    return out, [r[0] for r in ops.profile_records(detail=True)]


def ran(names, want):
    return any(nm.startswith(want) for nm in names)


# ---- (a) fp32 training steps ---------------------------------------------------------------------------------------------
def _train_case(kw, shape, form):
    def case(g, mp):
        from bts_amd.data import synthetic_batch
        from bts_amd.util import DiceCoefficient, DiceVAELoss, ScheduledOptim, train_step
        for k, v in FORMS[form].items():
            mp.setenv(k, v)
        m = _fresh_model(kw, shape)
        latent = kw['base_filters'] * 2 ** (kw['depth'] - 2)
        x, y, _, _ = synthetic_batch(shape[0], shape[1:], latent=latent, seed=12)
        opt = ScheduledOptim(1e-4)
        opt(epoch=0)
        res = {}
        for i in (1, 2):        # the second step re-packs the weight images and re-uses the optimiser state
            loss, macro, micro = train_step(m, opt, DiceVAELoss(), DiceCoefficient(), x.cuda(), y.cuda())
            res['loss of step %d' % i], res['macro dice of step %d' % i], res['micro dice of step %d' % i] = keep(loss), keep(macro), keep(micro)
        torch.cuda.synchronize()
        for i, p in enumerate(m.trainable_variables):
            res['variable %d %s' % (i, p.name)] = keep(p.t)
        assert len(opt._state) >= 1
        for i, (mom1, mom2) in enumerate(opt._state.values()):
            res['Adam m %d' % i], res['Adam v %d' % i] = keep(mom1), keep(mom2)
        return res
    return case


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('kw,shape', SHAPES, ids=['f8-8x16x24', 'f16-n2-32x16x40', 'cli-16x16x32'])
def test_fp32_train_steps_do_not_depend_on_unowned_bytes(kw, shape, form):
    """two train_steps of the guard test's models through every conv-form switch set: both losses and metrics, every trainable variable
    and both Adam moments after step 2"""
    assert_identical(*twin(_train_case(kw, shape, form), buffers=200))      # (the step allocated: saved activations, gradients, scratch)


# ---- (b) the 16-bit engine -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_16bit_forward_and_train_steps_do_not_depend_on_unowned_bytes(dtype):
    """LowPrecisionForward on a ragged sub-volume, then two LowPrecisionTrainer steps: after an overflow step of real fp16 training the
    blocks the caching allocator hands out hold Inf / NaN, so one kernel reading such bytes would make the next step overflow too"""
    def case(g, mp):
        from bts_amd import lowp
        from bts_amd.data import synthetic_batch
        from bts_amd.lowp_train import LowPrecisionTrainer
        from bts_amd.util import DiceCoefficient, ScheduledOptim
        kw, shape = dict(base_filters=16, groups=8, reduction=2, depth=3), (2, 32, 32, 48)
        m = _fresh_model(kw, shape)
        x, y, _, _ = synthetic_batch(shape[0], shape[1:], latent=32, seed=7)
        res = {'forward': keep(lowp.LowPrecisionForward(m, dtype)(x[:1, :24, :, :40].contiguous()))}
        opt = ScheduledOptim(1e-4)
        opt(epoch=0)
        tr = LowPrecisionTrainer(m, dtype)
        for i in (1, 2):
            loss, macro, micro = tr.step(opt, DiceCoefficient(), x, y)
            res['loss of step %d' % i], res['macro dice of step %d' % i], res['micro dice of step %d' % i] = keep(loss), keep(macro), keep(micro)
        tr.settle()
        torch.cuda.synchronize()
        assert tr.skipped_steps == 0, tr.skipped_steps
        res['skipped steps'] = keep(tr.skipped_steps)
        res['flat gradients'] = keep(m.flat_grads)
        for i, p in enumerate(m.trainable_variables):
            res['variable %d %s' % (i, p.name)] = keep(p.t)
        return res
    assert_identical(*twin(case, buffers=200))


# ---- (c) 16-bit kernels with tiling floors, on slab views ----------------------------------------------------------------
@pytest.mark.parametrize('dtype', ['float16', 'bfloat16'])
def test_16bit_kernels_with_tiling_floors_do_not_depend_on_unowned_bytes(dtype):
    """the call list and shapes of test_16bit_kernels_with_tiling_floors_stay_inside_slab_views: every operand a channel slice of a
    slab whose 8 lead and 16 tail channels hold the fill, every output that is not accumulated into the fill before its call"""
    def case(g, mp):
        from bts_amd import lowp, ops
        code, tdt = lowp.DTYPES[dtype]
        D = dev()
        gen = torch.Generator().manual_seed(2)
        res = {}

        def slab(n, d, h, w, c, written=True):
            buf, v = g.slab((n, d, h, w, c), tdt, D, lead=8, tail=16, values=torch.randn((n, d, h, w, c), generator=gen) if written else None)
            return buf, v, 8, c

        def vals(shape, scale=1.0):
            return (torch.randn(shape, generator=gen) * scale).to(D)

        # LDS-DMA stride-1 conv: ragged 32-wide and 16-wide tiles, both work splits; its accumulating data gradient
        variants = set()
        for i, (n, d, h, w, cin, cout) in enumerate([(1, 16, 20, 40, 32, 32), (2, 16, 24, 20, 16, 64), (1, 32, 24, 20, 64, 64)]):
            xb, xv, _, _ = slab(n, d, h, w, cin)
            yb, yv, yl, yc = slab(n, d, h, w, cout, written=False)
            wt, b = vals((3, 3, 3, cin, cout), 0.05), vals((cout,))
            _, names = recorded(lambda: lowp.conv(ops.K3S1, code, tdt, xv, lowp.pack(ops.K3S1, code, wt, cin, cout), b, cout, out=yv))
            assert ran(names, 'lp_s1d_kernel'), names
            variants.update(nm[len('lp_s1d_kernel'):] for nm in names if nm.startswith('lp_s1d_kernel<'))
            res['s1d %d y' % i] = keep(yv)
            lowp.conv_bwd_data(ops.K3S1, code, yv, lowp.pack(ops.K3S1, code, wt, cin, cout, role=ops.ROLE_BWD), xv, True)
            res['s1d %d dx' % i] = keep(xv)
            assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, cin)
        assert {v[1] for v in variants} == {'0', '1'} and {v[3] for v in variants} == {'4', '5'}, variants      # <work split, log2 tile width>
        # streaming 1x1x1 (ragged last block) and its accumulating data gradient
        xb, xv, _, _ = slab(2, 9, 13, 20, 48)
        yb, yv, yl, yc = slab(2, 9, 13, 20, 32, written=False)
        wt = vals((1, 1, 1, 48, 32), 0.1)
        _, names = recorded(lambda: lowp.conv(ops.K1, code, tdt, xv, lowp.pack(ops.K1, code, wt, 48, 32), None, 32, out=yv))
        assert ran(names, 'lp_k1_kernel'), names
        res['k1 y'] = keep(yv)
        lowp.conv_bwd_data(ops.K1, code, yv, lowp.pack(ops.K1, code, wt, 48, 32, role=ops.ROLE_BWD), xv, True)
        res['k1 dx'] = keep(xv)
        assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, 48)
        # transposed form (ragged coarse grid) and the stride-2 conv's data gradient
        xb, xv, _, _ = slab(1, 8, 11, 24, 32)
        yb, yv, yl, yc = slab(1, 16, 22, 48, 64, written=False)
        wt = vals((3, 3, 3, 64, 32), 0.05)
        _, names = recorded(lambda: lowp.conv(ops.K3S2T, code, tdt, xv, lowp.pack(ops.K3S2T, code, wt, 32, 64), None, 64, out=yv))
        assert ran(names, 'lp_up_kernel'), names
        res['transposed y'] = keep(yv)
        assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, 32)
        wt2 = vals((3, 3, 3, 64, 32), 0.05)                     # stride-2 conv 64 -> 32: dy on (8, 11, 24)
        _, names = recorded(lambda: lowp.conv_bwd_data(ops.K3S2, code, xv, lowp.pack(ops.K3S2, code, wt2, 64, 32, role=ops.ROLE_BWD), yv, True))
        assert ran(names, 'lp_up_kernel'), names
        res['stride-2 dx'] = keep(yv)
        assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, 32)
        # strided weight gradients of both kinds: accumulating into zeros, and a first write into the fill
        dw = g.zeros((3, 3, 3, 64, 32), dtype=torch.float32, device=D)
        db = g.zeros((32,), dtype=torch.float32, device=D)
        dyc = vals((1, 8, 11, 24, 32)).to(tdt)
        ok, names = recorded(lambda: lowp.conv_bwd_weight(ops.K3S2, code, yv, dyc, dw, db, accumulate=True))
        assert ok and ran(names, 'lp_wgs_kernel'), names
        dwt = g.empty((3, 3, 3, 64, 32), dtype=torch.float32, device=D)
        ok, names = recorded(lambda: lowp.conv_bwd_weight(ops.K3S2T, code, xv, yv.contiguous(), dwt, None, accumulate=False))
        assert ok and ran(names, 'lp_wgs_kernel'), names
        res['wgs stride-2 dw'], res['wgs stride-2 db'], res['wgs transposed dw'] = keep(dw), keep(db), keep(dwt)
        assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, 32)
        # z-marching stride-1 conv for few channels: several columns, z chunks with a ragged last one, accumulating data gradient
        for i, (n, d, h, w, cin, cout) in enumerate([(1, 37, 16, 96, 32, 16), (2, 16, 32, 64, 16, 32)]):
            xb, xv, _, _ = slab(n, d, h, w, cin)
            yb, yv, yl, yc = slab(n, d, h, w, cout, written=False)
            wt, b = vals((3, 3, 3, cin, cout), 0.05), vals((cout,))
            _, names = recorded(lambda: lowp.conv(ops.K3S1, code, tdt, xv, lowp.pack(ops.K3S1, code, wt, cin, cout), b, cout, out=yv))
            assert ran(names, 'lp_s1z_kernel'), names
            res['s1z %d y' % i] = keep(yv)
            if cin == cout or cout % 16 == 0:
                lowp.conv_bwd_data(ops.K3S1, code, yv, lowp.pack(ops.K3S1, code, wt, cin, cout, role=ops.ROLE_BWD), xv, True)
                res['s1z %d dx' % i] = keep(xv)
            assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, cin)
        # LDS-tiled stride-2 conv of the 32-channel top level, and the whole-row-load gather on a grid whose last quad row ends the tensor
        for (n, d, h, w, cin, cout, sym) in [(2, 60, 44, 72, 32, 24, 'lp_s2t_kernel'), (1, 48, 40, 72, 64, 64, 'lp_conv_gather_kernel')]:
            xb, xv, _, _ = slab(n, d, h, w, cin)
            yb, yv, yl, yc = slab(n, d // 2, h // 2, w // 2, cout, written=False)
            wt, b = vals((3, 3, 3, cin, cout), 0.05), vals((cout,))
            _, names = recorded(lambda: lowp.conv(ops.K3S2, code, tdt, xv, lowp.pack(ops.K3S2, code, wt, cin, cout), b, cout, out=yv))
            assert ran(names, sym), names
            res[sym + ' y'] = keep(yv)
            assert g.untouched(yb, yl, yc) and g.untouched(xb, 8, cin)
        # streaming stride-1 weight gradient: x a slab view, an exact-size workspace
        xb, xv, _, _ = slab(1, 37, 16, 32, 64)
        dyc = vals((1, 37, 16, 32, 16)).to(tdt)
        dw3 = g.zeros((3, 3, 3, 64, 16), dtype=torch.float32, device=D)
        ok, names = recorded(lambda: lowp.conv_bwd_weight(ops.K3S1, code, xv, dyc, dw3, None, accumulate=True))
        assert ok and ran(names, 'lp_wgd_kernel'), names
        res['wgd dw'] = keep(dw3)
        assert g.untouched(xb, 8, 64)
        # all images in one launch into image buffers of exactly bts_lp_packed_bytes that hold the fill
        entries = []
        for kind, role, cin, cout in ((ops.K3S1, ops.ROLE_FWD, 32, 24), (ops.K3S1, ops.ROLE_BWD, 16, 64), (ops.K1, ops.ROLE_FWD, 48, 8), (ops.K3S2T, ops.ROLE_FWD, 32, 16)):
            k = 1 if kind == ops.K1 else 3
            wsrc = vals((k, k, k, cout, cin) if kind == ops.K3S2T else (k, k, k, cin, cout))
            nbytes = lowp.lib().query('bts_lp_packed_bytes', kind, role, cin, cout)
            entries.append((kind, role, wsrc, g.empty((nbytes // 2,), dtype=torch.int16, device=D), cin, cout, cin, 0, 0))
        lowp.PackTable().run(code, entries)
        for i, e in enumerate(entries):
            res['packed image %d' % i] = keep(e[3])
        return res
    assert_identical(*twin(case))


# ---- (d) fp32 kernels on slab views ----------------------------------------------------------------------------------------
def _f32_slab(g, shape, lead, tail, values=None):
    buf, v = g.slab(shape, torch.float32, dev(), lead=lead, tail=tail, values=values)
    return buf, v, lead, shape[-1]


@pytest.mark.parametrize('route', sorted(ROUTES))
def test_fp32_conv_routes_on_slab_views_do_not_depend_on_unowned_bytes(route):
    """each route of the fp32 dispatch at its shape and switches: forward and data gradient (first write, then accumulating) with x, dy and
    the outputs as channel slices of slabs with ld = C + 8 (views at float offset 4 or 8: the alignment cases of the plan are kept, so the
    route's kernel still takes the forward call), exact-size poisoned workspaces"""
    kind, dims, cin, cout, env, want = ROUTES[route]

    def case(g, mp):
        from bts_amd import ops
        _route_env(mp, env)
        D = dev()
        n, (d, h, w) = 1, dims
        oshape = ops.conv_out_shape(kind, (n, d, h, w, cin), cout)
        xb, xv, xl, _ = _f32_slab(g, (n, d, h, w, cin), 4, 4, rnd((n, d, h, w, cin), 91))
        yb, yv, yl, _ = _f32_slab(g, oshape, 8, 0)
        wt, b = rnd(wshape(kind, cin, cout), 92, 0.2).to(D), rnd((cout,), 93).to(D)
        res = {}
        wp = ops.conv_pack(kind, ops.ROLE_FWD, wt, cin, cout)
        _, names = recorded(lambda: ops.conv_fwd(kind, xv, wp, b, cout, out=yv))
        assert ran(names, want), (route, names)
        res['y'] = keep(yv)
        dyb, dyv, dyl, _ = _f32_slab(g, oshape, 4, 4, rnd(oshape, 94))
        dxb, dxv, dxl, _ = _f32_slab(g, (n, d, h, w, cin), 8, 0)
        wpb = ops.conv_pack(kind, ops.ROLE_BWD, wt, cin, cout)
        _, names = recorded(lambda: ops.conv_bwd_data(kind, dyv, wpb, dxv, accumulate=False))
        res['dx by ' + ' + '.join(names)] = keep(dxv)
        ops.conv_bwd_data(kind, dyv, wpb, dxv, accumulate=True)
        res['dx accumulated'] = keep(dxv)
        torch.cuda.synchronize()
        assert g.untouched(xb, xl, cin) and g.untouched(yb, yl, cout) and g.untouched(dyb, dyl, cout) and g.untouched(dxb, dxl, cin)
        return res
    assert_identical(*twin(case))


WGRAD_PATHS = {
    # kind, N, (D, H, W), Cin, Cout, switches, kernel, whether it must (True) or must not (False) run
    'wgw': (1, 1, (4, 8, 32), 32, 32, {}, 'wgw_kernel', True),
    'direct': (1, 1, (4, 8, 32), 32, 32, {'BTS_WGW': '0'}, 'wgw_kernel', False),
    'k1w': (0, 1, (33, 31, 35), 64, 24, {}, 'k1w_kernel', True),
}


@pytest.mark.parametrize('path', sorted(WGRAD_PATHS))
def test_fp32_weight_gradient_paths_on_slab_views_do_not_depend_on_unowned_bytes(path):
    """the three paths of tests/test_wgw_gpu.py (Winograd form, direct kernel, streaming 1x1x1 form): x and dy channel slices of poisoned
    slabs, dw and db poisoned before the first write, then accumulated into; exact-size poisoned workspace (split partials + finalize)"""
    kind, n, dims, cin, cout, env, sym, must = WGRAD_PATHS[path]

    def case(g, mp):
        from bts_amd import ops
        for k in ('BTS_WGW', 'BTS_K1W', 'BTS_WINO'):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        D = dev()
        d, h, w = dims
        k = 1 if kind == 0 else 3
        xb, xv, xl, _ = _f32_slab(g, (n, d, h, w, cin), 8, 0, rnd((n, d, h, w, cin), 41))
        dyb, dyv, dyl, _ = _f32_slab(g, (n, d, h, w, cout), 4, 4, rnd((n, d, h, w, cout), 42))
        dw = g.empty((k, k, k, cin, cout), dtype=torch.float32, device=D)
        db = g.empty((cout,), dtype=torch.float32, device=D)
        _, names = recorded(lambda: ops.conv_bwd_weight(kind, xv, dyv, dw, db))
        assert ran(names, sym) == must, (path, names)
        res = {'dw': keep(dw), 'db': keep(db)}
        ops.conv_bwd_weight(kind, xv, dyv, dw, db, accumulate=True)
        res['dw accumulated'], res['db accumulated'] = keep(dw), keep(db)
        dw0 = g.empty((k, k, k, cin, cout), dtype=torch.float32, device=D)
        ops.conv_bwd_weight(kind, xv, dyv, dw0, None)
        res['dw without db'] = keep(dw0)
        torch.cuda.synchronize()
        assert g.untouched(xb, xl, cin) and g.untouched(dyb, dyl, cout)
        return res
    assert_identical(*twin(case))


@pytest.mark.parametrize('form', ['tiled', 'w3', 'wino'])
def test_fp32_fused_pairs_on_slab_views_do_not_depend_on_unowned_bytes(form):
    """the fused shortcut pair (conv3x3x3 + conv1x1x1 of one x) and the data-gradient pair, with the tiled kernel taking both parts and
    with either Winograd form taking the 3x3x3 part (then a 1x1x1 launch of its own follows)"""
    env = {'tiled': {}, 'w3': dict(BTS_WINO_MIN_WGS='1', BTS_W3='1'), 'wino': dict(BTS_WINO_MIN_WGS='1', BTS_W3='0')}[form]

    def case(g, mp):
        from bts_amd import ops
        _route_env(mp, env)
        D = dev()
        n, (d, h, w), cin, cout = 1, (8, 8, 32), 32, 32
        xb, xv, xl, _ = _f32_slab(g, (n, d, h, w, cin), 4, 4, rnd((n, d, h, w, cin), 50))
        w3, b3 = rnd((3, 3, 3, cin, cout), 51, 0.2).to(D), rnd((cout,), 52).to(D)
        w1, b1 = rnd((1, 1, 1, cin, cout), 53, 0.3).to(D), rnd((cout,), 54).to(D)
        wp3, wp1 = ops.conv_pack(ops.K3S1, ops.ROLE_FWD, w3, cin, cout), ops.conv_pack(ops.K1, ops.ROLE_FWD, w1, cin, cout)
        out, names = recorded(lambda: ops.conv_fwd_fused2(xv, wp3, b3, wp1, b1, cout))
        assert out is not None, 'the shortcut pair is fusable at this shape'
        if form != 'tiled':
            assert ran(names, form + '_kernel'), names
        res = {'fused c1': keep(out[0]), 'fused res': keep(out[1])}
        dyb, dyv, dyl, _ = _f32_slab(g, (n, d, h, w, cout), 4, 4, rnd((n, d, h, w, cout), 84))
        d2b, d2v, d2l, _ = _f32_slab(g, (n, d, h, w, cout), 8, 0, rnd((n, d, h, w, cout), 85))
        dxb, dxv, dxl, _ = _f32_slab(g, (n, d, h, w, cin), 8, 0)
        wpb3, wpb1 = ops.conv_pack(ops.K3S1, ops.ROLE_BWD, w3, cin, cout), ops.conv_pack(ops.K1, ops.ROLE_BWD, w1, cin, cout)
        _, names = recorded(lambda: ops.conv_bwd_data_pair(dyv, wpb3, d2v, wpb1, dxv, False))
        if form != 'tiled':
            assert ran(names, form + '_kernel'), names
        res['pair dx'] = keep(dxv)
        ops.conv_bwd_data_pair(dyv, wpb3, d2v, wpb1, dxv, True)
        res['pair dx accumulated'] = keep(dxv)
        torch.cuda.synchronize()
        assert g.untouched(xb, xl, cin) and g.untouched(dyb, dyl, cout) and g.untouched(d2b, d2l, cout) and g.untouched(dxb, dxl, cin)
        return res
    assert_identical(*twin(case))


def test_fp32_conv_with_groupnorm_statistics_does_not_depend_on_unowned_bytes():
    """bts_conv3d_fwd_gn at (1, (6, 10, 14), 12 -> 20, G = 2): Cin is no multiple of 8 and the z extent holds no whole tiles per group, so the
    statistics come through the library's own bts_gn_stats fallback over the workspace; x a slab view, with and without the fused form"""
    def case(g, mp):
        from bts_amd import ops
        _route_env(mp, {})
        D = dev()
        n, (d, h, w), cin, cout, groups = 1, (6, 10, 14), 12, 20, 2
        xb, xv, xl, _ = _f32_slab(g, (n, d, h, w, cin), 4, 4, rnd((n, d, h, w, cin), 61))
        wt, b = rnd((3, 3, 3, cin, cout), 62, 0.2).to(D), rnd((cout,), 63).to(D)
        wp = ops.conv_pack(ops.K3S1, ops.ROLE_FWD, wt, cin, cout)
        res = {}
        for tag in ('', ' unfused'):
            if tag:
                mp.setenv('BTS_IGEMM_NOGNFUSE', '1')
            y, mean, rstd = ops.conv_fwd_gn(ops.K3S1, xv, wp, b, cout, groups, 1e-5)
            res['y' + tag], res['mean' + tag], res['rstd' + tag] = keep(y), keep(mean), keep(rstd)
        torch.cuda.synchronize()
        assert g.untouched(xb, xl, cin)
        return res
    assert_identical(*twin(case))


@pytest.mark.parametrize('shape', [(2, 8, 16, 16, 32), (1, 8, 8, 16, 8), (1, 6, 10, 10, 16)], ids=['n2-8x16x16-32', '8x8x16-8', '6x10x10-16'])
def test_fp32_norm_gate_and_sampler_kernels_on_slab_views_do_not_depend_on_unowned_bytes(shape):
    """the kernels around the convolutions, each called on its own with dout / out / dx as channel slices of poisoned slabs, poisoned
    outputs and parameter gradients (first write) and exact-size poisoned workspaces: column sums, the gate's MLP, GroupNorm statistics /
    apply / backward in both modes, the block epilogue, the gate backward, the fused gate + GroupNorm-2 backward (declined by the third
    shape, which runs the separate calls only), max pooling and nearest up-sampling with their gradients, the strided add"""
    def case(g, mp):
        from bts_amd import ops
        D = dev()
        n, d, h, w, f = shape
        v = d * h * w
        groups, r = 8, max(f // 8, 1)          # (the gate kernels take power-of-two channel counts)
        gen = torch.Generator().manual_seed(f + d)

        def vals(*s, scale=1.0, shift=0.0):
            return (shift + scale * torch.randn(s, generator=gen)).to(D)

        def empties(*like):
            return [g.empty(tuple(t.shape), dtype=torch.float32, device=D) for t in like]
        res_, c2 = vals(*shape), vals(*shape)
        dob, dout, dol, _ = _f32_slab(g, shape, 8, 8, torch.randn(shape, generator=gen))
        w1, w2, wsp = vals(f, r, scale=0.3), vals(r, f, scale=0.3), vals(f, scale=0.3)
        gamma, beta = vals(f, scale=0.3, shift=1.0), vals(f, scale=0.2)
        out = {}
        gap = ops.colsum(res_, scale=1.0 / v)
        hbuf, ch = ops.se_mlp_fwd(gap, w1, w2)
        out['gap'], out['h'], out['ch'] = keep(gap), keep(hbuf), keep(ch)
        out['colsum of a view'], out['colsum of a view over n'] = keep(ops.colsum(dout)), keep(ops.colsum(dout, sum_over_n=True))
        for mode in (ops.GN_SLAB, ops.GN_CHANNEL):
            mean, rstd = ops.gn_stats(c2, groups, mode)
            yb, yv, yl, _ = _f32_slab(g, shape, 4, 4)
            ops.gn_apply(c2, gamma, beta, mean, rstd, groups, mode, 1, out=yv)
            dgam, dbet = empties(gamma, beta)
            dx = ops.gn_bwd(c2, dout, gamma, beta, mean, rstd, dgam, dbet, groups, mode, 1)
            for k, t in (('mean', mean), ('rstd', rstd), ('y', yv), ('dx', dx), ('dgamma', dgam), ('dbeta', dbet)):
                out['gn mode %d %s' % (mode, k)] = keep(t)
            torch.cuda.synchronize()
            assert g.untouched(yb, yl, f)
        mean, rstd = ops.gn_stats(c2, groups, ops.GN_SLAB)
        eb, ev, el, _ = _f32_slab(g, shape, 4, 4)
        sp = ops.block_epilogue_fwd(res_, c2, ev, wsp, ch, gamma, beta, mean, rstd, groups, ops.GN_SLAB)
        out['epilogue'], out['sp'] = keep(ev), keep(sp)
        dw1, dw2, dwsp = empties(w1, w2, wsp)
        out['gate dres'] = keep(ops.se_bwd(dout, res_, sp, gap, hbuf, ch, w1, w2, wsp, dw1, dw2, dwsp))
        out['gate dw1'], out['gate dw2'], out['gate dwsp'] = keep(dw1), keep(dw2), keep(dwsp)
        takes = ops.block_bwd_takes(res_, r, groups, dout, c2)
        assert takes == (v % 1024 == 0), (shape, takes)      # (600 voxels: units that are not whole 1024-element chunks)
        if takes:
            grads = empties(w1, w2, wsp, gamma, beta)
            dres, dc2 = ops.block_bwd(dout, res_, c2, sp, gap, hbuf, ch, w1, w2, wsp, gamma, beta, mean, rstd, groups, *grads)
            for k, t in zip(('dres', 'dc2', 'dw1', 'dw2', 'dwsp', 'dgamma', 'dbeta'), [dres, dc2] + grads):
                out['fused block backward ' + k] = keep(t)
        if d % 2 == 0 and h % 2 == 0 and w % 2 == 0:
            y, idx = ops.maxpool2_fwd(dout)
            pb, pv, pl, _ = _f32_slab(g, shape, 8, 0)
            ops.maxpool2_bwd(y, idx, pv, False)
            out['pool y'], out['pool idx'], out['pool dx'] = keep(y), keep(idx), keep(pv)
            ops.maxpool2_bwd(y, idx, pv, True)
            out['pool dx accumulated'] = keep(pv)
            torch.cuda.synchronize()
            assert g.untouched(pb, pl, f)
        ub, uv, ul, _ = _f32_slab(g, (n, 2 * d, 2 * h, 2 * w, f), 4, 4)
        ops.upsample2_fwd(dout, out=uv)
        out['upsampled'], out['upsample dx'] = keep(uv), keep(ops.upsample2_bwd(uv))
        ab, av, al, _ = _f32_slab(g, shape, 4, 8)
        ops.add_strided(av, dout, False)
        out['strided copy'] = keep(av)
        ops.add_strided(av, dout, True)
        out['strided add'] = keep(av)
        torch.cuda.synchronize()
        assert g.untouched(dob, dol, f) and g.untouched(eb, el, f) and g.untouched(ub, ul, f) and g.untouched(ab, al, f)
        return out
    assert_identical(*twin(case))


# ---- (e) inference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype,kw,build,vol,res_', [
    ('float32', dict(base_filters=8, groups=2, reduction=2, depth=3), (1, 16, 16, 24), (13, 9, 16), 8),      # the small model of test_infer_gpu.py
    ('float16', dict(base_filters=16, groups=8, reduction=2, depth=3), (1, 16, 16, 24), (13, 9, 20), 4),     # 16-bit storage needs 16 filters
], ids=['float32', 'float16'])
def test_segment_volume_does_not_depend_on_unowned_bytes(dtype, kw, build, vol, res_):
    """pad -> 8-way flip TTA -> mean -> mask -> labels on a volume whose extents need padding: probabilities and label map"""
    def case(g, mp):
        from bts_amd import infer
        m = _fresh_model(kw, build)
        gen = torch.Generator().manual_seed(21)
        x = torch.randn(vol + (2,), generator=gen) * 40.0 + 100.0
        mask = (torch.rand(vol + (1,), generator=gen) > 0.15).float()
        x = x * mask
        mean, std = torch.tensor([95.0, 110.0]), torch.tensor([35.0, 45.0])
        y, lab = infer.segment_volume(m, x.to(dev()), mask.to(dev()), mean, std, res_, compute_dtype=dtype)
        torch.cuda.synchronize()
        assert tuple(y.shape) == vol + (3,) and tuple(lab.shape) == vol and lab.dtype == torch.uint8
        return {'probabilities': keep(y), 'labels': keep(lab)}
    assert_identical(*twin(case))


def test_scan_and_input_batch_kernels_do_not_depend_on_unowned_bytes():
    """the kernels around the networks, whose outputs and workspaces come from `torch.empty` too: spline prefilter and zoom (every
    order, padding, mask, normalisation), flip / normalise / accumulate, the TTA finish, channel moments, the skull-strip hand-over,
    the input batch in both layouts and every intensity stage on it (blur out of place through the workspace, statistics passes)"""
    def case(g, mp):
        from bts_amd import ops
        D = dev()
        gen = torch.Generator().manual_seed(5)
        res = {}
        x = (torch.randn((9, 11, 13, 2), generator=gen) * 40.0 + 100.0).to(D)
        mean, std = torch.tensor([95.0, 110.0], device=D), torch.tensor([35.0, 45.0], device=D)
        coef = ops.spline_prefilter3d(x)
        res['spline coefficients'] = keep(coef)
        for order, src in ((3, coef), (1, x), (0, x)):
            y, m = ops.zoom3d(src, (12, 9, 17), order=order, pad_to=(16, 16, 24), want_mask=True, mean=mean if order == 3 else None,
                              std=std if order == 3 else None)
            res['zoom order %d' % order], res['zoom order %d mask' % order] = keep(y), keep(m)
        res['zoom down'] = keep(ops.zoom3d(coef, (5, 7, 6)))
        vol = torch.randn((2, 5, 6, 7, 3), generator=gen).to(D)
        m3, s3 = torch.tensor([0.1, -0.2, 0.3], device=D), torch.tensor([1.5, 0.5, 2.0], device=D)
        for flip in (0, 3, 7):
            res['flip %d' % flip], res['flip %d normalised' % flip] = keep(ops.flip_affine(vol, flip)), keep(ops.flip_affine(vol, flip, m3, s3))
        acc = ops.flip_affine(vol, 5, scale=0.125)
        ops.flip_affine(vol, 2, scale=0.125, out=acc, accumulate=True)
        res['flip accumulated'] = keep(acc)
        bm = (torch.rand((2, 5, 6, 7, 1), generator=gen) > 0.3).float().to(D)
        y, lab = ops.tta_finish(torch.sigmoid(vol), bm, 0.5)
        res['masked probabilities'], res['labels'] = keep(y), keep(lab)
        mom = ops.channel_moments(vol)
        res['channel mean'], res['channel variance'] = keep(mom[0]), keep(mom[1])
        xo, mo = ops.skull_strip(torch.randn((6, 7, 9, 2), generator=gen).to(D), torch.rand((6, 7, 9, 1), generator=gen).to(D),
                                 (torch.rand((6, 7, 9, 1), generator=gen) > 0.2).float().to(D), (5, 6, 7), (8, 8, 16))
        res['skull-stripped'], res['skull-strip mask'] = keep(xo), keep(mo)
        xs = [(torch.randn((16, 14, 18, 2), generator=gen) * 30.0 + 50.0).to(D) for _ in range(2)]
        ys = [torch.randint(0, 4, (16, 14, 18, 1), generator=gen).float().to(D) for _ in range(2)]
        var = [ops.channel_moments(t)[1] for t in xs]
        every = ops.INTENSITY_NOISE | ops.INTENSITY_BLUR | ops.INTENSITY_BRIGHT | ops.INTENSITY_CONTRAST | ops.INTENSITY_GAMMA
        params = [[(every, 0.1, 0.8, 1.1, 1.2, 1.3), (every | ops.INTENSITY_INVERT, 0.05, 1.2, 0.9, 0.8, 0.7)],
                  [(ops.INTENSITY_BLUR | ops.INTENSITY_CONTRAST, 0.0, 0.6, 1.0, 1.1, 1.0), (0, 0.0, 1.0, 1.0, 1.0, 1.0)]]
        for cf in (False, True):
            bx, by = ops.augment_batch(xs, ys, var, (12, 10, 14), [(2, 3, 1), (4, 4, 4)], [0, 5], [[0.1, -0.1], [0.0, 0.05]],
                                       [[1.1, 0.9], [1.0, 1.05]], 3, channels_first=cf)
            tag = ' channels first' if cf else ''
            res['batch x' + tag], res['batch y' + tag] = keep(bx), keep(by)
            ops.intensity_batch(bx, params, [(1, 2), (3, 4)], cf)
            res['batch x after the intensity stages' + tag] = keep(bx)
        return res
    assert_identical(*twin(case))


# ---- (f) controls ----------------------------------------------------------------------------------------------------------
def test_control_two_zero_filled_runs_are_bit_identical():
    """the determinism every comparison above rests on: the same case twice with fill 0x00"""
    kw, shape = SHAPES[0]
    assert_identical(*twin(_train_case(kw, shape, 'default'), fills=(0x00, 0x00), buffers=200), tags=('0x00', '0x00 again'))


def test_control_the_harness_notices_a_read_of_poisoned_memory():
    """negative control without any fault: a library reduction over an `empty` buffer nobody wrote returns what the fill reads as, and
    the comparison of the two runs raises"""
    def case(g, mp):
        from bts_amd import ops
        buf = g.empty((2, 4, 4, 4, 8), dtype=torch.float32, device=dev())
        return {'colsum': keep(ops.colsum(buf))}
    zero, poisoned = twin(case)
    assert tuple(zero['colsum'].shape) == (2, 8)
    assert bool((zero['colsum'] == 0).all()) and bool(torch.isnan(poisoned['colsum']).all())
    with pytest.raises(AssertionError, match='depend on unowned bytes'):
        assert_identical(zero, poisoned)
    assert_identical(zero, zero)


def test_control_the_harness_notices_a_neighbour_cancelled_by_zero_weights():
    """negative control for the slab cases: a convolution whose input view is made to TAKE IN four neighbour channels that hold the fill,
    with all-zero weights for them -- what a kernel does that loads a lane it does not own and cancels it by a zero-padded weight.  With
    finite neighbours (the 5.0 / 7.0 / randn of the other slab tests) the result would be unchanged; under the poison it is NaN, and the
    comparison raises"""
    def case(g, mp):
        from bts_amd import ops
        _route_env(mp, dict(BTS_WINO='0'))
        D = dev()
        n, d, h, w, cin, cout = 1, 8, 8, 32, 32, 32
        buf, _ = g.slab((n, d, h, w, cin), torch.float32, D, lead=4, tail=4, values=rnd((n, d, h, w, cin), 91))
        wt = rnd((3, 3, 3, cin + 4, cout), 92, 0.2)
        wt[:, :, :, :4, :] = 0.0          # the four lead channels of the slab are not this view's: cancelled, not masked
        wp = ops.conv_pack(ops.K3S1, ops.ROLE_FWD, wt.to(D), cin + 4, cout)
        return {'y': keep(ops.conv_fwd(ops.K3S1, buf[..., :cin + 4], wp, None, cout))}
    zero, poisoned = twin(case)
    assert bool(torch.isfinite(zero['y']).all()) and float(zero['y'].abs().max()) > 0 and bool(torch.isnan(poisoned['y']).all())
    with pytest.raises(AssertionError, match='depend on unowned bytes'):
        assert_identical(zero, poisoned)
