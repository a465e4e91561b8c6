"""CPU: the host-only planning code of the C-ABI library (split-K plans, workspace sizing, dispatch thresholds, descriptor tables) walked
over every layer shape of the three single-GPU BASELINE configurations (configs[1]: 1 x 128^3, configs[2]: 8 x 128^3, configs[4]:
1 x 160x192x160; CLI-default model) and the option matrix of row f-4 (max-pool / linear samplers change which kinds occur,
not the shapes).  No GPU, no compute call: every function here returns before any HIP call.  tests/test_asan_host.py runs this file and
tests/test_abi.py once more against the AddressSanitizer + UBSan build of the host code (`make -C .../csrc asan`).

What is asserted: the queries are total (no crash, no negative size other than the documented -1 "this form declines the shape"),
deterministic (the same answer twice) and monotone where the ABI says so (a workspace for N samples is never smaller than for one)."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)      # tests/lowp_ref.py

GRIDS = [(1, 128, 128, 128), (8, 128, 128, 128), (1, 160, 192, 160)]
F, DEPTH, G, R = 32, 4, 8, 8


def layer_shapes(n, d, h, w):
    """(kind, N, D, H, W, Cin, Cout) of every conv of the CLI-default model on an (n, d, h, w) volume: encoder.py:43-67,
    decoder.py:38-63, vae.py:53-99"""
    K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
    out = []

    def block(lvl, cin, f):
        s = (n, d >> lvl, h >> lvl, w >> lvl)
        out.append((K1,) + s + (cin, f))
        out.append((K3S1,) + s + (cin, f))
        out.append((K3S1,) + s + (f, f))
        out.append((K1,) + s + (f, 1))
    for lvl in range(DEPTH):
        f = F << lvl
        cin = 2 if lvl == 0 else f // 2
        for b in range(lvl + 1):
            block(lvl, cin if b == 0 else f * (b + 1) if lvl else f, f)
        if lvl < DEPTH - 1:
            out.append((K3S2, n, d >> lvl, h >> lvl, w >> lvl, f * (lvl + 1), f))
    top = F << (DEPTH - 1)
    for lvl in range(DEPTH - 2, -1, -1):       # decoder
        f = F << lvl
        cin = top * DEPTH if lvl == DEPTH - 2 else f * 2
        out.append((K3S2T, n, d >> (lvl + 1), h >> (lvl + 1), w >> (lvl + 1), cin, f))
        out.append((K1, n, d >> (lvl + 1), h >> (lvl + 1), w >> (lvl + 1), cin, f))      # linear up-sampler (f-4)
        block(lvl, f * (lvl + 1) + f, f)
    out.append((K1, n, d, h, w, F, 3))
    if (d, h, w) == (128, 128, 128):            # the VAE branch is tied to the training crop (vae.py:101-111)
        out.append((K3S2, n, d >> 3, h >> 3, w >> 3, top * DEPTH, 16))
        for lvl in range(DEPTH - 1, -1, -1):
            f = F << lvl
            out.append((K3S2T, n, d >> (lvl + 1), h >> (lvl + 1), w >> (lvl + 1), 1 if lvl == DEPTH - 1 else f * 2, f))
            if lvl < DEPTH - 1:
                block(lvl, f, f)
        out.append((K3S1, n, d, h, w, F, 2))
    return sorted(set(out))


@pytest.fixture(scope='module')
def L():
    import bts_amd  # noqa: F401
    from bts_amd._lib import lib
    lb = lib()
    want = os.environ.get('BTS_EXPECT_LIB')        # the sanitizer run: make sure the instrumented build is the one that answered
    if want:
        assert want in open('/proc/self/maps').read(), '%s is not mapped into this process' % want
    return lb


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_conv_planning_queries_are_total_and_deterministic(L, grid):
    n, d, h, w = grid
    shapes = layer_shapes(n, d, h, w)
    assert len(shapes) >= 40
    q7 = ['bts_conv3d_fwd_workspace', 'bts_conv3d_bwd_data_workspace', 'bts_conv3d_bwd_weight_workspace', 'bts_lp_conv3d_workspace',
          'bts_lp_conv3d_bwd_data_workspace', 'bts_lp_conv3d_bwd_weight_workspace']
    c7 = ['bts_conv3d_fwd_config', 'bts_conv3d_bwd_data_config']
    for (kind, N, D, H, W, ci, co) in shapes:
        for name in q7 + c7:
            f = getattr(L, '_' + name)
            a, b = f(kind, N, D, H, W, ci, co), f(kind, N, D, H, W, ci, co)
            assert a == b and a >= -3, (name, kind, N, D, H, W, ci, co, a, b)     # -1: the form declines; -3: BTS_ERR_UNSUPPORTED from a config query
            if name in q7 and N > 1 and a >= 0:
                one = f(kind, 1, D, H, W, ci, co)
                assert one <= a or one < 0 or a == 0, (name, kind, N, D, H, W, ci, co, one, a)
        if kind == 1:
            for name, args in (('bts_conv3d_fwd_can_fuse', (N, D, H, W, ci, co)), ('bts_conv3d_bwd_data_pair_workspace', (N, D, H, W, ci, co)),
                               ('bts_conv3d_fwd_gn_workspace', (kind, N, D, H, W, ci, co, G)),
                               ('bts_lp_conv3d_fwd_gn_workspace', (N, D, H, W, ci, co, G)),
                               ('bts_lp_conv3d_gnin_fwd_gn_workspace', (N, D, H, W, ci, co, G, G)),
                               ('bts_lp_conv3d_gnin_train_ok', (N, D, H, W, ci, co, G, G)),
                               ('bts_lp_conv3d_bwd_data_gn_bwd_workspace', (N, D, H, W, ci, co, G))):
                f = getattr(L, '_' + name)
                a = f(*args)
                assert a == f(*args) and a >= -4, (name, args, a)
        if kind == 3:
            a = L._bts_lp_convT3d_fwd_gn_workspace(N, D, H, W, ci, co, G)
            assert a == L._bts_lp_convT3d_fwd_gn_workspace(N, D, H, W, ci, co, G) and a >= -4
        for role in (0, 1):
            if co >= 1 and ci >= 1:
                fl = L._bts_conv_packed_floats(kind, role, ci, co)
                by = L._bts_lp_packed_bytes(kind, role, ci, co)
                assert fl > 0 and by != 0, (kind, role, ci, co, fl, by)


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_normalisation_and_gate_workspaces(L, grid):
    n, d, h, w = grid
    for lvl in range(DEPTH):
        V = (d >> lvl) * (h >> lvl) * (w >> lvl)
        f = F << lvl
        for mode in (0, 1):
            assert L._bts_gn_workspace(n, V, f, G, mode) >= 0 and L._bts_gn_bwd_workspace(n, V, f, G, mode) >= 0
        assert L._bts_lp_gn_workspace(n, V, f, G) >= -1 and L._bts_lp_gn_bwd_workspace(n, V, f, G) >= -1
        assert L._bts_colsum_workspace(n, V, f) >= 0 and L._bts_lp_colsum_workspace(n, V, f) >= -1
        assert L._bts_se_bwd_workspace(n, V, f, f // R) >= 0 and L._bts_lp_se_bwd_workspace(n, V, f, f // R) >= -1
        assert L._bts_block_bwd_workspace(n, V, f, f // R, G) >= -1 and L._bts_lp_block_bwd_workspace(n, V, f, f // R, G) >= -1
        assert L._bts_lp_conv1_gap_workspace(n, V, f) >= -1
        assert L._bts_channel_moments_workspace(f) >= 0
    assert L._bts_dense_workspace(n, 8192, 256) >= 0 and L._bts_dense_workspace(n, 128, 512) >= 0
    assert L._bts_loss_workspace() > 0 and L._bts_l2_workspace() > 0 and L._bts_lp_head_bwd_workspace(32, 3) >= 0



def test_split_data_gradient_query_matches_the_kernel_bounds(L):
    """bts_lp_conv3d_bwd_data_sc_split_ok answers from the same choice the launch makes: at 1 x 224^3 (64 -> 32) the split output's
    offsets leave 31 bits and the launch declines, so the query must say 0 (the trainer then keeps level 0 as one slab)"""
    assert L._bts_lp_conv3d_bwd_data_sc_split_ok(1, 224, 224, 224, 64, 32) == 0
    assert L._bts_lp_conv3d_bwd_data_sc_split_ok(1, 192, 192, 192, 64, 32) == 1
    assert L._bts_lp_conv3d_bwd_data_sc_split_ok(8, 128, 128, 128, 64, 32) == 1

@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_transposed_and_pooled_conv_queries_answer_from_one_plan(L, grid, monkeypatch):
    """bts_lp_convT3d_fwd_gn_workspace (every K3S2T shape) answers from the plan the launch makes: the same answer twice, a positive
    size, and at least as large for N samples as for one -- with the merged transposed kernel and the streaming 1x1x1 kernel on
    (default) and off.  bts_lp_conv1_gap_workspace (every level) is held to the same three properties, but it is a closed-form upper
    bound that sees neither Cin nor a switch (the launch asks for partial rows only where they fit it), so it is asked once."""
    n, d, h, w = grid
    up = [s for s in layer_shapes(n, d, h, w) if s[0] == 3]
    assert len(up) >= 3
    for switch in (None, 'BTS_LP_UP', 'BTS_LP_K1'):
        for name in ('BTS_LP_UP', 'BTS_LP_K1', 'BTS_LP_S2T'):
            monkeypatch.delenv(name, raising=False)
        if switch:
            monkeypatch.setenv(switch, '0')
        for (kind, N, D, H, W, ci, co) in up:
            a = L._bts_lp_convT3d_fwd_gn_workspace(N, D, H, W, ci, co, G)
            assert a == L._bts_lp_convT3d_fwd_gn_workspace(N, D, H, W, ci, co, G) and a > 0, (switch, N, D, H, W, ci, co, a)
            assert L._bts_lp_convT3d_fwd_gn_workspace(1, D, H, W, ci, co, G) <= a, (switch, N, D, H, W, ci, co, a)
    for lvl in range(DEPTH):
        V, f = (d >> lvl) * (h >> lvl) * (w >> lvl), F << lvl
        a = L._bts_lp_conv1_gap_workspace(n, V, f)
        assert a == L._bts_lp_conv1_gap_workspace(n, V, f) and a > 0, (n, V, f, a)
        assert L._bts_lp_conv1_gap_workspace(1, V, f) <= a, (n, V, f, a)


def test_transposed_conv_query_knows_the_merged_kernels_offset_bounds(L, monkeypatch):
    """a fine tensor whose byte offsets leave 31 bits (coarse 1 x 160x192x160, 64 -> 32: 2.5 GB) is not the merged transposed kernel's: the
    launch runs the gather kernels and bts_lp_gn_stats, so the query sizes the statistics pass and no partial slots (it used to size
    4.9 MB of slots the launch never wrote)"""
    monkeypatch.delenv('BTS_LP_UP', raising=False)
    for ci in (64, 32):
        assert L._bts_lp_convT3d_fwd_gn_workspace(1, 160, 192, 160, ci, 32, G) == L._bts_lp_gn_workspace(1, 8 * 160 * 192 * 160, 32, G) + 64
    # (half the extent: the merged kernel takes it, and its slots are the larger need)
    assert L._bts_lp_convT3d_fwd_gn_workspace(1, 80, 96, 80, 64, 32, G) > L._bts_lp_gn_workspace(1, 8 * 80 * 96 * 80, 32, G) + 64


def test_gather_family_calls_refuse_bad_arguments_before_any_launch(L, monkeypatch):
    """the 1x1x1, stride-2 and transposed entry points of the 16-bit engine return their argument statuses before any HIP call -- input
    channels that are not whole 16-channel steps, an input stride that is not a multiple of 8, output rows narrower than Cout
    (BTS_ERR_ALIGN), an unknown storage type (BTS_ERR_UNSUPPORTED), a short or misaligned workspace (BTS_ERR_WORKSPACE): the codes the
    trial-order dispatch returned.  Fake, never dereferenced device addresses; on a grid no fast kernel takes (8^3) and on one they do
    (32^3).  bts_lp_conv1_gap's storage type is asked at 8^3 only: at 32^3 the streaming kernel takes the fused call on its own
    conditions, which have never included the type, and the call reaches its launch."""
    for name in ('BTS_LP_UP', 'BTS_LP_K1', 'BTS_LP_S2T', 'BTS_LP_GATHERQ'):
        monkeypatch.delenv(name, raising=False)
    P, BF16, N, ci, co = 0x100000, 2, 1, 32, 32
    ALIGN, UNSUPPORTED, WORKSPACE = -2, -3, -4
    cases = (('Cin % 16', dict(ci=24), ALIGN), ('ldx % 8', dict(ldx=36), ALIGN), ('ldy < Cout', dict(ldy=16), ALIGN),
             ('dtype', dict(dtype=7), UNSUPPORTED))
    for S in (8, 32):
        for what, kw, want in cases:
            c_in = kw.get('ci', ci)
            ldx, ldy, dtype = kw.get('ldx', c_in), kw.get('ldy', co), kw.get('dtype', BF16)
            for kind in (0, 2, 3):
                r = L._bts_lp_conv3d_fwd(kind, dtype, P, P, P, P, None, 0, N, S, S, S, c_in, ldx, co, ldy, None)
                assert r == want, ('fwd', S, kind, what, r)
                # (the data gradient contracts over the forward's Cout: dy is the operand with the channel and stride rules, dx the output)
                r = L._bts_lp_conv3d_bwd_data(kind, dtype, P, P, P, None, 0, N, S, S, S, co, ldy, c_in, ldx, 0, None)
                assert r == want, ('bwd_data', S, kind, what, r)
            if what != 'ldy < Cout':      # (its y is dense by contract)
                nb = L._bts_lp_convT3d_fwd_gn_workspace(N, S, S, S, c_in, co, G)
                r = L._bts_lp_convT3d_fwd_gn(dtype, P, P, P, P, P, P, P, nb, N, S, S, S, c_in, ldx, co, G, 1e-5, None)
                assert r == want, ('convT3d_fwd_gn', S, what, r)
            if not (what == 'dtype' and S == 32):
                nb = L._bts_lp_conv1_gap_workspace(N, S * S * S, co)
                r = L._bts_lp_conv1_gap(dtype, P, P, P, P, P, P, nb, N, S, S, S, c_in, ldx, co, ldy, None)
                assert r == want, ('conv1_gap', S, what, r)
        for ws, short in ((P, 16), (P + 8, 0)):
            nb = L._bts_lp_convT3d_fwd_gn_workspace(N, S, S, S, ci, co, G)
            assert L._bts_lp_convT3d_fwd_gn(BF16, P, P, P, P, P, P, ws, short or nb, N, S, S, S, ci, ci, co, G, 1e-5, None) == WORKSPACE
            nb = L._bts_lp_conv1_gap_workspace(N, S * S * S, co)
            assert L._bts_lp_conv1_gap(BF16, P, P, P, P, P, ws, short or nb, N, S, S, S, ci, ci, co, co, None) == WORKSPACE


def test_weight_gradient_calls_refuse_an_impossible_bias_gradient_before_any_launch(L, monkeypatch):
    """a 16-bit weight-gradient call that cannot produce its db (dy rows wider than Cout; a Cout whose 16-byte chunks do not tile the
    256-thread column-sum block) answers from its plan, before dw is touched -- BTS_ERR_UNSUPPORTED / BTS_ERR_SHAPE as ever.  Fake,
    never dereferenced device addresses and a workspace as large as the query asks: nothing else is wrong with these calls."""
    monkeypatch.delenv('BTS_LP_WGD', raising=False)
    P, BF16, N, D, H, W, ci = 0x100000, 2, 1, 32, 32, 32, 32
    for co, lddy, want in ((32, 64, -3), (24, 24, -1)):
        for kind in (0, 1, 2, 3):
            nb = L._bts_lp_conv3d_bwd_weight_workspace(kind, N, D, H, W, ci, co)
            assert nb > 0
            r = L._bts_lp_conv3d_bwd_weight(kind, BF16, P, P, P, P, P, nb, N, D, H, W, ci, ci, co, lddy, 0, 0, 1, None)
            assert r == want, (kind, co, lddy, r)
        nb = L._bts_lp_conv3d_bwd_weight_pair_workspace(N, D, H, W, ci, co)
        assert nb > 0
        r = L._bts_lp_conv3d_bwd_weight_pair(BF16, P, 0, P, P, P, P, P, P, nb, N, D, H, W, ci, ci, co, lddy, co, 0, 0, 1, None)
        assert r == want, ('pair', co, lddy, r)
        nb = L._bts_lp_conv3d_bwd_weight_workspace(1, N, D, H, W, ci, co)
        r = L._bts_lp_conv3d_gnin_bwd_weight(BF16, P, P, P, P, P, G, P, P, P, P, nb, N, D, H, W, ci, co, lddy, 1, None)
        assert r == want, ('gnin', co, lddy, r)


def test_gn_bwd_tiling_query_is_the_rule_the_python_side_used_to_state(L):
    """bts_lp_gn_bwd_tiled (the one statement of the GroupNorm-backward tiling) against tests/lowp_ref.gn_bwd_tiled_ref, the expression
    bts_amd.lowp carried before; lowp.gn_bwd_tiled is a probe of it; outside the tiling bts_lp_gn_bwd and lowp.gn_bwd decline as ever,
    before any launch"""
    import lowp_ref
    from bts_amd import lowp
    seen = set()
    for V in (64, 512, 2048, 4096, 4097, 32768, 128 ** 3):
        for C in (8, 16, 24, 32, 64, 128, 256, 512):
            for g in (1, 2, 4, 8, 16, 32):
                if C % g:
                    continue
                want = bool(lowp_ref.gn_bwd_tiled_ref(V, C, g))
                assert L._bts_lp_gn_bwd_tiled(V, C, g) == int(want), (V, C, g)
                assert lowp.gn_bwd_tiled(V, C, g) is want, (V, C, g)
                seen.add(want)
                if not want and C <= 256 and not C & (C - 1):      # (other C: BTS_ERR_SHAPE, as ever)
                    P = 0x100000
                    r = L._bts_lp_gn_bwd(2, P, P, P, None, P, P, P, P, P, P, P, 1 << 40, 1, V, C, C, g, 1, 1, None, None)
                    assert r == -3, (V, C, g, r)
    assert seen == {True, False}

    class FakeX(object):      # lowp.gn_bwd reads the shape, asks the rule and returns None: no tensor is touched, nothing is launched
        shape = (1, 1, 1, 4097, 32)
    assert lowp.gn_bwd(2, None, FakeX(), None, None, None, None, None, None, None, 8, True) is None


def test_weight_gradient_args_query_is_the_rule_the_python_side_used_to_state(L):
    """bts_lp_conv3d_bwd_weight_args_ok (lp_wg_args' answer for the dense, aligned, unfolded call) against
    tests/lowp_ref.wgrad_supported_ref, the expression bts_amd.lowp carried before; lowp.wgrad_supported is a probe of it, and
    lowp.conv_bwd_weight declines (False, nothing launched) exactly where it says no"""
    import lowp_ref
    from bts_amd import lowp
    chans = (4, 8, 12, 16, 24, 32, 64, 256, 264, 512)
    seen = set()
    for kind in (0, 1, 2, 3):
        for ext in ((16, 16, 16), (15, 16, 16), (16, 16, 17)):
            for ci in chans:
                for co in chans:
                    want = bool(lowp_ref.wgrad_supported_ref(kind, ci, co, ext))
                    assert L._bts_lp_conv3d_bwd_weight_args_ok(kind, ext[0], ext[1], ext[2], ci, co) == int(want), (kind, ext, ci, co)
                    assert lowp.wgrad_supported(kind, ci, co, ext) is want, (kind, ext, ci, co)
                    seen.add(want)
    assert seen == {True, False}
    assert L._bts_lp_conv3d_bwd_weight_args_ok(4, 16, 16, 16, 32, 32) == 0 and L._bts_lp_conv3d_bwd_weight_args_ok(-1, 16, 16, 16, 32, 32) == 0
    # the kinds that do not read the extents are asked without them (the paired launch's caller)
    assert lowp.wgrad_supported(1, 64, 32) is True and lowp.wgrad_supported(1, 64, 264) is False

    class Fake(object):      # lowp.conv_bwd_weight reads the two shapes, asks the rule and returns False: nothing is launched
        def __init__(self, *shape):
            self.shape = shape
    for kind, ext, ci, co in ((1, (16, 16, 16), 32, 264), (0, (16, 16, 16), 12, 32), (2, (15, 16, 16), 32, 32), (3, (16, 16, 16), 32, 12)):
        assert lowp.conv_bwd_weight(kind, 2, Fake(1, *ext, ci), Fake(1, *ext, co), None, None) is False, (kind, ext, ci, co)


def test_paired_weight_gradient_query_at_the_split_level0_shapes(L, monkeypatch):
    """the trainer's level-0 split (two dense 32-channel operands, no single-tensor fallback) relies on the paired launch taking
    64 -> 32 at 128^3; the streaming kernel's 32-wide columns do not exist where W % 32 != 0"""
    monkeypatch.delenv('BTS_LP_WGD', raising=False)
    assert L._bts_lp_conv3d_bwd_weight_pair_workspace(8, 128, 128, 128, 64, 32) >= 0
    assert L._bts_lp_conv3d_bwd_weight_pair_workspace(1, 128, 128, 128, 64, 32) >= 0
    assert L._bts_lp_conv3d_bwd_weight_pair_workspace(1, 128, 128, 112, 64, 32) == -1


def test_pack_descriptor_tables_are_written_inside_their_bounds(L):
    """bts_conv_pack_desc / bts_lp_pack_desc fill entry `index` of a host table of `*_desc_bytes()` entries: a guard band behind the
    table must stay untouched (the ASan run checks the same thing from the allocator's side)"""
    shapes = [s for s in layer_shapes(1, 128, 128, 128) if s[5] % 8 == 0 and s[6] % 8 == 0][:24]
    for desc_bytes, desc, sizes in ((L._bts_conv_pack_desc_bytes, L._bts_conv_pack_desc, lambda k, r, ci, co: L._bts_conv_packed_floats(k, r, ci, co) * 4),
                                    (L._bts_lp_pack_desc_bytes, L._bts_lp_pack_desc, lambda k, r, ci, co: L._bts_lp_packed_bytes(k, r, ci, co))):
        nb = desc_bytes()
        assert nb > 0
        guard = 256
        buf = ctypes.create_string_buffer(b'\xa5' * (nb * len(shapes) + guard), nb * len(shapes) + guard)
        first = 0
        for i, (kind, N, D, H, W, ci, co) in enumerate(shapes):
            for role in (0, 1):
                if sizes(kind, role, ci, co) <= 0:
                    continue
                # (fake, never dereferenced device addresses: the descriptor only records them)
                r = desc(ctypes.cast(buf, ctypes.c_void_p), i, first, kind, role, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x100000), ci, co, ci, 0, 0)
                assert r > 0, (kind, role, ci, co, r)      # = blocks of this entry
            first += r
        assert buf.raw[nb * len(shapes):] == b'\xa5' * guard


# ---- the fp32 conv engine's dispatch: bts_conv3d_kernel answers from the choice the launches run on ----
SYM = dict(upm=20, k1s=21, dsc=22, wino=23, c2=25, w3=27)
TILED = tuple(range(5)) + tuple(range(8, 13))      # igemm_kernel config ids, + 8: the 1x1x1 staging variant
CONV_SWITCHES = ('BTS_WINO', 'BTS_W3', 'BTS_WINO_MIN_WGS', 'BTS_IGEMM_DSC_MIN', 'BTS_IGEMM_C2_MIN', 'BTS_IGEMM_K1S_MIN', 'BTS_IGEMM_UPM_MIN',
                 'BTS_IGEMM_NOGNFUSE', 'BTS_IGEMM_NOPAIR')
FWD, BWD, Y2, X2, SIGMOID = 0, 1, 1, 2, 1


def conv_kernel(L, direction, kind, N, D, H, W, ci, co, flags=0, second=0, groups=0, aligned=15, ws=-1, ldx=None, ldy=None, ld2=None):
    """bts_conv3d_kernel on dense rows unless told otherwise; aligned: bit 0 read, 1 written, 2 second operand, 3 workspace; ws < 0: all it asks"""
    if ld2 is None:
        ld2 = 0 if not second else (co if (second == Y2) == (direction == FWD) else ci)
    return L._bts_conv3d_kernel(direction, kind, N, D, H, W, ci, ldx or ci, co, ldy or co, flags, second, ld2, groups, aligned, ws)


@pytest.fixture
def default_switches(monkeypatch):
    for name in CONV_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_conv_kernel_query_is_deterministic_and_agrees_with_the_config_queries(L, grid, default_switches):
    """every layer shape, forward and data gradient: the same kernel twice, a known symbol, and where it is the tiled kernel the
    config the bts_conv3d_*_config queries (bench.py's attribution) name"""
    for (kind, N, D, H, W, ci, co) in layer_shapes(*grid):
        for direction, cfg in ((FWD, L._bts_conv3d_fwd_config), (BWD, L._bts_conv3d_bwd_data_config)):
            k = conv_kernel(L, direction, kind, N, D, H, W, ci, co)
            assert k == conv_kernel(L, direction, kind, N, D, H, W, ci, co), (direction, kind, N, D, H, W, ci, co)
            assert k in TILED or k in SYM.values(), (direction, kind, N, D, H, W, ci, co, k)
            if k in TILED:
                assert k == cfg(kind, N, D, H, W, ci, co), (direction, kind, N, D, H, W, ci, co, k)
            assert (k >= 8 and k in TILED) <= (kind == 0)
            if kind == 1:      # the forms of the 3x3x3 stride-1 call name a kernel too (or the tiled kernel's refusal of the fused pair)
                for second in ((Y2,) if direction == FWD else (X2,)):
                    k2 = conv_kernel(L, direction, kind, N, D, H, W, ci, co, second=second)
                    assert k2 == conv_kernel(L, direction, kind, N, D, H, W, ci, co, second=second)
                    assert k2 in TILED or k2 in SYM.values() or k2 == -3, (direction, N, D, H, W, ci, co, second, k2)
                kg = conv_kernel(L, direction, kind, N, D, H, W, ci, co, groups=G)
                assert kg == k, (direction, N, D, H, W, ci, co, k, kg)      # asking for GroupNorm partials never changes the kernel


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_can_fuse_is_the_tiled_kernels_answer_to_the_fused_pair(L, grid, default_switches):
    """bts_conv3d_fwd_can_fuse is 0 exactly where the tiled kernel, were the fused-shortcut call left to it, would run cfg 1 and refuse
    (BTS_ERR_UNSUPPORTED).  It answers for every switch setting, so the equivalence is read with the Winograd forms off; with them on,
    a refused call still always has can_fuse == 0 (the forms take the pair as two launches wherever they accept the 3x3x3 part)."""
    seen = set()
    for (kind, N, D, H, W, ci, co) in layer_shapes(*grid):
        if kind != 1:
            continue
        fuse = L._bts_conv3d_fwd_can_fuse(N, D, H, W, ci, co)
        k_on = conv_kernel(L, FWD, 1, N, D, H, W, ci, co, second=Y2)
        default_switches.setenv('BTS_WINO', '0')
        k_off = conv_kernel(L, FWD, 1, N, D, H, W, ci, co, second=Y2)
        default_switches.delenv('BTS_WINO')
        assert fuse == L._bts_conv3d_fwd_can_fuse(N, D, H, W, ci, co)
        assert (fuse == 0) == (k_off == -3), (N, D, H, W, ci, co, fuse, k_off)
        assert k_off == -3 or k_off == SYM['c2'] or (k_off in TILED and k_off != 1), (N, D, H, W, ci, co, k_off)
        assert k_on != -3 or fuse == 0, (N, D, H, W, ci, co, fuse, k_on)
        seen.add(fuse)
    assert seen == {0, 1}      # (every grid has layers of both sorts)


def test_conv_dispatch_facts_of_the_plan_table(L, default_switches):
    """DESIGN "Dispatch plan", at 1 x 128^3"""
    S = (1, 128, 128, 128)
    assert conv_kernel(L, FWD, 1, *S, 32, 2) == SYM['dsc']
    assert conv_kernel(L, FWD, 1, *S, 2, 32) == SYM['c2']
    assert conv_kernel(L, FWD, 1, *S, 2, 32, second=Y2) == SYM['c2']      # ... with the fused shortcut output in the same launch
    assert conv_kernel(L, FWD, 1, *S, 32, 32) == SYM['w3']
    assert conv_kernel(L, BWD, 1, *S, 32, 32) == SYM['w3']
    assert conv_kernel(L, FWD, 1, *S, 32, 32, flags=SIGMOID) in TILED      # never a Winograd form with the sigmoid
    assert conv_kernel(L, FWD, 0, *S, 32, 32) == SYM['k1s']
    assert conv_kernel(L, FWD, 0, 1, 16, 16, 16, 32, 32) in range(8, 13)
    default_switches.setenv('BTS_W3', '0')
    assert conv_kernel(L, FWD, 1, *S, 32, 32) == SYM['wino']
    assert conv_kernel(L, FWD, 1, *S, 32, 32, flags=SIGMOID) in TILED
    default_switches.setenv('BTS_WINO', '0')
    assert conv_kernel(L, FWD, 1, *S, 32, 32) == L._bts_conv3d_fwd_config(1, *S, 32, 32) == 0
    default_switches.delenv('BTS_W3')      # BTS_WINO=0 alone switches both forms off
    assert conv_kernel(L, FWD, 1, *S, 32, 32) == 0
    assert conv_kernel(L, FWD, 1, *S, 32, 2) == SYM['dsc'] and conv_kernel(L, FWD, 1, *S, 2, 32) == SYM['c2']


def test_conv_kernel_query_sees_what_the_operands_allow(L, default_switches):
    """a query never names a kernel whose launcher would refuse the call: a misaligned or oddly strided x sends a Winograd, streaming or
    direct shape to the tiled kernel, and a split-K shape without a usable workspace gets the kernel that runs unsplit"""
    S = (1, 128, 128, 128)
    X_OFF, NO_WS = 14, 0
    for direction in (FWD, BWD):
        assert conv_kernel(L, direction, 1, *S, 32, 32, aligned=X_OFF) == 0
        assert conv_kernel(L, direction, 1, *S, 32, 32, ldx=34) == 0
        assert conv_kernel(L, direction, 0, *S, 32, 32, aligned=X_OFF) == 8
    assert conv_kernel(L, FWD, 1, *S, 32, 32, aligned=13) == 0                  # y off its 16-byte boundary
    assert conv_kernel(L, FWD, 1, *S, 32, 2, aligned=X_OFF) in TILED            # dsc reads 16-byte rows
    assert conv_kernel(L, FWD, 1, *S, 2, 32, aligned=13) in TILED               # c2 stores them
    assert conv_kernel(L, FWD, 1, *S, 2, 32, second=Y2, aligned=11) in TILED    # ... to y2 as well
    # 256 -> 256 at 16^3: 128 Winograd workgroups -- the F(2x2x2,3x3x3) form takes the call only with its 4-way split-K workspace
    T = (1, 16, 16, 16, 256, 256)
    need = L._bts_conv3d_fwd_workspace(1, *T)
    assert need > 0
    assert conv_kernel(L, FWD, 1, *T) == conv_kernel(L, FWD, 1, *T, ws=need) == SYM['w3']
    for kw in (dict(ws=NO_WS), dict(ws=need - 4), dict(ws=need, aligned=7)):      # none, short, misaligned
        assert conv_kernel(L, FWD, 1, *T, **kw) in TILED, kw
    assert conv_kernel(L, FWD, 1, *T, ws=NO_WS) == L._bts_conv3d_fwd_config(1, *T)
    # the merged transposed kernel needs its split-K workspace on a small grid too: without it the tiled kernel runs the 8 classes
    U = (1, 8, 8, 8, 256, 128)
    assert L._bts_conv3d_fwd_workspace(3, *U) > 0
    assert conv_kernel(L, FWD, 3, *U) == SYM['upm'] and conv_kernel(L, FWD, 3, *U, ws=NO_WS) in TILED
    assert conv_kernel(L, FWD, 3, *U, aligned=X_OFF) in TILED
    # statuses come back as they do from the launch: odd extents under stride 2, rows narrower than the channels
    assert conv_kernel(L, FWD, 2, 1, 7, 8, 8, 32, 32) == -1 and conv_kernel(L, FWD, 1, *S, 32, 32, ldx=16) == -1
    assert conv_kernel(L, FWD, 2, 1, 8, 8, 8, 32, 32, second=Y2) == -1          # the second forms exist for 3x3x3 stride 1 only


# ---- the fp32 weight gradient's dispatch: bts_conv3d_bwd_weight_kernel answers from the choice the launch runs on ----
WG_DIRECT = (100, 104, 109, 110)      # wgrad_kernel: register staging | LDS-DMA staging | the fixed-geometry sweeps of stride 1 | 2
WGW, K1W = 24, 26
WG_SWITCHES = ('BTS_WGW', 'BTS_K1W')


def wg_query(L, name, kind, N, D, H, W, ci, co, aligned=3, ldx=None, lddy=None):
    """a bts_conv3d_bwd_weight_* query on dense rows unless told otherwise; aligned: bit 0 x, bit 1 dy on a 16-byte boundary"""
    return getattr(L, '_bts_conv3d_bwd_weight_' + name)(kind, N, D, H, W, ci, ldx or ci, co, lddy or co, aligned)


def wg_kernel(L, *a, **kw):
    return wg_query(L, 'kernel', *a, **kw)


@pytest.fixture
def default_wg_switches(monkeypatch):
    for name in WG_SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


@pytest.mark.parametrize('grid', GRIDS, ids=lambda g: '%dx%dx%dx%d' % g)
def test_weight_gradient_kernel_query_is_deterministic_and_follows_its_switches(L, grid, default_wg_switches):
    """every layer shape: the same kernel twice, a known symbol or a status, form 3 exactly where the kernel is wgw_kernel, and each
    switch turns its own kernel into the direct kernel that stands behind it and changes nothing else: wgw_kernel into the fixed sweep
    (109), k1w_kernel into the LDS-DMA staging (104) or, where a channel count is no whole 16 bytes (the 1- and 3-channel heads), into
    the register staging (100)"""
    seen = set()
    for shape in layer_shapes(*grid):
        k1w_behind = 104 if shape[5] % 4 == 0 and shape[6] % 4 == 0 else 100
        k = wg_kernel(L, *shape)
        assert k == wg_kernel(L, *shape), shape
        assert k in WG_DIRECT + (WGW, K1W) or k < 0, (shape, k)
        f = wg_query(L, 'form', *shape)
        assert (f == 3) == (k == WGW) and f in (0, 3, k), (shape, k, f)
        for switch, own, behind in (('BTS_WGW', WGW, 109), ('BTS_K1W', K1W, k1w_behind)):
            default_wg_switches.setenv(switch, '0')
            k0, f0 = wg_kernel(L, *shape), wg_query(L, 'form', *shape)
            default_wg_switches.delenv(switch)
            assert k0 == (behind if k == own else k), (shape, switch, k, k0)
            assert (f0 == 3) == (k0 == WGW), (shape, switch, k0, f0)
        seen.add(k)
    assert {WGW, K1W, 100, 110} <= seen      # (every grid has layers of these sorts)


def test_weight_gradient_dispatch_facts_of_the_plan_table(L, default_wg_switches):
    """DESIGN "Dispatch plan", at 1 x 128^3 unless a shape is given"""
    S = (1, 128, 128, 128)
    K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
    assert wg_kernel(L, K3S1, *S, 32, 32) == WGW
    assert wg_kernel(L, K3S1, *S, 32, 32, aligned=2) == 100               # x off its boundary: register staging
    assert wg_kernel(L, K3S1, *S, 32, 32, ldx=34) == 100                  # rows that are no whole 16 bytes
    assert wg_kernel(L, K3S1, 1, 8, 8, 24, 32, 32) == 104                 # ragged W: the general LDS-DMA staging
    assert wg_kernel(L, K3S1, 1, 2, 4, 16, 32, 32) == WGW                 # one sub-tile
    assert wg_kernel(L, K3S1, *S, 2, 32) == 100
    assert wg_kernel(L, K3S1, *S, 32, 2) == 100                           # the swapped form
    assert wg_kernel(L, K3S2, *S, 32, 32) == 110
    assert wg_kernel(L, K3S2T, 1, 64, 64, 64, 64, 32) == 110
    assert wg_kernel(L, K1, *S, 32, 32) == K1W
    assert wg_kernel(L, K1, 1, 16, 16, 16, 32, 32) == 104
    assert wg_kernel(L, K1, 1, 32, 32, 32, 32, 32) == K1W                 # 32768 voxels: the threshold
    assert wg_kernel(L, K1, 1, 32, 32, 31, 32, 32) == 104
    # statuses come back as they do from the launch: odd extents under stride 2
    assert wg_kernel(L, K3S2, 1, 7, 8, 8, 32, 32) == wg_query(L, 'form', K3S2, 1, 7, 8, 8, 32, 32) == -1
    assert L._bts_conv3d_bwd_weight_workspace(K3S2, 1, 7, 8, 8, 32, 32) == -1
    # the K-split is capped: the larger grid asks for no more workspace
    need = L._bts_conv3d_bwd_weight_workspace(K3S1, *S, 32, 32)
    assert need > 0 and need == L._bts_conv3d_bwd_weight_workspace(K3S1, 1, 160, 192, 160, 32, 32)
