"""The case table of the tiled fp32 conv kernel (igemm_kernel, csrc/conv_igemm.hip): one row per variant the launcher compiles and the
model runs, at the smallest shape that reaches it.  tests/test_tiled_configs_gpu.py runs every row against the fp64 oracle;
tests/test_tiled_configs_host.py checks on the CPU that every row is named the symbol it claims and that no layer of the model runs a
(direction, kind, form, symbol) the table does not hold.  No torch, no GPU: plain data and the arithmetic of a row's operands.

How the plan picks a config (choose_cfg; vox = voxels of the iteration grid, Npad = Cout rounded up to 32, N counted 8-fold for the
parity classes of the transposed geometry):
  stride-2 geometry: cfg 2 where Npad >= 128, else cfg 3;
  Npad <= 32: cfg 0 (M256 x N32, two M sub-tiles per wave) where N * ceil(vox / 256) >= 512, else cfg 4;
  else cfg 1 (M256 x N64, two M and two N sub-tiles) where N * ceil(vox / 256) * ceil(Npad / 64) >= 512;
  else cfg 2 (M64 x N128, two N sub-tiles, gridy = ceil(Npad / 128)) where Npad >= 128 and N * ceil(vox / 64) * ceil(Npad / 128) >= 384;
  else cfg 3.
The profile symbol is the config, + 8 for the 1x1x1 staging (four k-groups per pass).  It does not tell the instantiation: each row's
comment states the plan facts that select it -- the geometry, the halo IX x IY of the TX x TY tile (the fixed-geometry sweep FIXG runs
only 3x3x3 stride 1 on cfg 0 / 1 with IX == 34 and IY == 6, i.e. TX = 32, TY = 4: W >= 17, H >= 3; every other 27-tap call runs T27, the
fused shortcut output FUSE2), and whether the contraction is split (a workspace is asked for)."""
import collections

FWD, BWD = 0, 1
K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
Y2, X2 = 1, 2                  # second form: fused shortcut output (forward) | second input of the data-gradient pair
UNSUPPORTED = -3               # BTS_ERR_UNSUPPORTED: the fused shortcut output on cfg 1
TILED = tuple(range(5)) + tuple(range(8, 13))
SWITCHES = ('BTS_WINO', 'BTS_W3', 'BTS_WINO_MIN_WGS', 'BTS_IGEMM_DSC_MIN', 'BTS_IGEMM_C2_MIN', 'BTS_IGEMM_K1S_MIN', 'BTS_IGEMM_UPM_MIN',
            'BTS_IGEMM_NOGNFUSE', 'BTS_IGEMM_NOPAIR')
NOWINO = {'BTS_WINO': '0'}
NOK1S = {'BTS_IGEMM_K1S_MIN': str(1 << 40)}

# direction, kind, (N, D, H, W, Cin, Cout) as the ABI names them (the forward input's extents, the forward's channels); sym: the profile
# symbol claimed (or UNSUPPORTED); env: switches, every other one unset; second: 0 | Y2 | X2; sigmoid / accumulate: the call's flags;
# bias: a bias is passed (forward); xslab: the tensor READ is channels [1, 1 + C) of a slab of C + 3 channels (off its 16-byte boundary,
# rows that are no whole 16 bytes: IG_FLAG_VECIN off); yslab: the tensor WRITTEN is channels [4, 4 + C) of a slab of C + 8 channels, whose
# other channels must keep their bytes; groups: GroupNorm statistics from the same call (bts_conv3d_fwd_gn); splitk: the workspace
# query must ask for bytes (the contraction is split over blockIdx.z and finished by igemm_reduce_kernel)
Row = collections.namedtuple('Row', 'name direction kind n dims cin cout sym env second sigmoid accumulate bias xslab yslab groups splitk')


def row(name, direction, kind, n, dims, cin, cout, sym, env=None, second=0, sigmoid=False, accumulate=False, bias=True, xslab=False,
        yslab=False, groups=0, splitk=False):
    return Row(name, direction, kind, n, tuple(dims), cin, cout, sym, dict(env or {}), second, sigmoid, accumulate, bias, xslab, yslab,
               groups, splitk)


BIG = (16, 64, 128)            # 131072 voxels = 512 tiles of 256: the smallest whole-tile grid of cfg 0 (and of cfg 1 at Npad = 64)
BIG_R = (17, 62, 125)          # 131750 voxels, ragged on every axis, still TX = 32, TY = 4
THIN = (128, 64, 16)           # 131072 voxels with W = 16: TX = 16, IX = 18, no fixed geometry
THIN_R = (137, 64, 15)         # 131520 voxels, W and D ragged, TX = 16
K1BIG = (32, 64, 64)           # 131072 voxels
K1BIG_R = (33, 64, 62)         # 130944 voxels = 512 tiles of 256 (the last one ragged), W no multiple of 32, D odd

ROWS = [
    # ---- 1x1x1, cfg 0 (sym 8): igemm_kernel<2,1,4,1,4>, tile 32 x 4 x 2, no halo; one staging pass of 32 channels ----
    # 2 -> 32 is the first block's shortcut: Cin is no whole k-group, so k1s_kernel declines.  G = 8: groups of 4 planes = 2 z-tiles, gridy = 1
    row('k1 cfg0 2->32 + GroupNorm sums', FWD, K1, 1, K1BIG, 2, 32, 8, groups=8),
    # the data gradient of the 32 -> 3 head: contraction over 3 channels, 32 written
    row('k1 cfg0 data gradient of 32->3, accumulated', BWD, K1, 1, K1BIG, 32, 3, 8, accumulate=True),
    # whole k-groups reach the tiled kernel only with the streaming kernel's threshold out of reach
    row('k1 cfg0 8->32 behind k1s, no bias, into a slab', FWD, K1, 1, K1BIG, 8, 32, 8, env=NOK1S, bias=False, yslab=True),
    row('k1 cfg0 ragged 5->24, x off its boundary', FWD, K1, 1, K1BIG_R, 5, 24, 8, xslab=True),
    # ---- 1x1x1, cfg 1 (sym 9): igemm_kernel<2,2,4,1,4>, gridy = Npad / 64; below 65536 voxels k1s_kernel declines ----
    # G = 8: groups of 2 planes = 1 z-tile, gridy = 4
    row('k1 cfg1 8->256 + GroupNorm sums', FWD, K1, 1, (16, 32, 64), 8, 256, 9, groups=8),
    row('k1 cfg1 64->256, two staging passes, no bias', FWD, K1, 1, (16, 32, 64), 64, 256, 9, bias=False),
    row('k1 cfg1 data gradient of 256->8, accumulated', BWD, K1, 1, (16, 32, 64), 256, 8, 9, accumulate=True),
    # Cout = 40: Npad = 64, one block whose second 32-wide sub-tile holds 8 channels
    row('k1 cfg1 ragged 5->40, x off its boundary, into a slab', FWD, K1, 1, K1BIG_R, 5, 40, 9, xslab=True, yslab=True),
    # ---- 1x1x1, cfg 2 (sym 10): igemm_kernel<1,2,2,2,4>, tile 32 x 2 x 1, gridy = Npad / 128 ----
    row('k1 cfg2 16->128', FWD, K1, 1, (16, 32, 48), 16, 128, 10),
    row('k1 cfg2 data gradient of 128->16, accumulated', BWD, K1, 1, (16, 32, 48), 128, 16, 10, accumulate=True),
    # Cout = 136: Npad = 160, gridy = 2, the second 128-wide block holds 8 channels.  G = 8: groups of 2 planes = 2 z-tiles
    row('k1 cfg2 16->136 + GroupNorm sums, gridy 2', FWD, K1, 1, (16, 32, 24), 16, 136, 10, groups=8),
    row('k1 cfg2 ragged 12->136, x off its boundary, into a slab, no bias', FWD, K1, 1, (15, 30, 28), 12, 136, 10, bias=False, xslab=True,
        yslab=True),
    # ---- 1x1x1, the small tilings the model's deep levels run (sym 11: <1,1,2,2,4>, sym 12: <1,1,4,1,4>) ----
    row('k1 cfg3 ragged 12->40', FWD, K1, 1, (6, 10, 14), 12, 40, 11, xslab=True, yslab=True),
    row('k1 cfg3 data gradient of 40->12, accumulated', BWD, K1, 1, (6, 10, 14), 40, 12, 11, accumulate=True, xslab=True, yslab=True),
    row('k1 cfg4 ragged 12->20', FWD, K1, 1, (5, 6, 7), 12, 20, 12, xslab=True, yslab=True),
    # ---- stride-2 geometry (27 taps at stride 2, T27; TX <= 8: IX = 2 TX + 1), cfg 2 (sym 2): igemm_kernel<1,2,2,2,1,false,false,true> ----
    # output 4^3 = one 4 x 4 x 4 tile, halo 9 x 9 x 9; KG = 2: no split
    row('down cfg2 16->128', FWD, K3S2, 1, (8, 8, 8), 16, 128, 2),
    # KG = 16 on one tile: split over blockIdx.z, partials in the workspace
    row('down cfg2 128->128 split-K', FWD, K3S2, 1, (8, 8, 8), 128, 128, 2, splitk=True),
    # the data gradient of the transposed conv is the stride-2 conv of dy (8^3 -> 4^3)
    row('down cfg2 data gradient of transposed 128->16, accumulated', BWD, K3S2T, 1, (4, 4, 4), 128, 16, 2, accumulate=True),
    # output 3 x 5 x 7 in a 4 x 4 x 4 tiling, Npad = 160: gridy = 2
    row('down cfg2 ragged 12->136, x off its boundary, into a slab, no bias', FWD, K3S2, 1, (6, 10, 14), 12, 136, 2, bias=False, xslab=True,
        yslab=True),
    row('down cfg3 ragged 12->20', FWD, K3S2, 1, (4, 6, 10), 12, 20, 3, xslab=True, yslab=True),
    row('down cfg3 data gradient of transposed 20->12', BWD, K3S2T, 1, (2, 3, 5), 20, 12, 3, xslab=True, yslab=True),
    # ---- the 8 output-parity classes (blockIdx.z = class, 1 / 2 / 4 / 8 taps from tables, halo TX + 1) where upm_kernel declines: a
    #      contraction that is no whole k-group ----
    # cfg 1 (sym 1): igemm_kernel<2,2,4,1,1>; 8 classes x 16 tiles x 4 blocks = 512
    row('up cfg1 4->256', FWD, K3S2T, 1, (8, 16, 32), 4, 256, 1),
    row('up cfg1 1->256, the VAE\'s first transposed conv at batch 8', FWD, K3S2T, 8, (8, 8, 8), 1, 256, 1),
    # cfg 0 (sym 0): igemm_kernel<2,1,4,1,1>; 8 classes x 64 tiles
    row('up cfg0 4->32', FWD, K3S2T, 1, (16, 32, 32), 4, 32, 0),
    row('up cfg0 ragged 3->24, x off its boundary, into a slab, no bias', FWD, K3S2T, 1, (17, 31, 31), 3, 24, 0, bias=False, xslab=True,
        yslab=True),
    # cfg 2 (sym 2): igemm_kernel<1,2,2,2,1>; Npad = 128: 8 x 48 tiles of 64 = 384, 8 x 12 x 2 = 192 < 512
    row('up cfg2 4->128', FWD, K3S2T, 1, (8, 16, 24), 4, 128, 2),
    # Npad = 160: 8 x 25 x 2 = 400 blocks of cfg 2, 8 x 7 x 3 = 168 < 512
    row('up cfg2 ragged 4->136, x off its boundary, into a slab', FWD, K3S2T, 1, (5, 12, 26), 4, 136, 2, xslab=True, yslab=True),
    # the data gradient of the stride-2 conv gathers over the fine grid's parity classes (the model's 16^3 1024 -> 16); dy 4 x 8 x 24 = 768
    # voxels, 512 channels written: 8 x 12 x 4 = 384
    row('up cfg2 data gradient of stride-2 512->12, accumulated', BWD, K3S2, 1, (8, 16, 48), 512, 12, 2, accumulate=True),
    row('up cfg3 1->40', FWD, K3S2T, 1, (2, 3, 5), 1, 40, 3, xslab=True, yslab=True),
    row('up cfg1 ragged 3->40, x off its boundary, into a slab', FWD, K3S2T, 1, (17, 31, 31), 3, 40, 1, xslab=True, yslab=True),
    # ---- 3x3x3 stride 1 behind the Winograd forms, cfg 0 (sym 0) ----
    # the sigmoid flag alone keeps the Winograd forms off; TX = 32, TY = 4: IX = 34, IY = 6 -> FIXG <2,1,4,1,1,false,true>, three workgroups a CU
    row('s1 cfg0 fixed geometry, sigmoid, default switches', FWD, K3S1, 1, BIG, 8, 8, 0, sigmoid=True),
    # the row the full-size form-agreement tests lean on: two single-buffered staging passes
    row('s1 cfg0 fixed geometry 16->32', FWD, K3S1, 1, BIG, 16, 32, 0, env=NOWINO),
    # W = 16: TX = 16, IX = 18 -> T27 <2,1,4,1,1,false,false,true>, tile 16 x 4 x 4.  G = 4: groups of 32 planes = 8 z-tiles
    row('s1 cfg0 27-tap form + GroupNorm sums', FWD, K3S1, 1, THIN, 8, 8, 0, env=NOWINO, groups=4),
    # an x off its boundary sends the call to the tiled kernel under default switches
    row('s1 cfg0 fixed geometry, ragged 8->24, x off its boundary, into a slab', FWD, K3S1, 1, BIG_R, 8, 24, 0, xslab=True, yslab=True),
    row('s1 cfg0 27-tap form, ragged 8->24, no bias', FWD, K3S1, 1, THIN_R, 8, 24, 0, env=NOWINO, bias=False, xslab=True, yslab=True),
    # FUSE2 + FIXG <2,1,4,1,1,true,true>: the second accumulator set beside two M sub-tiles
    row('s1 cfg0 fixed geometry + fused shortcut', FWD, K3S1, 1, BIG, 8, 32, 0, env=NOWINO, second=Y2),
    # FUSE2 without the fixed geometry <2,1,4,1,1,true>
    row('s1 cfg0 27-tap form + fused shortcut', FWD, K3S1, 1, THIN, 8, 8, 0, env=NOWINO, second=Y2),
    row('s1 cfg0 data gradient, accumulated', BWD, K3S1, 1, BIG, 8, 16, 0, env=NOWINO, accumulate=True),
    # the second input at the centre tap (x2 rows from global memory), fixed geometry
    row('s1 cfg0 data-gradient pair', BWD, K3S1, 1, BIG, 8, 8, 0, env=NOWINO, second=X2),
    # ---- 3x3x3 stride 1, cfg 1 (sym 1): 64 accumulators a lane ----
    # FIXG <2,2,4,1,1,false,true>
    row('s1 cfg1 fixed geometry 8->256', FWD, K3S1, 1, (8, 32, 128), 8, 256, 1, env=NOWINO),
    # no registers for the second accumulator set: the query and the call answer BTS_ERR_UNSUPPORTED, can_fuse 0
    row('s1 cfg1 fused shortcut is refused', FWD, K3S1, 1, (8, 32, 128), 8, 256, UNSUPPORTED, env=NOWINO, second=Y2),
    # T27 <2,2,4,1,1,false,false,true>; Cout = 40: the second 32-wide sub-tile holds 8 channels
    row('s1 cfg1 27-tap form, ragged 4->40, x off its boundary, into a slab, no bias', FWD, K3S1, 1, THIN_R, 4, 40, 1, bias=False, xslab=True,
        yslab=True),
    # G = 8: groups of 2 planes = 1 z-tile of the 32 x 4 x 2 tile, gridy = 4
    row('s1 cfg1 fixed geometry 4->256 + GroupNorm sums', FWD, K3S1, 1, (16, 32, 64), 4, 256, 1, env=NOWINO, groups=8),
    row('s1 cfg1 data gradient of 40->8, accumulated', BWD, K3S1, 1, BIG, 40, 8, 1, env=NOWINO, accumulate=True),
    row('s1 cfg1 data-gradient pair of 40->8', BWD, K3S1, 1, BIG, 40, 8, 1, env=NOWINO, second=X2),
    # ---- 3x3x3 stride 1, cfg 2 (sym 2): T27 <1,2,2,2,1,false,false,true>, tile 32 x 2 x 1, 12288 voxels x 2 blocks = 384 ----
    row('s1 cfg2 8->256', FWD, K3S1, 1, (8, 32, 48), 8, 256, 2, env=NOWINO),
    row('s1 cfg2 + fused shortcut', FWD, K3S1, 1, (8, 32, 48), 8, 256, 2, env=NOWINO, second=Y2),
    row('s1 cfg2 data-gradient pair of 256->8', BWD, K3S1, 1, (8, 32, 48), 256, 8, 2, env=NOWINO, second=X2),
    row('s1 cfg2 data gradient of 256->8, accumulated', BWD, K3S1, 1, (8, 32, 48), 256, 8, 2, env=NOWINO, accumulate=True),
    # Npad = 160: gridy = 2.  G = 8: groups of 2 planes = 2 z-tiles
    row('s1 cfg2 8->136 + GroupNorm sums, gridy 2', FWD, K3S1, 1, (16, 32, 24), 8, 136, 2, env=NOWINO, groups=8),
    row('s1 cfg2 ragged 8->136, x off its boundary, into a slab, no bias', FWD, K3S1, 1, (15, 30, 28), 8, 136, 2, bias=False, xslab=True,
        yslab=True),
    # ---- 3x3x3 stride 1, cfg 3 (sym 3), the deep levels with the Winograd forms off: every form once ----
    row('s1 cfg3 ragged 12->40', FWD, K3S1, 1, (6, 10, 14), 12, 40, 3, env=NOWINO, xslab=True, yslab=True),
    row('s1 cfg3 + fused shortcut', FWD, K3S1, 1, (6, 10, 14), 12, 40, 3, env=NOWINO, second=Y2),
    row('s1 cfg3 data gradient of 40->16, accumulated', BWD, K3S1, 1, (6, 10, 14), 40, 16, 3, env=NOWINO, accumulate=True),
    row('s1 cfg3 data-gradient pair of 40->16', BWD, K3S1, 1, (6, 10, 14), 40, 16, 3, env=NOWINO, second=X2),
]


def by_name():
    return {r.name: r for r in ROWS}


def operands(r):
    """(ldx, ldy, flags, ld2, aligned, workspace_bytes) of bts_conv3d_kernel for the call the GPU test makes of row r: ldx / ldy are the
    rows of the forward input / output (the data gradient writes the former and reads the latter)"""
    c_read, c_written = (r.cin, r.cout) if r.direction == FWD else (r.cout, r.cin)
    ld_read = c_read + 3 if r.xslab else c_read
    ld_written = c_written + 8 if r.yslab else c_written
    ldx, ldy = (ld_read, ld_written) if r.direction == FWD else (ld_written, ld_read)
    flags = (1 if r.sigmoid else 0) | (2 if r.accumulate else 0)
    aligned = (0 if r.xslab else 1) | 2 | 4 | 8
    # (bts_conv3d_fwd_fused2 takes no workspace; every other call passes what its query asks for)
    return ldx, ldy, flags, (r.cout if r.second else 0), aligned, (0 if r.second == Y2 else -1)


def named(L, r):
    """bts_conv3d_kernel's answer for row r (L: the ctypes library, the row's switches already in the environment)"""
    ldx, ldy, flags, ld2, aligned, ws = operands(r)
    d, h, w = r.dims
    return L._bts_conv3d_kernel(r.direction, r.kind, r.n, d, h, w, r.cin, ldx, r.cout, ldy, flags, r.second, ld2, r.groups, aligned, ws)


def workspace(L, r):
    d, h, w = r.dims
    q = L._bts_conv3d_fwd_workspace if r.direction == FWD else L._bts_conv3d_bwd_data_workspace
    return q(r.kind, r.n, d, h, w, r.cin, r.cout)


def key(r):
    """what the completeness test matches a layer against"""
    return (r.direction, r.kind, r.second, r.sym)
