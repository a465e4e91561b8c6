"""References, fp32 restatements and error bounds for the fp32 normalisation and gate kernels: csrc/groupnorm.hip (bts_gn_stats,
bts_gn_apply, bts_gn_bwd), the gate half of csrc/se.hip (bts_se_mlp_fwd, bts_block_epilogue_fwd, bts_se_bwd) and csrc/block_bwd.hip
(bts_block_bwd).  Plain Python on the CPU, in the pattern of tests/step_ref.py and tests/lowp_ref.py.

For every kernel: the fp64 REFERENCE, an fp32 RESTATEMENT of the formula its source documents (torch float32 on the CPU, in the
documented order, products and sums as written, no fma unless the source writes one) and a BOUND.  Tensors are (N, V, C) with
V = D H W; modes are SLAB = 0 (the raw channels_last reshape: group g is the g-th contiguous 1/G of a sample's memory, affine index
g * C/G + c mod C/G) and CHANNEL = 1 (textbook GroupNorm).

RULES (step_ref's and lowp_ref's).  Scalars are rounded to fp32 as the ABI receives them (eps).  The mean, rstd, ch, sp, gap and h
handed to a later kernel are INPUTS: the reference takes the fp32 values the kernel was given.  What an input (or a value the kernel
itself formed earlier) carries is added ONCE, outside the K of the operation it enters: no K multiplies another.  No K and no bound
comes from a run of a kernel.  Every entry below returns ABSOLUTE bounds with each K applied once; tests/test_norm_kernels_gpu.py
holds a kernel to 1.0 of its bound (= to its K), tests/test_norm_kernels_host.py a restatement to 1/4 (= to K/4), or to the bound
itself for the bounds WITHOUT a K (NO_K below).

THE Ks, from the count of roundings (eps32 = 2^-24; B = the sum of the absolute values of the terms that are added):
K_STATS = 16, bts_gn_stats.  Slab mode loads 4 values and forms (v0 + v1) + (v2 + v3) and (v0^2 + v1^2) + (v2^2 + v3^2) in fp32,
  then adds in fp64: a value passes 2 roundings into the sum, a square 3.  Channel mode and the generic kernel square and add in
  fp64 (exact to 2^-53).  One rounding at the end.  mean: 2 eps32 E|x| + eps32 |mean| <= 3 eps32 E|x|, bound K_STATS eps32 E|x|.
  var = E[x^2] - mean^2 in fp64: |d var| <= 3 eps32 E[x^2] + 2 |mean| 2 eps32 E|x| <= 3 eps32 E[x^2] + 2 eps32 (E[x^2] + mean^2)
  <= 5 eps32 (E[x^2] + mean^2); bound K_STATS eps32 (E[x^2] + mean^2): the cancellation of E[x^2] - mean^2 is paid for where it
  happens.  K/4 = 4 is below the worst case 5, which needs every rounding of a unit at its maximum and of one sign; the
  roundings of L/4 loads are independent (rms eps32 B sqrt(4 / L)).
  rstd = (var + eps)^-1/2:  |d rstd| <= rstd^3 |d var| / 2 (exact for d var >= 0, the function is convex and decreasing; for d var < 0
  to first order, the second-order term is 3/4 rstd^5 dvar^2, below 1e-6 of the first at the listed inputs; at a constant volume
  var = 0 is clamped from below, d var >= 0) plus the last rounding eps32 rstd, outside K.
K_EW = 16, element-wise forms (bts_gn_apply, dx of the backward kernels, out of the epilogue, dres): lowp_ref's K_LP.
  gn_apply general form ((x - m) rs gamma) + beta: 4 roundings, each on a quantity <= B = |x - m| rs |gamma| + |beta|; streaming form
  fma(x - m, rs gamma, beta): 3.  dx = (dE gamma - c1 - xh c2) rs with xh = (x - m) rs: on |dE gamma| 4 roundings (product, two
  subtractions, the product with rs), on |c1| 3, on |xh c2| 5 (two of xh, the product, one subtraction, rs): <= 5 eps32 B,
  B = (|dE gamma| + |c1| + |xh c2|) rs.  out = res (sp + ch) + relu(y): the sum, the product, the addition and y's 4: <= 4 on each
  term.  dres = dout (sp + ch) + ds wsp + dgap: <= 4.  K/4 = 4: a form of 4 roundings cannot pass it, one of 5 only with every
  rounding at its maximum and of one sign.
K_RED = 16, fp64 sums of fp32-rounded terms (A_j = sum dE xh of GroupNorm's backward: 3 roundings per term -- two of xh and the
  product; the gate's Pch = sum dout res and Pw = sum ds res: 1 per term): <= 3 eps32 B, B = the sum of the |terms|; K/4 = 4 holds
  rigorously.  The one rounding of the fp32 result (two when the call accumulates: eps32 (|old| + |v|) more) is added outside K.
K_DOT = 16 (lowp_ref's K_LP for dot products), fp32 dot products: the gate's res . wsp and dout . res (a 4-term pair sum per lane,
  then a butterfly over F/4 lanes: 3 + log2(F/4) <= 9 roundings on partial sums <= B) and the SE-MLP's fma chains (F / (256 / R)
  terms per slice, 256 / R slices added in order; then R terms).  The roundings act on partial sums and are independent: rms
  eps32 B / 2 sqrt(n / 3) <= 1.7 at the longest chain (32 terms).  Chains of >= 24 terms are held to lowp_ref's
  LONG_CHAIN_HOST_LIMIT (K/2) on the host, as lowp_ref's finding explains; the kernels to K.
K_GATE = 16 (lowp_ref's, with its derivation): sp and ch, sigmoids.  common.h's sigmoidf_ is 1 / (1 + expf(-a)); expf is at least as
  accurate as the __expf the derivation assumes, so lowp_ref.sigmoid_bound holds as it stands.  |a| <= GATE_MAX_ARG is asserted.
NO_K: bounds without a K, fp64 accumulation of EXACT terms and one rounding: dbeta (sum of dE), c1.  eps32 |v| + 1e-12 sum |terms|.
  FINDING of the GPU run, fixed in the kernel (no number was raised): the generic route (gn_bwd_group_generic_kernel) formed c1 as
  the fp64 sum of fp32 products dE * gamma, one rounding per term where the documented c1 = sum_j gamma_j B_j / L has none.  At
  (1,(48,48,48),20,4), channel mode, relu 1, one group's c1 cancels to 7e-6 of sum |dE gamma| / L = 0.4: the 553,000 roundings
  left 70 eps32 |c1| on it, and dx, which is -(c1 + xh c2) rstd where dE = 0, missed its bound by 3.76 at the 21 elements with
  |xh| < 3e-5.  The kernel now multiplies by gamma in fp64, as the vectorised route does (same figures as its neighbours: 0.21).
  The same holds for the fp32 addition old + v of an accumulating call: one rounding of up to eps32 |old + v| with no margin in
  it, so the host test holds the parameter gradients of an ACCUMULATING call to the bound itself (step_ref's rule for colsum).

THE ReLU MASK [y > 0] of bts_gn_bwd (relu = 1) and bts_block_bwd.  The kernels evaluate y = xh gamma + beta in fp32.  An element is
UNDECIDED when its fp64 |y| is within the forward bound K_EW eps32 (|xh gamma| + |beta|).  For dx / dc2 either branch is accepted
at an undecided element (ratio_either).  Each sum an undecided element enters (A_j, B_j and, through them, dgamma, dbeta, c1, c2
and every dx of the unit) gets that element's |term| added to its bound, in full: the kernel may have taken the other branch, and
then the sum differs by the whole term, not by eps32 of it.  (Adding the term inside a K eps32 B would allow nothing: a cap above
zero only makes sense with the term itself.)  Nothing is left out of a comparison.  The share of undecided elements is capped at
UNDECIDED_CAP = 1e-5 per case -- a condition on the INPUT, asserted from the reference alone by the host test for every listed
input (a seed that breaks it is replaced; the seed is an input, not a tolerance).  h > 0 in the gate's backward is decided by the
fp32 h the kernel is handed: exact.

SEAMS.  The inputs of the reductions carry outliers on the first and last item of every unit and of every block span (computed as
gn_geom and se_bwd_blocks compute them) and either side of the last whole trip of a span (1024 elements; the generic kernel: 256;
the gate: 256 / (F/4) voxels).  An item is what one lane loads: 4 consecutive elements (vectorised kernels), 1 element (generic),
one voxel (gate).  tests/test_norm_kernels_host.py asserts on the reference alone that dropping or double-counting any ONE seam item
moves some output by at least 8 of its bounds.  At a GroupNorm seam dy = M and x = centre + M (gamma > 0) or centre - 2 M
(gamma < 0), so the item survives the ReLU mask; where more than a quarter of a tensor is seams (units of 2 or 16 elements) x
stays random, and an item the mask removes is worth 8 bounds of the statistics and of the relu = 0 backward only.  At a gate
seam dout = res = M on every channel.

WHAT THE LISTED SHAPES DO NOT REACH (by reading the host code):
  * gn_apply_slab_stream / gn_bwd_apply_slab_stream / blk_bwd_apply falling back because N G L / 1024 / cpb > 0x7fffffff blocks:
    2^41 elements.  Not reachable in memory.
  * bts_gn_finalize_partials_ (the conv epilogue's entry) and its wide kernel (B >= 512): belongs to the conv tests.
  * gn_stats_channel_kernel's `P4 <= 256` is always true for C <= 1024; C > 1024 is generic by gn_geom.
  * gn_bwd_reduce_kernel's 4096-element unrolled trip needs a span >= 4096 (a unit above 256 * 3072 elements): reached in channel
    mode only, at (1,(32,32,48),64,8) (span 12288) and (1,(64,64,66),32,8) (span 33792); in slab mode the widest span is 2048 (the
    2048 trip).
  * se_mlp_fwd's R > 256 branch: no model has R > 32.
  * se_bwd_reduce's four-voxel unrolled trip is reached only where vspan >= 4 vpb: (1,(64,64,66),32,4) has vspan 544, vpb 32.
  * se_mlp_bwd_kernel (one block: N = 1 and F R < 2048) and the sample / param pair are both reached; B > 64 * 8 of
    se_bwd_partial_reduce's eight-load trip needs more than 512 partial rows per sample: reached only by the fused route at
    (1,(32,32,48),64,8,8) (G B = 8 * 192 rows).
  * colsum (the GAP) is step_ref's.
  * workspaces above 2^31 bytes and every `long` index past 2^31 elements: the full-size model tests.

MEASURED RESTATEMENT RATIOS, on the CPU (tests/test_norm_kernels_host.py -s; max over every listed shape, both modes, relu 0 and 1, the
three kinds of input; fraction of the bound, limit 1/4 = K/4; x 16 gives eps32 B for the single-K bounds):
  gn_stats  mean 0.059 (offset input, ragged slab), rstd 0.090; constant volume 0 / 0 (the clamp: rstd is exactly fl32(eps^-1/2))
  gn_apply  general form 0.225 = 3.6 eps32 B at (1,(32,32,48),64,8) (3.1e6 elements of a form of 4 roundings), streaming form 0.161
  gn_bwd    dx 0.225 (the same shape), dgamma 0.136; accumulating 0.098 (limit 1); dbeta 0.999 of its NO_K bound (limit 1: the one
            rounding at its worst over 1024 channels)
  se_mlp    h 0.053, ch 0.059; chains of >= 24 terms (5,256,32): h 0.033, ch 0.024 (limit 1/2)
  epilogue  sp 0.088, out 0.220 (8.6e6 elements)
  se_bwd    ds 0.181, dres 0.172, dgap 0.010, dw1 0.024, dw2 0.058, dwsp 0.029; accumulating calls (limit 1: the fp32 addition onto
            |old| ~ 1 is one rounding without a margin): dw1 0.291, dw2 0.523, dwsp 0.054
  Nothing is above its limit: no finding on the host.
CONTROL (run once on the CPU, restatements only, (3,(6,10,14),16,8) slab, relu 1; the test that keeps it is
test_control_dropped_element_and_wrong_divisor_fail_the_gpu_side_bound): a restatement that drops the last element of the ragged
second span of unit (0, 1) puts the statistics 2.08e4 and dgamma / dbeta 1.34e6 bounds away; one that divides c1's sum by L - 1
puts dx 588 bounds away.  Both are held to 1 on the GPU.

MEASURED GPU RATIOS, on an MI355X (tests/test_norm_kernels_gpu.py -s, 134 cases; max per kernel and output; fraction of the bound,
limit 1 = K):
  gn_stats  mean 0.059, rstd 0.090 (the restatement's figures to the digit)
  gn_apply  0.171      gn_bwd  dx 0.230 (generic route past its block cap), dgamma 0.569 (accumulating, C = 1024; 0.136 else), dbeta 0.999
  se_mlp    h 0.053, ch 0.059      epilogue  sp 0.088, out 0.189
  se_bwd    ds 0.181, dres 0.176, dgap 0.012, dw1 0.047, dw2 0.098, dwsp 0.054
  bts_block_bwd   dc2 0.156, dgamma 0.128, dbeta 0.990, ds 0.199, dres 0.112, dgap 0.009, dw1 0.063, dw2 0.189, dwsp 0.041
  the two-kernel route on the same tensors: the same figures except dres 0.146
  Before the fix of the FINDING above: gn_bwd dx 3.761 at (1,(48,48,48),20,4), channel mode, relu 1.  Nothing else was above 1.
"""
import math

import torch

from oracle import torch_ref as R  # noqa: F401  (the host test pins the references to it)
from step_ref import EPS32, TINY, check, f32, fma32, ratio  # noqa: F401
import lowp_ref as LP

F64 = torch.float64
F32 = torch.float32
SLAB, CHANNEL = 0, 1

K_STATS = 16
K_EW = LP.K_LP
K_RED = 16
K_DOT = LP.K_LP
K_GATE = LP.K_GATE
LONG_CHAIN_HOST_LIMIT = LP.LONG_CHAIN_HOST_LIMIT
NO_K = ('dbeta',)
UNDECIDED_CAP = 1e-5
GN_EPS = 1e-5



def cdiv(a, b):
    return (a + b - 1) // b


# ----------------------------------------------------------------------------------------------------------------
# the host code's block arithmetic, restated (csrc/groupnorm.hip gn_geom, gn_stream_cpb; csrc/se.hip se_bwd_blocks)
# ----------------------------------------------------------------------------------------------------------------
def gn_geom(n, v, c, g, mode):
    E = v * c
    L = E // g
    generic = c % 4 != 0 or (c & (c - 1)) != 0 or c > 1024 or L % 4 != 0
    unit = L if mode == SLAB else E
    units = n * g if mode == SLAB else n
    B = min(cdiv(2048, units), 256)
    span = cdiv(cdiv(unit, B), 1024) * 1024
    return dict(E=E, L=L, cg=c // g, generic=generic, unit=unit, units=units, span=span, B=cdiv(unit, span))


def gn_stream_cpb(n, v, c, g, mode, ld=None):
    """chunks per block of the streaming apply kernels, or 0 where the general / generic kernel runs"""
    q = gn_geom(n, v, c, g, mode)
    ld = c if ld is None else ld
    if q['generic'] or ld % 4 != 0 or mode != SLAB or q['L'] % 1024 != 0 or 1024 % c != 0:
        return 0
    cpu = q['L'] // 1024
    cpb = 8
    while cpb > 1 and cpu % cpb != 0:
        cpb //= 2
    return cpb


def se_bwd_blocks(v, n, f):
    vpb = 256 // (f // 4)
    B = min(cdiv(1024, n), 512)
    span = cdiv(cdiv(v, B), vpb) * vpb
    return cdiv(v, span), span, vpb


def block_bwd_plan(n, v, f, r, g):
    """blk_bwd_plan of csrc/block_bwd.hip: does the fused backward take the shape?"""
    if n <= 0 or v <= 0 or r <= 0 or g <= 0 or f < 4 or f > 256 or (f & (f - 1)) != 0 or f % g != 0:
        return False
    L = v * f // g
    cg = f // g
    if (v * f) % g != 0 or L % 1024 != 0 or 1024 % f != 0 or 256 % cg != 0:
        return False
    return not gn_geom(n, v, f, g, SLAB)['generic']


def _span_seams(lo, hi, trip, width):
    """first and last item of [lo, hi) and either side of its last whole trip (positions of the item's first element)"""
    s = {lo, hi - width}
    t = lo + (hi - lo) // trip * trip
    for i in (t - width, t):
        if lo <= i < hi:
            s.add(i)
    return s


def gn_index(v, c, g, mode):
    """-> grp, idx: (V*C,) long, the group and the affine index of every element of one sample"""
    r = torch.arange(v * c)
    ch = r % c
    cg = c // g
    if mode == SLAB:
        grp = r // (v * c // g)
        return grp, grp * cg + ch % cg
    return ch // cg, ch


def gn_seams(n, v, c, g, mode):
    """(items, width) long: flat indices into x.reshape(-1) of every seam item"""
    q = gn_geom(n, v, c, g, mode)
    E, L, cg = q['E'], q['L'], q['cg']
    items = []
    if q['generic']:
        for u in range(n * g):
            nn, gg = divmod(u, g)
            for e in sorted(_span_seams(0, L, 256, 1)):
                off = gg * L + e if mode == SLAB else (e // cg) * c + gg * cg + e % cg
                items.append([nn * E + off])
        return torch.tensor(items)
    for u in range(q['units']):
        base = u * q['unit']
        pos = set()
        for b in range(q['B']):
            lo = b * q['span']
            pos |= _span_seams(lo, min(lo + q['span'], q['unit']), 1024, 4)
        for p in sorted(pos):
            items.append([base + p + e for e in range(4)])
    return torch.tensor(items)


def se_seams(n, v, f):
    """seam voxels (index into the N*V voxels) of bts_se_bwd's reduce pass"""
    B, span, vpb = se_bwd_blocks(v, n, f)
    pos = set()
    for b in range(B):
        lo = b * span
        pos |= _span_seams(lo, min(lo + span, v), vpb, 1)
    return torch.tensor([nn * v + p for nn in range(n) for p in sorted(pos)])


def blk_seams(n, v, f, g):
    """seam voxels of the fused reduce pass: its blocks are GroupNorm's slab spans"""
    it = gn_seams(n, v, f, g, SLAB)
    return torch.unique(it[:, 0] // f)


def seam_outlier(L):
    """M: dropping an item of 4 M^2 from E[x^2] must move rstd by 8 bounds: M^2 >= 2.2e-6 L (E[x^2] + mean^2), see gn_stats_ref;
    8 up to L = 2^18 (needs 2.7 at E[x^2] + mean^2 = 5), 32 beyond (needs 3.4 at the 1.08e6 elements of the largest unit)"""
    return 32.0 if L >= (1 << 18) else 8.0


# ----------------------------------------------------------------------------------------------------------------
# shapes (N, (D, H, W), C, G): each the smallest that reaches its path (worked out from the host code above)
# ----------------------------------------------------------------------------------------------------------------
GN_SHAPES = [
    (1, (1, 1, 1), 16, 8),        # generic: L = 2
    (2, (2, 4, 2), 12, 3),        # generic: C not a power of two
    (2, (4, 4, 4), 2, 2),         # generic: C % 4 != 0
    (1, (2, 2, 2), 16, 8),        # vectorised, one block shorter than a trip (L = 16)
    (3, (6, 10, 14), 16, 8),      # vectorised, ragged: slab L = 1680 (spans 1024 + 656), channel E = 13440 (14 spans, the last 128)
    (1, (4, 6, 8), 128, 8),       # streaming, cpb = 1
    (1, (8, 8, 12), 64, 8),       # streaming, cpb = 2
    (1, (8, 8, 8), 64, 8),        # streaming, cpb = 4
    (1, (16, 16, 16), 16, 8),     # streaming, cpb = 8
    (1, (2, 2, 2), 1024, 2),      # widest vectorised C; cg = 512: the two-stage finalize in slab mode
]
GN_SHAPE_BLOCK_CAP = (1, (32, 32, 48), 64, 8)        # slab: 256-block cap in force, span 2048, B = 192
GN_SHAPE_GENERIC_CAP = (1, (48, 48, 48), 20, 4)      # generic apply kernels past 8192 blocks (2,211,840 elements)
GN_SHAPE_VECTOR_CAP = (1, (64, 64, 66), 32, 8)       # channel mode: vectorised apply kernels past 8192 blocks (8,650,752 elements)
GN_SHAPE_RAGGED = (3, (6, 10, 14), 16, 8)
GN_SHAPE_STREAM = (1, (8, 8, 12), 64, 8)
GN_CONSTANT_SHAPES = [(1, (2, 2, 2), 16, 8), (1, (4, 6, 8), 128, 8)]

# (N, (D, H, W), F, R, G)
GATE_SHAPES = [
    (1, (1, 1, 1), 4, 1, 4),          # one lane per voxel, V < vpb
    (3, (6, 10, 14), 16, 2, 8),       # 14 reduce blocks of 64 voxels, the last holding 8
    (1, (2, 2, 3), 256, 32, 8),       # a whole wave per voxel
    (2, (4, 4, 8), 64, 8, 8),
]
GATE_SHAPE_CAP = (1, (64, 64, 66), 32, 4, 8)      # past the 8192-block caps of the epilogue and of se_bwd_apply
MLP_SHAPES = [(5, 256, 32), (1, 4, 1)]
BLOCK_SHAPES = [
    (1, (8, 8, 16), 4, 1, 4),         # cg = 1, F = 4
    (1, (1, 2, 2), 256, 32, 1),       # cg = 256, one chunk per unit
    (3, (4, 6, 8), 128, 16, 8),       # cpb = 1, N odd
    (2, (8, 8, 12), 64, 8, 8),        # cpb = 2
]
BLOCK_SHAPE_CAP = (1, (32, 32, 48), 64, 8, 8)     # block cap in force, span 2048


def nvox(dims):
    return dims[0] * dims[1] * dims[2]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_inputs(shape, mode, kind='wide', seed=0, seams=True):
    """x, dy (N, V, C), gamma, beta (C).  kind: 'wide' 0.5 + 2 randn; 'offset' 8 + 0.5 randn (E[x^2] - mean^2 cancels);
    'constant' a value whose fp32 square rounds DOWN (E[x^2] - mean^2 < 0 in the kernel: the clamp).  |gamma| in [0.5, 1.5) with
    random sign so that a seam item can be placed on the positive side of the ReLU."""
    n, dims, c, g = shape
    v = nvox(dims)
    gen = _gen(9000 + seed)
    gamma = (0.5 + torch.rand(c, generator=gen)) * torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
    beta = 0.2 * torch.randn(c, generator=gen)
    if kind == 'constant':
        x = torch.full((n, v, c), CONSTANT_VALUE, dtype=F32)
    elif kind == 'offset':
        x = 8.0 + 0.5 * torch.randn((n, v, c), generator=gen)
    else:
        x = 0.5 + 2.0 * torch.randn((n, v, c), generator=gen)
    dy = torch.randn((n, v, c), generator=gen)
    if seams and kind != 'constant':
        it = gn_seams(n, v, c, g, mode).reshape(-1)
        _, idx = gn_index(v, c, g, mode)
        M = seam_outlier(gn_geom(n, v, c, g, mode)['L'])
        centre = 8.0 if kind == 'offset' else 0.5
        sgn = torch.sign(gamma[idx[it % (v * c)]])
        if 4 * it.numel() <= x.numel():      # (a unit that is all seams has no "outliers": x stays random there, dy carries M)
            x.view(-1)[it] = centre + torch.where(sgn > 0, M, -2.0 * M)
        dy.view(-1)[it] = M
    return x, dy, gamma.float(), beta.float()


def _constant_value():
    """the first of a few candidates whose fp32 square lies BELOW the exact square"""
    for cand in (3.3, 1.7, 2.9, 0.7):
        x = torch.tensor(cand, dtype=F32)
        if float((x * x).double()) < float(x.double() * x.double()):
            return float(x)
    raise AssertionError('no candidate rounds down')


CONSTANT_VALUE = _constant_value()


# ----------------------------------------------------------------------------------------------------------------
# GroupNormalization statistics
# ----------------------------------------------------------------------------------------------------------------
def _unit_of(n, v, c, g, mode):
    """(N*V*C,) long: the (sample, group) unit of every element"""
    grp, _ = gn_index(v, c, g, mode)
    return (torch.arange(n)[:, None] * g + grp[None, :]).reshape(-1)


def _usum(t, unit, units):
    return torch.zeros(units, dtype=F64).index_add_(0, unit, t.reshape(-1).double())


def gn_stats_from_sums(s, q, count, eps):
    """fp64 sums -> mean, rstd.  var = E[x^2] - mean^2 only HERE (the kernel's form, and the seam test perturbs sums); the reference
    itself takes the two-pass variance."""
    m = s / count
    var = torch.clamp(q / count - m * m, min=0.0)
    return m, 1.0 / torch.sqrt(var + eps)


def gn_stats_bounds(mean, rstd, ea, e2):
    return K_STATS * EPS32 * ea + TINY, K_STATS * EPS32 * 0.5 * rstd ** 3 * (e2 + mean * mean) + EPS32 * rstd + TINY


def gn_stats_ref(x, g, mode, eps=GN_EPS, abi_eps=True):
    """x (N, V, C) -> dict mean, rstd (N*G,) fp64, b_mean, b_rstd absolute, and the raw sums s, q, L.  abi_eps False: eps as the
    fp64 oracle takes it (only for pinning the reference to the oracle; a kernel receives fl32(eps))"""
    n, v, c = x.shape
    eps = f32(eps) if abi_eps else eps
    unit = _unit_of(n, v, c, g, mode)
    L = float(v * c // g)
    xd = x.double().reshape(-1)
    s = _usum(xd, unit, n * g)
    mean = s / L
    var = _usum((xd - mean[unit]) ** 2, unit, n * g) / L
    rstd = 1.0 / torch.sqrt(var + eps)
    ea, q = _usum(xd.abs(), unit, n * g) / L, _usum(xd * xd, unit, n * g)
    bm, br = gn_stats_bounds(mean, rstd, ea, q / L)
    return dict(mean=mean, rstd=rstd, b_mean=bm, b_rstd=br, s=s, q=q, L=L, ea=ea, eps=eps)


def gn_stats_f32(x, g, mode, eps=GN_EPS, drop=None):
    """groupnorm.hip:49-127.  Vectorised slab kernel: per load (v0 + v1) + (v2 + v3) and the same tree of the four squares in fp32,
    fp64 from there.  Channel mode and the generic kernel: fp64 throughout.  E[x^2] - mean^2 clamped at 0, one rounding.
    drop: a flat element index left out of the sums (the control)."""
    n, v, c = x.shape
    q = gn_geom(n, v, c, g, mode)
    L = float(q['L'])
    keep = torch.ones(x.numel(), dtype=F32)
    if drop is not None:
        keep[drop] = 0.0
    xs = x.reshape(-1) * keep
    if mode == SLAB and not q['generic']:
        w = xs.reshape(n * g, -1, 4)
        a = (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])
        w2 = w * w
        b = (w2[..., 0] + w2[..., 1]) + (w2[..., 2] + w2[..., 3])
        s, ss = a.double().sum(1), b.double().sum(1)
    else:
        unit = _unit_of(n, v, c, g, mode)
        s, ss = _usum(xs, unit, n * g), _usum(xs.double() ** 2, unit, n * g)
    m, rstd = gn_stats_from_sums(s, ss, L, f32(eps))
    return m.float(), rstd.float()


# ----------------------------------------------------------------------------------------------------------------
# GroupNormalization application
# ----------------------------------------------------------------------------------------------------------------
def _expand(t, unit):
    return t.reshape(-1)[unit]


def gn_apply_ref(x, gamma, beta, mean, rstd, g, mode, relu):
    """-> y (N, V, C) fp64, its bound, and the pre-activation (for the mask).  mean, rstd: the fp32 values the kernel is given."""
    n, v, c = x.shape
    unit = _unit_of(n, v, c, g, mode)
    _, idx = gn_index(v, c, g, mode)
    idx = idx.repeat(n)
    m, rs = _expand(mean.double(), unit), _expand(rstd.double(), unit)
    ga, be = gamma.double()[idx], beta.double()[idx]
    d = x.double().reshape(-1) - m
    y = d * rs * ga + be
    B = d.abs() * rs * ga.abs() + be.abs()
    out = torch.relu(y) if relu else y
    return out.reshape(x.shape), (K_EW * EPS32 * B + TINY).reshape(x.shape), y.reshape(x.shape)


def gn_apply_f32(x, gamma, beta, mean, rstd, g, mode, relu, fused):
    """fused: gn_apply_slab_stream_kernel's fma(x - m, rs * gamma, beta); else ((x - m) * rs * gamma) + beta"""
    n, v, c = x.shape
    unit = _unit_of(n, v, c, g, mode)
    _, idx = gn_index(v, c, g, mode)
    idx = idx.repeat(n)
    m, rs = _expand(mean.float(), unit), _expand(rstd.float(), unit)
    ga, be = gamma.float()[idx], beta.float()[idx]
    d = x.reshape(-1) - m
    y = fma32(d, rs * ga, be) if fused else d * rs * ga + be
    return (torch.relu(y) if relu else y).reshape(x.shape)


# ----------------------------------------------------------------------------------------------------------------
# GroupNormalization backward (groupnorm.hip:453-458)
# ----------------------------------------------------------------------------------------------------------------
def gn_bwd_ref(x, dy, gamma, beta, mean, rstd, g, mode, relu, old_dgamma=None, old_dbeta=None):
    """the documented formula in fp64 at the fp32 mean / rstd:
         xh = (x - mean) rstd, y = gamma xh + beta, dE = dy [y > 0];  A_j = sum dE xh, B_j = sum dE per (n, g, j);
         dgamma = sum_n A, dbeta = sum_n B;  c1 = sum_j gamma_j B_j / L, c2 = sum_j gamma_j A_j / L;  dx = (dE gamma - c1 - xh c2) rstd
    -> dict dx, dx_alt (the other branch at undecided elements), dgamma, dbeta, b_* absolute, undecided (bool, N V C)."""
    n, v, c = x.shape
    cg = c // g
    L = float(v * c // g)
    unit = _unit_of(n, v, c, g, mode)
    _, idx1 = gn_index(v, c, g, mode)
    idx = idx1.repeat(n)
    cls = (torch.arange(n)[:, None] * c + idx1[None, :]).reshape(-1)      # (n, affine index): the class sums' bins
    m, rs = _expand(mean.double(), unit), _expand(rstd.double(), unit)
    gad, bed = gamma.double(), beta.double()
    ga, be = gad[idx], bed[idx]
    xh = (x.double().reshape(-1) - m) * rs
    dyd = dy.double().reshape(-1)
    y = ga * xh + be
    if relu:
        on = (y > 0).double()
        und = y.abs() <= K_EW * EPS32 * ((ga * xh).abs() + be.abs())
    else:
        on = torch.ones_like(y)
        und = torch.zeros_like(y, dtype=torch.bool)
    de = dyd * on
    uw = und.double() * dyd.abs()

    def csum(t):
        return torch.zeros(n * c, dtype=F64).index_add_(0, cls, t).reshape(n, c)

    A, Bs = csum(de * xh), csum(de)
    absA, absB = csum((de * xh).abs()), csum(de.abs())
    uA, uB = csum(uw * xh.abs()), csum(uw)
    dgamma, dbeta = A.sum(0), Bs.sum(0)
    b_dgamma = K_RED * EPS32 * absA.sum(0) + EPS32 * dgamma.abs() + uA.sum(0) + TINY
    b_dbeta = EPS32 * dbeta.abs() + 1e-12 * absB.sum(0) + uB.sum(0) + TINY
    if old_dgamma is not None:
        b_dgamma = b_dgamma + EPS32 * (old_dgamma.double().abs() + dgamma.abs())
        dgamma = dgamma + old_dgamma.double()
    if old_dbeta is not None:
        b_dbeta = b_dbeta + EPS32 * (old_dbeta.double().abs() + dbeta.abs())
        dbeta = dbeta + old_dbeta.double()

    def gsum(t):      # (n, c) class values -> (n*g,) group sums; the affine index is g * cg + j in both modes
        return t.reshape(n, g, cg).sum(-1).reshape(-1)

    c1, c2 = gsum(gad * Bs) / L, gsum(gad * A) / L
    b_c1 = EPS32 * c1.abs() + 1e-12 * gsum(gad.abs() * absB) / L + gsum(gad.abs() * uB) / L
    b_c2 = K_RED * EPS32 * gsum(gad.abs() * absA) / L + EPS32 * c2.abs() + gsum(gad.abs() * uA) / L
    k1, k2 = c1[unit], c2[unit]
    dx = (de * ga - k1 - xh * k2) * rs
    dx_alt = torch.where(und, (dyd * (1.0 - on) * ga - k1 - xh * k2) * rs, dx)
    Bdx = ((de * ga).abs() + k1.abs() + (xh * k2).abs()) * rs
    b_dx = K_EW * EPS32 * Bdx + rs * (b_c1[unit] + xh.abs() * b_c2[unit]) + TINY
    sh = x.shape
    return dict(dx=dx.reshape(sh), dx_alt=dx_alt.reshape(sh), b_dx=b_dx.reshape(sh), dgamma=dgamma, b_dgamma=b_dgamma, dbeta=dbeta,
                b_dbeta=b_dbeta, undecided=und.reshape(sh), de=de.reshape(sh), c1=c1, c2=c2, b_c1=b_c1, b_c2=b_c2)


def gn_bwd_autograd(x, dy, gamma, beta, g, mode, relu):
    """autograd through R.group_norm in fp64 (its own fp64 statistics) -> dx (N, V, C), dgamma, dbeta.  x as (N, V, C)."""
    n, v, c = x.shape
    xd = x.double().reshape(n, v, 1, 1, c).requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = group_norm_oracle(xd, gd, bd, g, mode)
    if relu:
        y = torch.relu(y)
    y.backward(dy.double().reshape(n, v, 1, 1, c))
    return xd.grad.reshape(n, v, c), gd.grad, bd.grad


def group_norm_oracle(x5, gamma, beta, g, mode):
    """R.group_norm on an NDHWC tensor in either semantics (channels_first evaluated on NCDHW, returned as NDHWC)"""
    if mode == SLAB:
        return R.group_norm(x5, gamma, beta, g, -1)
    return R.group_norm(x5.permute(0, 4, 1, 2, 3), gamma, beta, g, 1).permute(0, 2, 3, 4, 1)


def gn_bwd_f32(x, dy, gamma, beta, mean, rstd, g, mode, relu, old_dgamma=None, old_dbeta=None, drop=None, c1_count=None):
    """the kernels' arithmetic: xh = (x - m) * rs, mask on xh * gamma + beta > 0 in fp32, fp32 products dE * xh added in fp64, one
    rounding (then the fp32 addition onto old); c1, c2 from the fp64 class sums, rounded once; dx in fp32 as written.
    drop: a flat element index left out of the sums; c1_count: a wrong divisor for c1 (both: the control)."""
    n, v, c = x.shape
    cg = c // g
    L = float(v * c // g)
    unit = _unit_of(n, v, c, g, mode)
    _, idx1 = gn_index(v, c, g, mode)
    idx = idx1.repeat(n)
    cls = (torch.arange(n)[:, None] * c + idx1[None, :]).reshape(-1)
    m, rs = _expand(mean.float(), unit), _expand(rstd.float(), unit)
    ga, be = gamma.float()[idx], beta.float()[idx]
    xh = (x.reshape(-1) - m) * rs
    de = dy.reshape(-1).clone()
    if relu:
        de = torch.where(xh * ga + be > 0, de, torch.zeros_like(de))
    keep = torch.ones_like(de)
    if drop is not None:
        keep[drop] = 0.0
    A = torch.zeros(n * c, dtype=F64).index_add_(0, cls, (de * xh * keep).double()).reshape(n, c)
    Bs = torch.zeros(n * c, dtype=F64).index_add_(0, cls, (de * keep).double()).reshape(n, c)
    dgamma, dbeta = A.sum(0).float(), Bs.sum(0).float()
    if old_dgamma is not None:
        dgamma = old_dgamma + dgamma
    if old_dbeta is not None:
        dbeta = old_dbeta + dbeta
    gad = gamma.double()
    c1 = ((gad * Bs).reshape(n, g, cg).sum(-1).reshape(-1) / (L if c1_count is None else c1_count)).float()
    c2 = ((gad * A).reshape(n, g, cg).sum(-1).reshape(-1) / L).float()
    dx = (de * ga - c1[unit] - xh * c2[unit]) * rs
    return dx.reshape(x.shape), dgamma, dbeta


def ratio_either(got, ref, alt, bound):
    """ratio() against whichever of ref / alt is nearer, element by element (alt == ref at decided elements)"""
    got = got.detach().double().cpu()
    err = torch.minimum((got - ref).abs(), (got - alt).abs())
    return ratio(err, torch.zeros_like(err), bound)


def check_either(got, ref, alt, bound, what):
    got = got.detach().double().cpu()
    assert not torch.isnan(got).any(), '%s: NaN in the result' % what
    r = ratio_either(got, ref, alt, bound)
    print('%-44s ratio %.3f of its bound' % (what, r))
    assert r <= 1.0, '%s: error is %.3f x its bound' % (what, r)
    return r


# ----------------------------------------------------------------------------------------------------------------
# the gate: SE-MLP, epilogue, backward (resnet.py:121-137; se.hip)
# ----------------------------------------------------------------------------------------------------------------
def gate_inputs(shape, seed=0, seams=False):
    """res, c2, dout (N, V, F); w1 (F, R), w2 (R, F), wsp (F) scaled so that the gates' arguments have deviation ~2 and stay below
    GATE_MAX_ARG; gamma, beta; sp_in, gap_in: independent inputs of the backward kernels (a sigmoid's values; a mean's).
    seams: the BACKWARD inputs dout / res carry M = 8 on every channel of the seam voxels (sp is then an independent input)."""
    n, dims, f, r, g = shape
    v = nvox(dims)
    gen = _gen(9500 + seed)
    res = torch.randn((n, v, f), generator=gen)
    c2 = 0.5 + 2.0 * torch.randn((n, v, f), generator=gen)
    dout = torch.randn((n, v, f), generator=gen)
    w1 = torch.randn((f, r), generator=gen) * (1.0 / math.sqrt(f))
    w2 = torch.randn((r, f), generator=gen) * (2.0 / math.sqrt(r))
    wsp = torch.randn(f, generator=gen) * (2.0 / math.sqrt(f))
    gamma = (0.5 + torch.rand(f, generator=gen)) * torch.where(torch.rand(f, generator=gen) < 0.5, -1.0, 1.0)
    beta = 0.2 * torch.randn(f, generator=gen)
    sp_in = torch.sigmoid(2.0 * torch.randn((n, v), generator=gen))
    gap_in = torch.randn((n, f), generator=gen)
    p = dict(res=res, c2=c2, dout=dout, w1=w1, w2=w2, wsp=wsp, gamma=gamma, beta=beta, sp_in=sp_in, gap_in=gap_in)
    if seams:
        sv = se_seams(n, v, f) if seams == 'gate' else blk_seams(n, v, f, g)
        p['res'] = res.clone()
        p['res'].view(n * v, f)[sv] = 8.0
        p['dout'].view(n * v, f)[sv] = 8.0
        p['seam_voxels'] = sv
        if seams == 'blk':      # the GroupNorm side of the fused pass: c2 on the positive side of the ReLU at the seam voxels
            _, idx = gn_index(v, f, g, SLAB)
            sgn = torch.sign(gamma[idx]).reshape(v, f)
            c2.view(n * v, f)[sv] = 0.5 + 8.0 * sgn[sv % v]
    return p


def se_mlp_ref(gap, w1, w2):
    """-> h (N, R), ch (N, F) fp64 and absolute bounds: h = relu(gap W1): K_DOT eps32 |gap| |W1|; ch = sigmoid(h W2):
    lowp_ref.sigmoid_bound with da = K_DOT eps32 |h| |W2| + bound(h) |W2| (what h carries, once)"""
    gd, w1d, w2d = gap.double(), w1.double(), w2.double()
    h = torch.relu(gd @ w1d)
    b_h = K_DOT * EPS32 * (gd.abs() @ w1d.abs()) + TINY
    z = h @ w2d
    dz = K_DOT * EPS32 * (h.abs() @ w2d.abs()) + b_h @ w2d.abs()
    return h, b_h, torch.sigmoid(z), LP.sigmoid_bound(z, dz)


def sigmoid_f32(a):
    one = torch.tensor(1.0, dtype=F32)
    return one / (one + torch.exp(-a))


def se_mlp_f32(gap, w1, w2):
    """se.hip:123-160: 256 / R slices each run an fma chain over every (256 / R)-th input, the slices are added in order; ReLU; an
    fma chain over the R hidden units; 1 / (1 + expf(-z))"""
    n, f = gap.shape
    r = w1.shape[1]
    P = 256 // r
    part = torch.zeros((P, n, r), dtype=F32)
    for sl in range(min(P, f)):
        s = torch.zeros((n, r), dtype=F32)
        for cc in range(sl, f, P):
            s = fma32(gap[:, cc:cc + 1], w1[cc:cc + 1, :], s)
        part[sl] = s
    t = torch.zeros((n, r), dtype=F32)
    for sl in range(P):
        t = t + part[sl]
    h = torch.relu(t)
    z = torch.zeros((n, f), dtype=F32)
    for k in range(r):
        z = fma32(h[:, k:k + 1], w2[k:k + 1, :], z)
    return h, sigmoid_f32(z)


def _lane_dot_f32(a, b):
    """sum over the last axis as the gate kernels do: per lane (p0 + p1) + (p2 + p3) of the four fp32 products, then the xor butterfly
    over the F/4 lanes (offsets F/8 .. 1; every lane ends with the same value: fp32 addition commutes)"""
    p = (a * b).reshape(a.shape[:-1] + (a.shape[-1] // 4, 4))
    acc = (p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])
    while acc.shape[-1] > 1:
        h = acc.shape[-1] // 2
        acc = acc[..., :h] + acc[..., h:]
    return acc[..., 0]


def epilogue_ref(res, c2, wsp, ch, gamma, beta, mean, rstd, g, mode):
    """-> sp (N, V), b_sp, out (N, V, F), b_out (absolute).  c2 None: the gate alone.  ch, mean, rstd: the fp32 inputs."""
    rd, wd = res.double(), wsp.double()
    dot = (rd * wd).sum(-1)
    sp = torch.sigmoid(dot)
    b_sp = LP.sigmoid_bound(dot, K_DOT * EPS32 * (rd.abs() * wd.abs()).sum(-1))
    chd = ch.double()[:, None, :]
    out = rd * (sp[..., None] + chd)
    B = rd.abs() * (sp[..., None] + chd.abs())
    if c2 is not None:
        t, bt, _ = gn_apply_ref(c2, gamma, beta, mean, rstd, g, mode, True)
        out = out + t
        B = B + (bt - TINY) / (K_EW * EPS32)
    return sp, b_sp, out, K_EW * EPS32 * B + rd.abs() * b_sp[..., None] + TINY


def epilogue_f32(res, c2, wsp, ch, gamma, beta, mean, rstd, g, mode):
    sp = sigmoid_f32(_lane_dot_f32(res, wsp.expand_as(res)))
    out = res * (sp[..., None] + ch[:, None, :])
    if c2 is not None:
        out = out + gn_apply_f32(c2, gamma, beta, mean, rstd, g, mode, True, False)
    return sp, out


def se_bwd_ref(dout, res, sp, gap, h, ch, w1, w2, wsp, old=None):
    """SURVEY Appendix A' "ResnetBlock gate" in fp64 at the fp32 sp, gap, h, ch the kernel is given:
         g = dout res;  t_v = sum_c g;  ds_v = t_v sp_v (1 - sp_v);  Pch[n][c] = sum_v g;  dz2 = Pch ch (1 - ch);
         dz1 = [h > 0] dz2 W2^T;  dW2 = h^T dz2;  dW1 = gap^T dz1;  dgap = dz1 W1^T / V;  dwsp = sum_{n,v} ds res;
         dres = dout (sp + ch) + ds wsp + dgap
    old: dict of the destinations' contents (dw1, dw2, dwsp) when the call accumulates.  -> dict of values and absolute b_*."""
    n, v, f = res.shape
    d, r = dout.double(), res.double()
    s, chd, hd, gd = sp.double(), ch.double(), h.double(), gap.double()
    w1d, w2d, wd = w1.double(), w2.double(), wsp.double()
    gg = d * r
    t, Bt = gg.sum(-1), gg.abs().sum(-1)
    ds = t * s * (1.0 - s)
    b_ds = K_DOT * EPS32 * Bt * s * (1.0 - s) + TINY
    Pch, eP = gg.sum(1), K_RED * EPS32 * gg.abs().sum(1)
    sg = chd * (1.0 - chd)
    dz2, e2 = Pch * sg, eP * sg
    hon = (hd > 0).double()
    dz1, e1 = hon * (dz2 @ w2d.t()), hon * (e2 @ w2d.abs().t())
    o = {}
    o['dw2'] = hd.t() @ dz2
    o['b_dw2'] = hd.abs().t() @ e2 + EPS32 * o['dw2'].abs() + TINY
    o['dw1'] = gd.t() @ dz1
    o['b_dw1'] = gd.abs().t() @ e1 + EPS32 * o['dw1'].abs() + TINY
    o['dgap'] = (dz1 @ w1d.t()) / v
    o['b_dgap'] = (e1 @ w1d.abs().t()) / v + EPS32 * o['dgap'].abs() + TINY
    dsr = ds[..., None] * r
    o['dwsp'] = dsr.sum((0, 1))
    o['b_dwsp'] = K_RED * EPS32 * dsr.abs().sum((0, 1)) + (b_ds[..., None] * r.abs()).sum((0, 1)) + EPS32 * o['dwsp'].abs() + TINY
    o['ds'], o['b_ds'] = ds, b_ds
    spc = s[..., None] + chd[:, None, :]
    o['dres'] = d * spc + ds[..., None] * wd + o['dgap'][:, None, :]
    B = d.abs() * spc + (ds[..., None] * wd).abs() + o['dgap'].abs()[:, None, :]
    o['b_dres'] = K_EW * EPS32 * B + wd.abs() * b_ds[..., None] + o['b_dgap'][:, None, :] + TINY
    if old is not None:
        for k in ('dw1', 'dw2', 'dwsp'):
            o['b_' + k] = o['b_' + k] + EPS32 * (old[k].double().abs() + o[k].abs())
            o[k] = o[k] + old[k].double()
    return o


def se_bwd_f32(dout, res, sp, gap, h, ch, w1, w2, wsp, old=None):
    """se.hip:230-425: the per-voxel dot product as _lane_dot_f32, ds = (t * s) * (1 - s), the products dout * res and ds * res
    rounded to fp32 and added in fp64, the SE-MLP backward in fp64, one rounding per output; dres in fp32 left to right"""
    n, v, f = res.shape
    one = torch.tensor(1.0, dtype=F32)
    t = _lane_dot_f32(dout, res)
    ds = t * sp * (one - sp)
    Pch = (dout * res).double().sum(1)
    Pw = (ds[..., None] * res).double().sum((0, 1))
    chd, hd = ch.double(), h.double()
    dz2 = Pch * chd * (1.0 - chd)
    dz1 = (hd > 0).double() * (dz2 @ w2.double().t())
    o = dict(ds=ds, dw2=(hd.t() @ dz2).float(), dw1=(gap.double().t() @ dz1).float(), dwsp=Pw.float(),
             dgap=((dz1 @ w1.double().t()) * (1.0 / v)).float())
    if old is not None:
        for k in ('dw1', 'dw2', 'dwsp'):
            o[k] = old[k] + o[k]
    o['dres'] = dout * (sp[..., None] + ch[:, None, :]) + ds[..., None] * wsp + o['dgap'][:, None, :]
    return o


GATE_OUTPUTS = ('ds', 'dgap', 'dw1', 'dw2', 'dwsp', 'dres')
