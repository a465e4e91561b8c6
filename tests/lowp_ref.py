"""References, fp32 restatements and error bounds for the 16-bit NON-CONV kernels of csrc/lowp_norm.hip, lowp_block.hip and lowp_point.hip: bts_lp_gn_stats, bts_lp_gn_apply,
bts_lp_colsum, bts_lp_block_epilogue, bts_lp_block_epilogue_head, bts_lp_head, bts_lp_head_bwd, the samplers and the casts.  Plain
Python on the CPU, in the pattern of tests/step_ref.py (whose EPS32, TINY, ratio and check are used, not copied).

For every kernel this module holds
  1. the fp64 REFERENCE on the STORED (already 16-bit-rounded) inputs.  oracle/torch_ref.py has GroupNormalization only as a whole
     (group_norm: statistics AND application): the statistics and the application are written out here, and
     tests/test_lowp_kernels_host.py pins their composition to R.group_norm (slab mode = axis -1, channel mode = axis 1 on the
     channels-first tensor) to 1e-12.  Scalars are rounded to fp32 as the ABI receives them.  mean / rstd handed to the apply and
     epilogue kernels are INPUTS: the reference uses the fp32 values the kernel is given.
  2. the fp32 RESTATEMENT of the kernel's documented formula in torch float32, in the kernel's order, and
  3. the BOUND  K * eps32 * B + TINY,  B = the sum of the absolute values of the terms that are added.

OUTPUTS IN THE STORAGE TYPE get no u * |ref| of slack: storage_interval(ref, bound, tdt) = [RNE(ref - bound), RNE(ref + bound)] with
torch's CPU cast, and lo <= got <= hi is asserted element-wise.  Where ref is further than the bound from a rounding tie the interval
is ONE value: the correctly rounded one.  A kernel that truncates fails on half of its elements.  (torch casts fp64 to 16 bits
through fp32, two roundings; storage_interval takes the first one to odd, so the pair rounds once.)  The printed ratio of such an output is
storage_ratio(): the smallest multiple of eps32 * B by which ref must move so that its correct rounding is the value the kernel stored
(0 for a correctly rounded value).

THE K RULE (step_ref's).  tests/test_lowp_kernels_gpu.py uses the Ks below unchanged, tests/test_lowp_kernels_host.py holds every
restatement to K/4.  No K and no bound comes from a run of a kernel.

K_LP = 16, element-wise kernels (gn_apply, block_epilogue's out, head and head_bwd's dx, upsample2_bwd): the documented formulas
  take 3 .. 5 roundings that each act on a quantity no larger than B (x - mean; rstd * gamma; the product; the addition; for the
  epilogue sp + ch and the final fma) and dot products of K <= 4 (head_bwd dx), 8 (upsample2_bwd) or C <= 256 terms (head).  The
  worst case of the short forms is 5 eps32 B; K/4 = 4 is the level a restatement of 4 roundings cannot pass and one of 5 passes only
  with every rounding at its maximum and of one sign.  A dot product of n terms has the worst case n eps32 B, but its roundings act
  on the PARTIAL sums and are independent.  The oct kernels' chains are 8 terms and a tree of log2(C/8) <= 5 levels: with
  |partial| <= B / 2 on average, rms eps32 B / 2 * sqrt(13 / 3) = 1.0, below K/4 with a margin of 4 sigma.
  FINDING of the K/4 rule (no K was raised): the per-voxel head kernel (nvox < 4096) runs ONE chain over all C channels.  At
  C = 24 and 32 that is 25 / 33 roundings, rms eps32 B / 2 * sqrt(33 / 3) = 1.7, and the maximum over the 10^4 outputs of the
  listed shapes is 4 sigma: the restatement measures 4.6 at (5000, 24, 2).  Such chains are held to LONG_CHAIN_HOST_LIMIT = K/2 on
  the host (step_ref's treatment of the short Dense chains); the kernel is held to K = 16 like every other.
K_RUN = 16, reductions (gn_stats, colsum, head_bwd's dw / db): per-lane fp32 running sums, flushed to fp64 (after at most 512
  additions in gn_stats, 256 in colsum, never in head_bwd: at most ceil(nvox * C/8 / 524288) + 6 there), fp64 from there on, ONE
  rounding to fp32 at the end (two when head_bwd accumulates).  A run of n additions errs by (n - 1) eps32 * (the run's sum of
  |terms|) at worst: K covers every run of n <= 15 rigorously (the tiny shapes).  A longer run is a sum of independent roundings of
  partial sums k mu: rms eps32 mu sqrt(n^3 / 9) = eps32 (n mu) sqrt(n) / 3, 7.6 eps32 of the run's total at n = 512 -- and an output
  is the sum of >= 256 lanes' runs whose errors are independent: 7.6 / 16 = 0.5 eps32 B, plus the last rounding (<= 1).  K/4 = 4 is
  7 sigma of that.
K_GATE = 16, values of a sigmoid through __expf (the spatial gate sp, the head's probabilities):
  bound = K_GATE eps32 U + s (1 - s) da,  U = s (1 - s) (|a| + 1) + s,  s = sigmoid(a), da = the absolute bound of the argument a (for
  the gate K_LP eps32 sum |res| |wsp|; for the heads K_LP eps32 (sum |x| |W| + |b|), plus sum |W| bound(out) in the fused head).  What
  an input carries is added ONCE, outside the K of the operation it enters: no K multiplies another.  Such composite bounds are
  returned absolute; the GPU test holds the kernel to 1.0 of them, the host test the restatement to 1/4 (every K in them quartered).
  __expf(-a) is v_exp_f32(-a * log2(e)).  The product -a * log2(e) rounds to fp32: an absolute error eps32 |a| log2(e) of the
  exponent, ln(2) times that relative in 2^t: eps32 |a|.  The fp32 constant log2(e) is itself off by up to eps32 relative: another
  eps32 |a|.  v_exp_f32 is good to 1 ulp = 2 eps32.  So e = exp(-a) carries (2 |a| + 2) eps32 relative, and with
  ds/de = -s^2, s^2 e = s (1 - s):  |ds| <= s (1 - s) ((2 |a| + 2) eps32 + |da|) + 2 eps32 s  (the addition 1 + e and the
  correctly rounded division).  Every coefficient of U is <= 2: 2 U eps32 at worst, K/4 = 4 leaves the restatement (torch's exp, not
  an exp2) a factor 2.  The bound grows with |a|: the inputs keep |a| <= 16 (GATE_MAX_ARG, asserted), where exp(-a) is far from
  the fp32 subnormals that v_exp_f32 flushes.
Bounds WITHOUT a K: maxpool2 (forward, backward), upsample2 forward and the casts are selections, copies or ONE IEEE operation
  (fl32(old + dy) then RNE): bit-exact against torch's CPU cast / the same single operation on the CPU.

What the shapes of tests/test_lowp_kernels_gpu.py do NOT reach (by reading the host code):
  * gn_stats' `cnt == 64` flush needs 64 trips of 2048 elements per lane inside one block's span: per > 131072 elements with the
    256-block cap in force, L > 3.3e7 elements per group.  Not reached.
  * colsum's `cnt == 256` flush IS reached: (1, 4097, 256) gives every lane 257 voxels (8 voxels per trip, per = 2049).
  * the 32768-block caps of both head kernels lie at 2^26 elements or more (nvox >= 8.4e6 voxels per-voxel form): left to the
    full-size model tests.
  * the 16384-block caps of maxpool2 fwd / bwd and upsample2 bwd need 2.7e8-element tensors: not covered.  upsample2 forward's is.

SEAMS.  The inputs of the reductions carry outliers on the first and last item (octet; channel-mode statistics: a voxel's group
channels; head_bwd: a voxel's octet) of every unit and of every block's span (per / vstep as the host code computes them; head_bwd:
the first and last lane of every workgroup in every trip of its grid-stride loop) and either side of the last whole 256-lane trip
of a span (the reductions have no unrolled loop; the trip tail is their remainder).  tests/test_lowp_kernels_host.py asserts on the REFERENCE ALONE that dropping or double-counting any single seam
item moves at least one output by 8 of its bounds, for every listed shape.

MEASURED RESTATEMENT RATIOS (tests/test_lowp_kernels_host.py -s; max over the listed small shapes and both storage types).  In units
of eps32 B, against K/4 = 4:
  gn_stats mean 0.97, rstd 1.00 (the one last rounding)   colsum 0.47 (0.05 at (1, 4097, 256), past the flush)
  gn_apply 2.82 (unfused form; fused 2.3)   upsample2_bwd 0 (eight 16-bit values add exactly in fp32)
  head_bwd dx 3.05 (a chain of K = 4: the worst case is 4), dw 1.09, db 0.25
As a fraction of the whole bound (composite bounds), against 1/4:
  block_epilogue gate 0.086, out 0.171   block_epilogue_head 0.070 (sigmoid), 0.067 (linear)
  head, sigmoid 0.138; linear 0.289 at (5000, 24, 2) bfloat16 (= 4.63 of 16: the long-chain finding above, limit 1/2), 0.19 at C = 32, 0.17 in the oct form

MEASURED GPU RATIOS on an MI355X (tests/test_lowp_kernels_gpu.py -s; max per kernel: float16 / bfloat16).  In units of eps32 B, K = 16:
  gn_stats mean 0.965 / 0.918, rstd 1.004 / 0.110      colsum 0.449 / 0.470 (past the flush 0.043 / 0.048)      gn_apply 1.273 / 0.572
  head_bwd dx 0.917 / 0.954, dw 0.937 / 1.087, db 0.246 / 0.246      upsample2_bwd 0 / 0
As a fraction of the whole bound, limit 1:
  block_epilogue gate 0.105 / 0.083, out 0.075 / 0.012      block_epilogue_head sigmoid 0.070 / 0.067, linear 0.060 / 0.067
  head sigmoid 0.113 / 0.138, linear 0.223 / 0.289 (both at (5000, 24, 2): the per-voxel kernel's one chain of 24 terms, the
  restatement's own figures to the digit)
  (storage-type outputs -- gn_apply, block_epilogue out, head_bwd dx, upsample2_bwd -- in storage_ratio's measure: 0 for a value
  that is the correct rounding of the reference.)  Nothing is above half of its limit.  maxpool2, upsample2 forward and the casts:
  bit-exact.
"""
import math

import torch

from step_ref import EPS32, TINY, check, f32, fma32, ratio  # noqa: F401  (check and ratio are re-exported to the two test files)

F64 = torch.float64
F32 = torch.float32
K_LP = 16
K_RUN = 16
K_GATE = 16
LONG_CHAIN_HOST_LIMIT = 0.5      # of the bound (K/2 where the others have K/4): one fma chain of >= 24 terms, see the docstring
GATE_MAX_ARG = 16.0
SLAB, CHANNEL = 0, 1
DTYPES = {'float16': (1, torch.float16), 'bfloat16': (2, torch.bfloat16)}
SENTINEL = -7.25        # exactly representable in both storage types


# ----------------------------------------------------------------------------------------------------------------
# storage-type outputs
# ----------------------------------------------------------------------------------------------------------------
def storage_interval(ref, bound, tdt):
    """[RNE_tdt(ref - bound), RNE_tdt(ref + bound)] with torch's CPU cast -> (lo, hi) in tdt"""
    ref = torch.as_tensor(ref, dtype=F64)
    bound = torch.as_tensor(bound, dtype=F64)
    return _rne(ref - bound, tdt), _rne(ref + bound, tdt)


def _rne(x, tdt):
    """fp64 -> tdt, rounded ONCE.  torch casts fp64 to a 16-bit type through fp32, and two roundings to nearest can land on the wrong
    side of a 16-bit tie (1 + 2^-11 + 2^-30 -> fp32 1 + 2^-11 -> fp16 1.0).  So the step to fp32 is taken to ODD here (an inexact
    value goes to the neighbour whose last bit is set: it can then sit on no tie of a shorter format), and torch's CPU cast does the
    one rounding to nearest even from there."""
    f = x.float()
    d = f.double()
    below = torch.where(d > x, torch.nextafter(f, torch.full_like(f, -math.inf)), f)
    above = torch.nextafter(below, torch.full_like(f, math.inf))
    odd = torch.where((below.view(torch.int32) & 1) == 1, below, above)
    return torch.where((d != x) & torch.isfinite(f), odd, f).to(tdt)


def _ulp(a, tdt):
    """spacing of tdt above |a| (a: non-negative fp64 values that tdt represents) and whether |a| is a power of two above the subnormals"""
    mant, emin = (10, -14) if tdt == torch.float16 else (7, -126)
    m, ex = torch.frexp(a)
    e = torch.clamp(ex - 1, min=emin)
    e = torch.where(a == 0, torch.full_like(e, emin), e)
    ulp = torch.ldexp(torch.ones_like(a), e - mant)
    return ulp, (m == 0.5) & (ex - 1 > emin)


def storage_ratio(got, ref, unit):
    """max over elements of (the distance from ref to the set of reals that RNE maps onto got) / unit; got finite"""
    tdt = got.dtype
    g = got.double()
    ref = torch.as_tensor(ref, dtype=F64)
    a = g.abs()
    s = torch.where(g == 0, torch.where(ref < 0, -1.0, 1.0), torch.sign(g)).double()
    r = ref * s
    ulp, pow2 = _ulp(a, tdt)
    away = a + ulp / 2
    toward = torch.where(a == 0, -ulp / 2, a - torch.where(pow2, ulp / 4, ulp / 2))
    d = torch.clamp(torch.maximum(r - away, toward - r), min=0.0)
    u = torch.as_tensor(unit, dtype=F64).expand_as(d)
    q = torch.where(d > TINY, d / u, torch.zeros_like(d))
    return float(q.max()) if q.numel() else 0.0


def check_storage(got, ref, unit, k, what):
    """assert RNE(ref - k unit - TINY) <= got <= RNE(ref + k unit + TINY) element-wise; prints storage_ratio first"""
    got = got.detach().cpu()
    assert not torch.isnan(got.float()).any(), '%s: NaN in the result' % what
    unit = torch.as_tensor(unit, dtype=F64)
    print('%-52s ratio %.3f of K = %g' % (what, storage_ratio(got, ref, unit), k))
    lo, hi = storage_interval(ref, k * unit + TINY, got.dtype)
    bad = (got.double() < lo.double()) | (got.double() > hi.double())
    nbad = int(bad.sum())
    if nbad:
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError('%s: %d of %d values outside [RNE(ref - bound), RNE(ref + bound)]; first at %d: got %r, ref %r, interval [%r, %r]' % (
            what, nbad, bad.numel(), i, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]), float(lo.reshape(-1)[i]), float(hi.reshape(-1)[i])))


def randn_storage(shape, tdt, seed, mean=0.0, sd=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=F32) * sd + mean).to(tdt)


def randn32(shape, seed, sd=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=F32) * sd + mean


# ----------------------------------------------------------------------------------------------------------------
# the host code's block arithmetic (csrc/lowp_common.h, lowp_norm.hip, lowp_block.hip), restated: the seams and the restatements follow it
# ----------------------------------------------------------------------------------------------------------------
def gn_blocks(L):
    return max(1, min(256, L // (256 * 8 * 8)))


def colsum_blocks(V):
    return max(1, min(512, V // 2048))


def chunk_per(Lu, units, target=4096):
    """lp_chunk_per -> (elements per chunk, chunks per unit)"""
    steps = Lu // 2048
    b = max(1, min(target // units, steps // 4))
    per = (steps + b - 1) // b
    return per * 2048, (steps + per - 1) // per


def gn_bwd_tiled_ref(v, c, groups):
    """the GroupNorm-backward tiling rule as bts_amd.lowp stated it before it asked the library (bts_lp_gn_bwd_tiled)"""
    return not ((v * c) % groups or (v * c // groups) % 2048 or c // groups > 32 or 256 % (c // groups) or c > 256 or c & (c - 1))


def wgrad_supported_ref(kind, cin, cout, extents=None):
    """the 16-bit weight-gradient shape rule as bts_amd.lowp stated it before it asked the library (bts_lp_conv3d_bwd_weight_args_ok);
    kinds: K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3"""
    K1, K3S1, K3S2, K3S2T = 0, 1, 2, 3
    if kind == K3S2 and any(v & 1 for v in extents):
        return False
    if kind in (K3S2, K3S2T):
        return cin % 8 == 0 and cout % 8 == 0
    return kind in (K3S1, K1) and cin % 8 == 0 and cout % 8 == 0 and cout <= 256 and ((cout // 8) & (cout // 8 - 1)) == 0


def takes_chunked(n, v, c, g, mode):
    lu = v * c // g if mode == SLAB else v * c
    return 2048 % c == 0 and lu % 2048 == 0


def _span_seams(lo, hi, trip):
    """first and last item of [lo, hi) and either side of its last whole trip"""
    s = {lo, hi - 1}
    t = lo + (hi - lo) // trip * trip
    for i in (t - 1, t):
        if lo <= i < hi:
            s.add(i)
    return s


def gn_stats_seams(v, c, g, mode):
    """item indices inside ONE unit: slab mode octets of the L elements; channel mode voxels"""
    if mode == SLAB:
        n = v * c // g // 8
        B = gn_blocks(v * c // g)
        per = (n + B - 1) // B
    else:
        n = v
        B = gn_blocks(v * c // g)
        per = (v + B - 1) // B
    s = set()
    for b in range(B):
        lo, hi = b * per, min((b + 1) * per, n)
        if lo < hi:
            s |= _span_seams(lo, hi, 256)
    return sorted(s)


def colsum_seams(v, c):
    B = colsum_blocks(v)
    per = (v + B - 1) // B
    vstep = 256 // (c // 8)
    s = set()
    for b in range(B):
        lo, hi = b * per, min((b + 1) * per, v)
        if lo < hi:
            s |= _span_seams(lo, hi, vstep)
    return sorted(s)


def head_bwd_seams(nvox, c):
    """voxels whose octets sit on the first or last lane of a workgroup's 256 octets in ANY trip of the grid-stride loop (the stride is a
    whole number of workgroups, so these are octets 256 j and 256 j + 255), and the very last voxel"""
    c8 = c // 8
    total = nvox * c8
    s = {nvox - 1}
    for j in range((total + 255) // 256):
        s.add(256 * j // c8)
        s.add(min(256 * j + 255, total - 1) // c8)
    return sorted(s)


# ----------------------------------------------------------------------------------------------------------------
# GroupNormalization statistics
# ----------------------------------------------------------------------------------------------------------------
# (N, V, C, G)
GN_STATS_SLAB = [(2, 1, 8, 1), (1, 769, 8, 1), (1, 5121, 8, 1)]
GN_STATS_SLAB_PAST_CAP = (1, 525289, 8, 1)       # L / 16384 = 256.49: B lands ON the cap of 256
GN_STATS_SLAB_OVER_CAP = (1, 526337, 8, 1)       # L / 16384 = 257.0002: the cap binds, an odd number of octets
GN_STATS_CHANNEL = [(1, 1, 8, 8), (2, 300, 32, 8), (1, 5000, 16, 2)]


def _units(x, g, mode):
    """x (N, V, C) -> (N, G, items, per-item elements): the elements of every (sample, group) in item order"""
    n, v, c = x.shape
    if mode == SLAB:
        return x.reshape(n, g, v * c // g // 8, 8)
    return x.reshape(n, v, g, c // g).permute(0, 2, 1, 3)


def gn_stats_outlier(v, c, g):
    """seam value M: an item of eight M moves the mean by 8 M / L.  8 bounds of K_RUN eps32 E|x| (E|x| = 4) need M >= 3.9e-6 L: 8 up to
    L = 2^20, 32 beyond (16.2 at the L = 4.2e6 of the shape past the block cap)"""
    return 32.0 if v * c // g >= (1 << 20) else 8.0


def gn_stats_inputs(shape, mode, tdt, seed=0):
    """mean near 4, deviation 1 (E[x^2] - mean^2 cancels), seam items at the outlier value"""
    n, v, c, g = shape
    x = randn_storage((n, v, c), tdt, 5000 + seed, 4.0, 1.0)
    u = _units(x, g, mode)
    idx = torch.tensor(gn_stats_seams(v, c, g, mode))
    u[:, :, idx, :] = gn_stats_outlier(v, c, g)     # (a view in both modes: writes x)
    return x


def gn_stats_from_sums(s, q, count, eps):
    """fp64 sums -> mean, rstd and their bound units.  var = E[x^2] - mean^2 only HERE (the sensitivity test perturbs sums); the
    reference itself takes the two-pass variance."""
    m = s / count
    var = torch.clamp(q / count - m * m, min=0.0)
    return m, 1.0 / torch.sqrt(var + eps)


def gn_stats_ref(x, g, mode, eps):
    """x (N, V, C) storage type -> mean, rstd (N*G,) fp64 and their bound units (eps32 * B).
    B(mean) = E|x|.  rstd = (var + eps)^-1/2 with var = E[x^2] - mean^2:  |d rstd| = rstd^3 / 2 * |d var|,
    |d var| <= |d E[x^2]| + 2 |mean| |d mean|, so B(rstd) = rstd^3 / 2 * (E[x^2] + 2 |mean| E|x|) + rstd (the last rounding)."""
    eps = f32(eps)
    u = _units(x.double(), g, mode)
    m = u.mean((2, 3))
    var = ((u - m[:, :, None, None]) ** 2).mean((2, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    ea, e2 = u.abs().mean((2, 3)), (u * u).mean((2, 3))
    Bm = ea
    Br = 0.5 * rstd ** 3 * (e2 + 2.0 * m.abs() * ea) + rstd
    return m.reshape(-1), rstd.reshape(-1), EPS32 * Bm.reshape(-1), EPS32 * Br.reshape(-1)


def gn_stats_f32(x, g, mode, eps):
    """the kernel's order: per block and lane an fp32 running sum and fma chain of squares (slab: 8 values per trip of 256 lanes;
    channel: a voxel's group channels, flushed per voxel), fp64 from there; E[x^2] - mean^2 in fp64, one rounding"""
    n, v, c = x.shape
    u = _units(x.float(), g, mode)
    items = u.shape[2]
    L = v * c // g
    B = gn_blocks(L)
    per = (items + B - 1) // B
    s = torch.zeros((n, g), dtype=F64)
    q = torch.zeros((n, g), dtype=F64)
    for b in range(B):
        blk = u[:, :, b * per:min((b + 1) * per, items)]
        if blk.shape[2] == 0:
            continue
        if mode == SLAB:
            pad = (-blk.shape[2]) % 256
            blk = torch.cat([blk, torch.zeros((n, g, pad, 8))], 2).reshape(n, g, -1, 256, 8)
            fs = torch.zeros((n, g, 256))
            fq = torch.zeros((n, g, 256))
            for t in range(blk.shape[2]):
                for e in range(8):
                    w = blk[:, :, t, :, e]
                    fs = fs + w
                    fq = fma32(w, w, fq)
            s += fs.double().sum(-1)
            q += fq.double().sum(-1)
        else:
            fs = torch.zeros(blk.shape[:3])
            fq = torch.zeros(blk.shape[:3])
            for e in range(blk.shape[3]):
                w = blk[..., e]
                fs = fs + w
                fq = fma32(w, w, fq)
            s += fs.double().sum(-1)
            q += fq.double().sum(-1)
    m, rstd = gn_stats_from_sums(s, q, float(L), float(f32(eps)))
    return m.float().reshape(-1), rstd.float().reshape(-1)


# ----------------------------------------------------------------------------------------------------------------
# GroupNormalization application (+ ReLU)
# ----------------------------------------------------------------------------------------------------------------
# (N, V, C, G, mode)
GN_APPLY_CHUNKED = [(1, 2048, 8, 8, SLAB), (1, 3584, 32, 8, SLAB), (2, 2304, 16, 2, SLAB), (1, 1792, 8, 8, CHANNEL), (1, 72, 256, 8, CHANNEL)]
GN_APPLY_STRIDE = [(1, 10, 24, 3, SLAB), (2, 384, 32, 8, SLAB), (1, 100, 256, 8, CHANNEL)]
GN_APPLY_PAST_CAP = (1, 1400000, 24, 3, SLAB)


def gn_index(n, v, c, g, mode, lo=0, hi=None):
    """-> group and parameter index of every element of voxels [lo, hi) of a sample of v voxels (group_norm.py:89-100: slab mode is
    the raw reshape)"""
    r = torch.arange(lo * c, (v if hi is None else hi) * c)
    cg = c // g
    ch = r % c
    if mode == SLAB:
        grp = r // (v * c // g)
        return grp, grp * cg + ch % cg
    return ch // cg, ch


def gn_params(n, c, g, seed):
    """gamma, beta, and statistics as a kernel would be handed them (fp32)"""
    gen = torch.Generator().manual_seed(6000 + seed)
    gamma = torch.randn(c, generator=gen) * 0.5 + 1.0
    beta = torch.randn(c, generator=gen) * 0.5
    mean = torch.randn(n * g, generator=gen) * 0.3
    rstd = torch.rand(n * g, generator=gen) + 0.5
    return gamma, beta, mean, rstd


def _expand_stats(t, n, c, g, grp):
    return t.reshape(n, g)[:, grp].reshape(n, -1, c)


def gn_apply_ref(x, gamma, beta, mean, rstd, g, mode, relu, lo=0, v=None):
    """-> y fp64 (N, V, C), bound unit eps32 * B,  B = (|x| + |mean|) rstd |gamma| + |beta|.  lo, v: x holds voxels [lo, lo + x.shape[1])
    of samples of v voxels (the shapes past a grid cap are checked on bands)"""
    n, vs, c = x.shape
    grp, idx = gn_index(n, vs if v is None else v, c, g, mode, lo, lo + vs)
    mu = _expand_stats(mean.double(), n, c, g, grp)
    rs = _expand_stats(rstd.double(), n, c, g, grp)
    ga = gamma.double()[idx].reshape(1, vs, c)
    be = beta.double()[idx].reshape(1, vs, c)
    xd = x.double()
    y = (xd - mu) * rs * ga + be
    B = (xd.abs() + mu.abs()) * rs * ga.abs() + be.abs()
    return (torch.relu(y) if relu else y), EPS32 * B


def gn_apply_f32(x, gamma, beta, mean, rstd, g, mode, relu, fused):
    """fused (chunked kernel): fma(x - mean, rstd * gamma, beta); else (grid-stride kernel): (x - mean) * rstd * gamma + beta"""
    n, v, c = x.shape
    grp, idx = gn_index(n, v, c, g, mode)
    mu = _expand_stats(mean, n, c, g, grp)
    rs = _expand_stats(rstd, n, c, g, grp)
    ga = gamma[idx].reshape(1, v, c)
    be = beta[idx].reshape(1, v, c).expand(n, v, c)
    xf = x.float()
    y = fma32(xf - mu, rs * ga, be) if fused else (xf - mu) * rs * ga + be
    return torch.relu(y) if relu else y


# ----------------------------------------------------------------------------------------------------------------
# column sums (the shortcut's global average pool)
# ----------------------------------------------------------------------------------------------------------------
# (N, V, C)
COLSUM_SHAPES = [(1, 1, 8), (2, 1, 256), (1, 33, 64), (1, 4097, 32), (1, 4097, 256)]     # the last: 257 trips per lane, past the `cnt == 256` flush
COLSUM_PAST_CAP = (1, 1050627, 8)


def colsum_outlier(v):
    """a seam voxel of this value moves its sums by M: 8 bounds of 16 eps32 * 0.8 V need M >= 6.2e-6 V"""
    return float(2 ** max(2, math.ceil(math.log2(max(1.0, 8e-6 * v)))))


def colsum_inputs(shape, tdt, seed=0):
    n, v, c = shape
    x = randn_storage((n, v, c), tdt, 7000 + seed)
    x[:, torch.tensor(colsum_seams(v, c)), :] = colsum_outlier(v)
    return x


def lp_colsum_ref(x, scale):
    """-> out (N, C) fp64, bound unit eps32 * |scale| * sum |x|"""
    scale = f32(scale)
    xd = x.double()
    return scale * xd.sum(1), EPS32 * abs(scale) * xd.abs().sum(1)


def lp_colsum_f32(x, scale):
    """per block, a lane adds every vstep-th voxel of its octet in fp32 and empties the sum into fp64 after every 256 additions; lanes,
    blocks and the scale in fp64; one rounding"""
    n, v, c = x.shape
    B = colsum_blocks(v)
    per = (v + B - 1) // B
    vstep = 256 // (c // 8)
    tot = torch.zeros((n, c), dtype=F64)
    xf = x.float()
    for b in range(B):
        blk = xf[:, b * per:min((b + 1) * per, v)]
        if blk.shape[1] == 0:
            continue
        pad = (-blk.shape[1]) % vstep
        blk = torch.cat([blk, torch.zeros((n, pad, c))], 1).reshape(n, -1, vstep, c)
        fs = torch.zeros((n, vstep, c))
        for t in range(blk.shape[1]):
            fs = fs + blk[:, t]
            if (t + 1) % 256 == 0:              # (padding rows add exact zeros: the lanes that ran out flush nothing new)
                tot += fs.double().sum(1)
                fs = torch.zeros((n, vstep, c))
        tot += fs.double().sum(1)
    return (tot * f32(scale)).float()


# ----------------------------------------------------------------------------------------------------------------
# ResNet block epilogue (+ head)
# ----------------------------------------------------------------------------------------------------------------
# (N, V, C, G, mode)
EPILOGUE_CHUNKED = [(1, 2048, 8, 8, SLAB), (1, 768, 64, 8, SLAB), (2, 2304, 16, 2, SLAB), (1, 72, 256, 8, CHANNEL)]
EPILOGUE_STRIDE = [(1, 3, 8, 1, SLAB), (2, 384, 32, 8, SLAB), (1, 100, 256, 8, CHANNEL)]
EPILOGUE_PAST_CAP = (1, 4194305, 8, 1, SLAB)
EPILOGUE_HEAD = [s for s in EPILOGUE_CHUNKED if s[2] <= 64]


def epilogue_inputs(shape, tdt, seed=0, k=0):
    """res, c2 (N, V, C) storage; wsp (C) scaled so that the gate's argument has deviation 2 (both tails of the sigmoid, |a| <= 16);
    ch (N, C) in [0, 1); head weights (C, k) with pre-activations of deviation ~2"""
    n, v, c, g, mode = shape
    res = randn_storage((n, v, c), tdt, 8000 + seed)
    c2 = randn_storage((n, v, c), tdt, 8100 + seed)
    gen = torch.Generator().manual_seed(8200 + seed)
    wsp = torch.randn(c, generator=gen) * (2.0 / math.sqrt(c))
    ch = torch.rand((n, c), generator=gen)
    gamma, beta, mean, rstd = gn_params(n, c, g, seed + 50)
    out = dict(res=res, c2=c2, wsp=wsp, ch=ch, gamma=gamma, beta=beta, mean=mean, rstd=rstd)
    if k:
        out['hw'] = torch.randn((c, k), generator=gen) * (0.7 / math.sqrt(c))
        out['hb'] = torch.randn(k, generator=gen) * 0.5
    return out


def sigmoid_bound(a, da):
    """bound (absolute) of s = sigmoid(a) through __expf, the argument a itself good to da (absolute, its own K already in it):
    K_GATE eps32 (s (1 - s) (|a| + 1) + s)  +  s (1 - s) da.  What the argument carries is added ONCE, outside K_GATE (see the docstring)."""
    assert float(a.abs().max()) <= GATE_MAX_ARG
    s = torch.sigmoid(a)
    return K_GATE * EPS32 * (s * (1.0 - s) * (a.abs() + 1.0) + s) + s * (1.0 - s) * da + TINY


def epilogue_ref(p, g, mode, lo=0, v=None):
    """-> sp (N, V), its bound, out (N, V, C) fp64, its bound: both ABSOLUTE, every K applied once -- the tests hold the kernel to 1 and
    the restatement to 1/4 of them.  sp = sigmoid(dot): sigmoid_bound with the dot product's K_LP eps32 sum |res| |wsp|.
    out = res (sp + ch) + relu(GN(c2)):  K_LP eps32 B,  B = |res| (sp + |ch|) + B_gn,  plus |res| * bound(sp), what sp carries in.
    lo, v: as gn_apply_ref"""
    res, c2 = p['res'].double(), p['c2']
    w = p['wsp'].double()
    dot = (res * w).sum(-1)
    Bdot = (res.abs() * w.abs()).sum(-1)
    sp = torch.sigmoid(dot)
    bsp = sigmoid_bound(dot, K_LP * EPS32 * Bdot)
    t, Bt = gn_apply_ref(c2, p['gamma'], p['beta'], p['mean'], p['rstd'], g, mode, True, lo, v)
    chd = p['ch'].double()[:, None, :]
    out = res * (sp[..., None] + chd) + t
    B = res.abs() * (sp[..., None] + chd.abs()) + Bt / EPS32
    return sp, bsp, out, K_LP * EPS32 * B + res.abs() * bsp[..., None] + TINY


def _dot_f32(x, w):
    """sum over the last axis as the oct kernels do: an fma chain down each octet, then a pairwise tree across the octets"""
    c = x.shape[-1]
    xo = x.reshape(x.shape[:-1] + (c // 8, 8))
    wo = w.reshape(c // 8, 8)
    acc = torch.zeros(xo.shape[:-1])
    for e in range(8):
        acc = fma32(xo[..., e], wo[:, e].expand_as(acc), acc)
    while acc.shape[-1] > 1:
        acc = acc[..., 0::2] + acc[..., 1::2]
    return acc[..., 0]


def epilogue_f32(p, g, mode, fused):
    res = p['res'].float()
    dot = _dot_f32(res, p['wsp'])
    sp = 1.0 / (1.0 + torch.exp(-dot))
    t = gn_apply_f32(p['c2'], p['gamma'], p['beta'], p['mean'], p['rstd'], g, mode, True, fused)
    return sp, fma32(res, sp[..., None] + p['ch'][:, None, :], t)


def linear_sigmoid_bound(h, Bh, extra, sigmoid):
    """bound (absolute, every K applied once) of y = sigmoid?(h): h's own bound is K_LP eps32 Bh + extra (extra: absolute, what the
    inputs of the dot product already carry); the sigmoid adds its K_GATE term and passes h's bound on times y (1 - y)"""
    dh = K_LP * EPS32 * Bh + extra
    return sigmoid_bound(h, dh) if sigmoid else dh + TINY


def epilogue_head_ref(p, g, mode, bias, sigmoid):
    """y[v][k] = sigmoid?(sum_c out[v][c] W[c][k] + b[k]) on the UNROUNDED out -- fp64 directly"""
    _, _, out, bout = epilogue_ref(p, g, mode)
    W = p['hw'].double()
    h = out @ W
    Bh = out.abs() @ W.abs()
    if bias:
        h = h + p['hb'].double()
        Bh = Bh + p['hb'].double().abs()
    y = torch.sigmoid(h) if sigmoid else h
    return y, linear_sigmoid_bound(h, Bh, bout @ W.abs(), sigmoid)


def _head_dot_f32(x, w, bias):
    k = w.shape[1]
    cols = [_dot_f32(x, w[:, j].contiguous()) for j in range(k)]
    h = torch.stack(cols, -1)
    return h + bias if bias is not None else h


def epilogue_head_f32(p, g, mode, bias, sigmoid):
    _, out = epilogue_f32(p, g, mode, True)
    h = _head_dot_f32(out, p['hw'], p['hb'] if bias else None)
    return 1.0 / (1.0 + torch.exp(-h)) if sigmoid else h


# ----------------------------------------------------------------------------------------------------------------
# output head and its backward
# ----------------------------------------------------------------------------------------------------------------
# (nvox, C, K)
HEAD_PER_VOXEL = [(1, 8, 1), (4095, 32, 3), (5000, 24, 2)]
HEAD_OCT = [(4096, 16, 1), (4097, 32, 3), (5003, 64, 4), (4100, 256, 2)]
HEAD_BWD = [(1, 16, 1), (255, 32, 3), (4099, 64, 4)]
HEAD_BWD_PAST_CAP = (300007, 16, 2)


def head_inputs(shape, tdt, seed=0):
    nvox, c, k = shape
    x = randn_storage((nvox, c), tdt, 9000 + seed)
    gen = torch.Generator().manual_seed(9100 + seed)
    w = torch.randn((c, k), generator=gen) * (2.0 / math.sqrt(c))
    b = torch.randn(k, generator=gen) * 0.5
    return x, w, b


def head_ref(x, w, b, sigmoid):
    xd, wd = x.double(), w.double()
    h, Bh = xd @ wd, xd.abs() @ wd.abs()
    if b is not None:
        h, Bh = h + b.double(), Bh + b.double().abs()
    return (torch.sigmoid(h) if sigmoid else h), linear_sigmoid_bound(h, Bh, 0.0, sigmoid)


def head_f32(x, w, b, sigmoid, oct_form):
    """per-voxel kernel: one fma chain over the C channels; oct kernel: a chain per octet, a tree across"""
    xf = x.float()
    if oct_form:
        h = _head_dot_f32(xf, w, None)
    else:
        h = torch.zeros((x.shape[0], w.shape[1]))
        for c in range(x.shape[1]):
            h = fma32(xf[:, c:c + 1].expand_as(h), w[c].expand_as(h), h)
    if b is not None:
        h = h + b
    return 1.0 / (1.0 + torch.exp(-h)) if sigmoid else h


def head_bwd_inputs(shape, tdt, seed=0):
    """x storage, dpre fp32, w fp32; seam voxels (two per 256 octets) carry 8 in x and in dpre"""
    nvox, c, k = shape
    x = randn_storage((nvox, c), tdt, 9500 + seed)
    dpre = randn32((nvox, k), 9600 + seed)
    w = randn32((c, k), 9700 + seed, 0.5)
    idx = torch.tensor(head_bwd_seams(nvox, c))
    x[idx] = 8.0
    dpre[idx] = 8.0
    return x, dpre, w


def head_bwd_ref(x, dpre, w, old_dw=None, old_db=None):
    """-> dx, dw, db fp64 and bound units (eps32 * B): dx B = sum_k |dpre| |w|; dw B = sum_v |x| |dpre| (+ |old| + |new| when it
    accumulates: fl32(old + fl32(new))); db alike"""
    xd, dd, wd = x.double(), dpre.double(), w.double()
    dx, Bx = dd @ wd.t(), dd.abs() @ wd.abs().t()
    dw, Bw = xd.t() @ dd, xd.abs().t() @ dd.abs()
    db, Bb = dd.sum(0), dd.abs().sum(0)
    if old_dw is not None:
        Bw = Bw + old_dw.double().abs() + dw.abs()
        dw = dw + old_dw.double()
    if old_db is not None:
        Bb = Bb + old_db.double().abs() + db.abs()
        db = db + old_db.double()
    return (dx, dw, db), (EPS32 * Bx, EPS32 * Bw, EPS32 * Bb)


def head_bwd_f32(x, dpre, w, old_dw=None, old_db=None):
    """dx: an fma chain over k; dw, db: the small shapes give every lane one voxel, so the fp32 part is the product and the shuffle
    tree of a wave's 64 / (C/8) voxels; waves and workgroups in fp64"""
    nvox, c = x.shape
    k = dpre.shape[1]
    xf = x.float()
    dx = torch.zeros((nvox, c))
    for j in range(k):
        dx = fma32(dpre[:, j:j + 1].expand_as(dx), w[:, j].expand_as(dx), dx)
    vpw = 64 // (c // 8)
    pad = (-nvox) % vpw
    xp = torch.cat([xf, torch.zeros((pad, c))], 0).reshape(-1, vpw, c)
    dp = torch.cat([dpre, torch.zeros((pad, k))], 0).reshape(-1, vpw, k)
    prod = xp[..., :, None] * dp[..., None, :]                  # (waves, vpw, c, k): fma(x, d, 0)
    bsum = dp
    while prod.shape[1] > 1:
        prod = prod[:, 0::2] + prod[:, 1::2]
        bsum = bsum[:, 0::2] + bsum[:, 1::2]
    dw = prod[:, 0].double().sum(0).float()
    db = bsum[:, 0].double().sum(0).float()
    if old_dw is not None:
        dw = old_dw + dw
    if old_db is not None:
        db = old_db + db
    return dx, dw, db


# ----------------------------------------------------------------------------------------------------------------
# samplers: selections and copies are bit-exact
# ----------------------------------------------------------------------------------------------------------------
# (N, D, H, W, C): the INPUT grid of the pool, the COARSE grid of the repeat
MAXPOOL_SHAPES = [(1, 2, 2, 2, 8), (2, 2, 4, 6, 16)]
UPSAMPLE_SHAPES = [(1, 1, 1, 1, 8), (2, 3, 1, 5, 24)]
UPSAMPLE_PAST_CAP = (1, 66, 64, 128, 8)


def windows(x):
    """x (N, D, H, W, C) -> (N, D/2, H/2, W/2, C, 8): the 2x2x2 windows in scan order t = dz*4 + dy*2 + dx"""
    n, d, h, w, c = x.shape
    v = x.reshape(n, d // 2, 2, h // 2, 2, w // 2, 2, c)
    return v.permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, d // 2, h // 2, w // 2, c, 8)


def unwindows(wnd):
    n, d, h, w, c, _ = wnd.shape
    v = wnd.reshape(n, d, h, w, c, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4)
    return v.reshape(n, 2 * d, 2 * h, 2 * w, c)


def maxpool_inputs(shape, tdt, seed=0):
    """random values on a coarse grid (ties are frequent) with planted windows: all equal, all negative, -0.0 before +0.0 and +0.0
    before -0.0 among negatives, the maximum in the last position"""
    n, d, h, w, c = shape
    g = torch.Generator().manual_seed(9800 + seed)
    x = (torch.randint(-4, 5, shape, generator=g).float() * 0.5).to(tdt)
    wn = windows(x).clone()
    f = wn.reshape(-1, 8)
    f[0] = 1.5
    f[1] = -torch.arange(1, 9).to(tdt)
    f[2] = -1.0
    f[2, 3] = -0.0
    f[2, 5] = 0.0
    f[3] = -1.0
    f[3, 2] = 0.0
    f[3, 6] = -0.0
    f[4] = -2.0
    f[4, 7] = 3.0
    return unwindows(f.reshape(wn.shape)).contiguous()


def maxpool_ref(x):
    """first maximum in scan order, from -inf with a strict > (downsample.py:51-70 has no tie rule of its own; the fp32 engine's is this)
    -> y (storage type, the selected element itself), idx uint8"""
    wn = windows(x)
    wf = wn.float()
    best = torch.full(wf.shape[:-1], -math.inf)
    bi = torch.zeros(wf.shape[:-1], dtype=torch.long)
    for t in range(8):
        m = wf[..., t] > best
        best = torch.where(m, wf[..., t], best)
        bi = torch.where(m, torch.full_like(bi, t), bi)
    return best.to(x.dtype), bi.to(torch.uint8)


def maxpool_bwd_ref(dy, idx, old=None):
    """dx = dy at the window position idx, 0 elsewhere (+ old: ONE fp32 addition, then RNE) -> storage type, exact"""
    oh = torch.nn.functional.one_hot(idx.long(), 8).bool()
    wn = torch.where(oh, dy.float()[..., None], torch.zeros(()))
    dx = unwindows(wn)
    if old is not None:
        dx = old.float() + dx
    return dx.to(dy.dtype)


def upsample_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)


def upsample_bwd_ref(dy, old=None):
    """-> dx fp64, bound unit eps32 * (sum of the 8 |dy| (+ |old|))"""
    wn = windows(dy.double())
    s, B = wn.sum(-1), wn.abs().sum(-1)
    if old is not None:
        s, B = s + old.double(), B + old.double().abs()
    return s, EPS32 * B


def upsample_bwd_f32(dy, old=None):
    wn = windows(dy.float())
    s = torch.zeros(wn.shape[:-1])
    for t in range(8):
        s = s + wn[..., t]
    return s + old.float() if old is not None else s


# ----------------------------------------------------------------------------------------------------------------
# casts: an edge table, bit-exact against torch's CPU cast
# ----------------------------------------------------------------------------------------------------------------
def cast_edge_values():
    """fp32 values: ties to even of both types, fp16's 65504 / 65520 / 1e5, fp16 subnormals and 2^-25, +-0, +-inf, NaN, the largest
    bf16-representable fp32 and the next fp32 above it"""
    import numpy as np
    v = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan,
         1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -11 - 2.0 ** -24,        # fp16 ties at 1
         1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 1.0 + 2.0 ** -8 - 2.0 ** -24,            # bf16 ties at 1
         -(1.0 + 2.0 ** -11), -(1.0 + 3 * 2.0 ** -8), 2048.0 + 1.0, 2048.0 + 3.0, 256.0 + 1.0, 256.0 + 3.0,
         65504.0, 65519.996, 65520.0, -65520.0, 65536.0, 1e5, -1e5,
         2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -25, 2.0 ** -25, 2.0 ** -25 + 2.0 ** -40, 2.0 ** -26, -2.0 ** -25,
         5 * 2.0 ** -25, 1023 * 2.0 ** -24 + 2.0 ** -25,
         2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 2.0 ** -149,
         float(np.float32(3.3895313892515355e38)), float(np.nextafter(np.float32(3.3895313892515355e38), np.float32(np.inf))),
         float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max)]
    return torch.tensor(v, dtype=F32)


def cast_table(rows_of, c):
    """the edge values, cycled into (rows_of, c) fp32"""
    e = cast_edge_values()
    n = rows_of * c
    return e.repeat((n + e.numel() - 1) // e.numel())[:n].reshape(rows_of, c).contiguous()


def same_bits_or_nan(got, want):
    """storage-type or fp32 tensors: equal bit for bit, NaN equal to NaN of any payload"""
    it = torch.int16 if got.element_size() == 2 else torch.int32
    gn, wn = torch.isnan(got.float()), torch.isnan(want.float())
    return bool(torch.equal(gn, wn)) and bool(torch.equal(got.view(it)[~gn], want.view(it)[~wn]))


def chunks(v, width=1 << 18):
    """voxel ranges that cover [0, v): the shapes past a grid cap are compared piece by piece (their fp64 references are large)"""
    return [(lo, min(v, lo + width)) for lo in range(0, v, width)]
