"""Reference, fp32 restatement and error bounds for the compound loss kernels (csrc/loss_ce.hip), in the three-part scheme of
tests/step_ref.py, whose helpers and K rule this module uses.  Plain Python on the CPU.

  1. REFERENCE: torch float64, written from the formulas of the issue / DESIGN.md ("Compound loss"), autograd through torch.clamp;
     the Dice and VAE part is step_ref.loss_ref's (oracle.torch_ref.dice_vae_loss).
  2. RESTATEMENT: torch float32 on the CPU in the operation order the comment at the top of csrc/loss_ce.hip states.
  3. BOUNDS  |err| <= K * eps32 * B + TINY, B = the sum of the absolute values of the terms that are added.

The scalars gamma, w_pos, w_neg, w_dice, w_ce and gscale enter every function rounded to fp32, as the C ABI receives them.

THE CROSS-ENTROPY SUMS (per channel; K_CE_SUM = 16).  B = sum over the elements of
    w_pos t (1-q)^gamma (|log q| + 1 + gamma)  +  w_neg (1-t) q^gamma (|log(1-q)| + 1 + gamma)
All terms are positive: nothing cancels.  The "+ 1" pays for the rounding of the logarithm's argument 1 - q (relative eps32 of the
argument is an absolute eps32 of the logarithm), the "+ gamma" for the same rounding under the power.  Roundings of one term, in units
of eps32 of its share of B: logf 2 (1 ulp), the power 2 (powf: 1 ulp; by products: gamma - 1 roundings, 1 at gamma = 2, the tests' only integer), two or three products 3, the sum of the two halves 1, the conversion of
the fp32 term into the fp64 accumulator 0 -- 8 in the worst case, next power of two 16.  The accumulation itself is fp64.

THE GRADIENT (K_CE_GRAD = 32).  B = w_dice * (step_ref's Dice B) + |kce| * [ w_pos t (|T1| + |T2|) + w_neg (1-t) (|T3| + |T4|) ],
    T1 = gamma q (1-q)^gamma log q,  T2 = (1-q)^(gamma+1),  T3 = gamma q^gamma (1-q) log(1-q),  T4 = q^(gamma+1),
    kce = w_ce gscale / (count C); every T divided by q (1-q) when the gradient is not taken through the sigmoid; zero outside the clamp.
The gradient takes log(1-q) as log1pf(-q): logf(1 - q) would carry the rounding of 1 - q, eps32 / q relative to a logarithm of size q,
into T3, which is as large as the T4 it is added to (found by the K/4 rule: 160 to 320 bound units at p = 6e-4, t = 0, gamma > 0).
Roundings along the longest chain (T1, gamma <= 2, not through the sigmoid): 1 - q 1 (under the power: gamma <= 2 more), powf 2,
logf 2, gamma * q * lq 2, the difference 1, the product with pa 1, w_pos * t and the product 2, the sum of the two halves 1, q * om and
the division 2, kce (its own rounding and the product) 2, the sum with the Dice gradient 1 -- 19, next power of two 32.  For gamma
above 2 the argument's share under the power grows by eps32 per unit of gamma; the tests stay at gamma <= 2.

THE VALUE: fp64 from the sums, one rounding: value_bound = step_ref's with its 1.0 scaled by w_dice, plus w_ce * K_CE_SUM * eps32 *
mean(B of the sums).

MEASURED RESTATEMENT RATIOS (max over elements of |restatement - reference| / (eps32 * B); tests/test_loss_ce_host.py prints them with
-s).  Over step_ref.LOSS_SHAPES_SMALL, both through_sigmoid values, the three gscale values and the four (gamma, alpha) cases:
  CE sums 0.035 (0.42 on the saturated inputs, 0.02 on soft targets) of K_CE_SUM / 4 = 4: thousands of terms, the roundings average out
  dlogit 4.39 through the sigmoid, 4.47 not (2.19 on the saturated inputs, 4.05 on soft targets; 3.98 and 5.05 on the two shapes past
  the grid caps) of K_CE_GRAD / 4 = 8
On the GPU (tests/test_loss_ce_gpu.py): CE sums <= 0.50 of 16, dlogit <= 4.62 of 32; with w_ce = 0, dlogit 2.87 of step_ref's 16.
"""
import torch

import step_ref as S
from step_ref import (EPS32, LOSS_SHAPE_PAST_BWD, LOSS_SHAPE_PAST_PARTIAL, LOSS_SHAPES_SMALL, TINY, check, f32, fma32,  # noqa: F401
                      loss_inputs, ratio)

F64, F32 = torch.float64, torch.float32

EPS = 2.0 ** -23                 # the clamp: q = min(max(p, EPS), 1 - EPS), both bounds exact in fp32
K_CE_SUM = 16
K_CE_GRAD = 32
CASES = [(0.0, None), (2.0, None), (2.0, 0.25), (0.5, None)]      # (gamma, alpha) of the issue
AXES = (0, 1, 2, 3)


def weights(gamma, alpha):
    """(gamma, w_pos, w_neg) rounded to fp32, as util.LossSpec.kernel_args hands them to the C ABI"""
    if alpha is None:
        return f32(gamma), 1.0, 1.0
    return f32(gamma), f32(alpha), f32(1.0 - alpha)


def ce_terms64(p, t, gamma, wp, wn):
    """the per-element term e of the issue, float64, differentiable in p through torch.clamp"""
    q = torch.clamp(p, EPS, 1.0 - EPS)
    return wp * t * (1.0 - q) ** gamma * (-torch.log(q)) + wn * (1.0 - t) * q ** gamma * (-torch.log(1.0 - q))


def ce_value64(p, t, gamma, wp, wn):
    """CE = sum(e) / (N V C)"""
    return ce_terms64(p, t, gamma, wp, wn).sum() / p.numel()


def seg_loss_ref(p, y, x=None, yv=None, proj=None, gs=1.0, through_sigmoid=True, gamma=0.0, alpha=None, w_dice=1.0, w_ce=1.0,
                 count=None):
    """fp64 reference and bounds.  count: the global N V when p is one shard of a larger batch (default: p's own)."""
    base = S.loss_ref(p, y, x, yv, proj, gs=gs, through_sigmoid=through_sigmoid)
    gamma, wp, wn = weights(gamma, alpha)
    w_dice, w_ce, gs = f32(w_dice), f32(w_ce), f32(gs)
    c = p.shape[-1]
    count = float(p.numel() // c) if count is None else float(count)
    pd = p.double().requires_grad_(True)
    td = y.double()
    e = ce_terms64(pd, td, gamma, wp, wn)
    e.sum().backward()
    kce = w_ce * gs / (count * c)
    pv = pd.detach()
    q = torch.clamp(pv, EPS, 1.0 - EPS)
    om, lq, l1 = 1.0 - q, torch.log(q), torch.log(1.0 - q)
    inside = ((pv >= EPS) & (pv <= 1.0 - EPS)).double()
    T1, T2 = gamma * q * om ** gamma * lq, om ** (gamma + 1.0)
    T3, T4 = gamma * q ** gamma * om * l1, q ** (gamma + 1.0)
    Bg = abs(kce) * (wp * td * (T1.abs() + T2.abs()) + wn * (1.0 - td) * (T3.abs() + T4.abs())) * inside
    gce = kce * pd.grad
    if through_sigmoid:
        gce = gce * pv * (1.0 - pv)
    else:
        Bg = Bg / (q * om)
    ce_sums = e.detach().sum(AXES)
    B_sums = (wp * td * om ** gamma * (lq.abs() + 1.0 + gamma) + wn * (1.0 - td) * q ** gamma * (l1.abs() + 1.0 + gamma)).sum(AXES)
    ce = float(ce_sums.sum()) / (count * c)
    out = dict(base)
    out.update(ce=ce, ce_sums=ce_sums, B_ce_sums=EPS32 * B_sums, loss=w_dice * base['dice'] + (base['loss'] - base['dice']) + w_ce * ce,
               dlogit=w_dice * base['dlogit'] + gce, B_dlogit=w_dice * base['B_dlogit'] + EPS32 * Bg, dlogit_ce=gce,
               value_bound=base['value_bound'] - 4 * EPS32 * (1.0 - w_dice) + w_ce * K_CE_SUM * EPS32 * float(B_sums.sum()) / (count * c),
               count=count)
    return out


# ---- the fp32 restatement, in the operation order of csrc/loss_ce.hip ----------------------------------------------------------------
def _t32(v):
    return torch.tensor(f32(v), dtype=F32)


def _pw32(b, gamma):
    """pw of csrc/loss_ce.hip: gamma = 1, ..., 8 by products left to right, any other gamma by powf"""
    if gamma == int(gamma):
        r = b
        for _ in range(1, int(gamma)):
            r = r * b
        return r
    return torch.pow(b, _t32(gamma))


def ce_terms_f32(p, t, gamma, wp, wn):
    q = torch.clamp(p, f32(EPS), f32(1.0 - EPS))
    om = 1.0 - q
    lq, l1 = torch.log(q), torch.log(om)
    a, b = _t32(wp) * t, _t32(wn) * (1.0 - t)
    if gamma != 0.0:
        a = a * _pw32(om, gamma)
        b = b * _pw32(q, gamma)
    return a * (-lq) + b * (-l1)


def seg_sums_f32(p, y, x, yv, proj, gamma=0.0, alpha=None):
    """bts_seg_loss_sums: step_ref.loss_sums_f32's 3C+4, the fp32 terms e summed in fp64 per channel, N V -> (4C+5,) float64"""
    gamma, wp, wn = weights(gamma, alpha)
    e = ce_terms_f32(p, y, gamma, wp, wn)
    assert e.dtype == F32
    c = p.shape[-1]
    return torch.cat([S.loss_sums_f32(p, y, x, yv, proj), e.double().sum(AXES), torch.tensor([float(p.numel() // c)], dtype=F64)])


def seg_value_f64(sums, c, has_vae, w_dice=1.0, w_ce=1.0):
    """bts_seg_loss_value from the raw sums -> (loss, [dice, l2, kl, ce]) as fp32-rounded floats"""
    _, (d, l2, kl) = S.loss_value_f64(sums, c, has_vae)
    d64 = float((1.0 - (2.0 * sums[:c] + 1.0) / (sums[c:2 * c] + sums[2 * c:3 * c] + 1.0)).sum()) / c
    l264 = float(sums[3 * c] / sums[3 * c + 2]) if has_vae else 0.0
    kl64 = float(sums[3 * c + 1] / sums[3 * c + 3]) if has_vae else 0.0
    ce = float(sums[3 * c + 4:4 * c + 4].sum() / (sums[4 * c + 4] * c))
    return f32(f32(w_dice) * d64 + f32(w_ce) * ce + 0.1 * l264 + 0.1 * kl64), [d, l2, kl, f32(ce)]


def seg_bwd_f32(p, y, x, yv, proj, sums, gs=1.0, through_sigmoid=True, gamma=0.0, alpha=None, w_dice=1.0, w_ce=1.0):
    """bts_seg_loss_bwd as the comment of csrc/loss_ce.hip states it -> dlogit, dyvae, dproj (the last two: step_ref.loss_bwd_f32's)"""
    gamma, wp, wn = weights(gamma, alpha)
    c = p.shape[-1]
    gs64, wd, wc = f32(gs), f32(w_dice), f32(w_ce)
    D = sums[c:2 * c] + sums[2 * c:3 * c] + 1.0
    k1 = (-2.0 / (c * D) * gs64 * wd).float()
    k2 = (2.0 * (2.0 * sums[:c] + 1.0) / (c * D * D) * gs64 * wd).float()
    g = k1 * y + k2 * p
    if through_sigmoid:
        g = g * (p * (1.0 - p))
    kce = torch.tensor(wc / (float(sums[4 * c + 4]) * c) * gs64, dtype=F64).float()
    inside = (p >= f32(EPS)) & (p <= f32(1.0 - EPS))
    q = torch.clamp(p, f32(EPS), f32(1.0 - EPS))
    om = 1.0 - q
    if gamma == 0.0:
        pos, neg = -om, q
    else:
        g32 = _t32(gamma)
        lq, l1 = torch.log(q), torch.log1p(-q)          # (log1pf in the gradient: see the kernel's comment)
        pos = _pw32(om, gamma) * (g32 * q * lq - om)
        neg = _pw32(q, gamma) * (q - g32 * om * l1)
    s = _t32(wp) * y * pos + _t32(wn) * (1.0 - y) * neg
    if not through_sigmoid:
        s = s / (q * om)
    out = torch.where(inside, g + kce * s, g)
    assert out.dtype == F32
    if x is None:
        return out, None, None
    _, dyv, dproj = S.loss_bwd_f32(p, y, x, yv, proj, sums[:3 * c + 4], gs=gs, through_sigmoid=through_sigmoid)
    return out, dyv, dproj


# ---- inputs at the clamp -------------------------------------------------------------------------------------------------------------
SATURATION_P = [0.0, EPS / 2, EPS, 1.0 - EPS, 1.0 - EPS / 2, 1.0]      # all exact in fp32 (1 - EPS / 2 = 1 - 2^-24 is the fp32 below 1)


def saturation_inputs(c=3, reps=7):
    """every p of SATURATION_P against t = 0 and t = 1, `reps` times over: (1, 1, reps, 12, c) tensors"""
    pv = torch.tensor(SATURATION_P, dtype=F64).float()
    assert torch.equal(pv.double(), torch.tensor(SATURATION_P, dtype=F64))
    p = pv.repeat(2).view(1, 1, 1, 12, 1).expand(1, 1, reps, 12, c).contiguous()
    t = torch.tensor([0.0] * 6 + [1.0] * 6).view(1, 1, 1, 12, 1).expand(1, 1, reps, 12, c).contiguous()
    return p, t


def soft_targets(shape, seed=0):
    """t on {0, 0.25, 1} (all exact in fp32)"""
    g = torch.Generator().manual_seed(4000 + seed)
    return torch.tensor([0.0, 0.25, 1.0])[torch.randint(0, 3, shape, generator=g)]
