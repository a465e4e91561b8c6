"""References, fp32 restatements and error bounds for the kernels that close the training step
(csrc/loss.hip, optim.hip, dense.hip, pointwise.hip, augment.hip's moments and bts_colsum in se.hip).  Plain Python on the CPU.

For every kernel this module holds
  1. the fp64 REFERENCE (oracle/torch_ref.py where a function exists, autograd for the gradients),
  2. an fp32 RESTATEMENT: the formula the header and the kernel's comment cite, in torch float32 on the CPU, in the
     documented operation order, and
  3. the BOUND  |err| <= K * eps32 * B + TINY  (SURVEY 8c), B = the sum of the absolute values of the terms that are
     added, so cancellation is paid for where it happens.  eps32 = 2^-24 (unit roundoff), TINY = 2^-126 (the smallest
     normal fp32: a result below it may be flushed).

THE K RULE.  tests/test_step_kernels_gpu.py uses the K below unchanged.  tests/test_step_kernels_host.py holds every
restatement to K/4 of its bound (the margin between the arithmetic as written and the arithmetic a compiler may
legally produce: fma contraction, another association of a product).  A restatement above K/4, or the GPU above K, is
a finding to be explained from the arithmetic -- never a reason to raise a number.

Bounds that carry no K/4 margin, by their own arithmetic (each is a finding of the K/4 rule, explained here; no K was raised):
  * bounds WITHOUT a K (column sums, channel moments, the L2 value, the loss sums): fp64 accumulation, then ONE
    rounding to fp32.  One rounding errs by up to 1.0 * eps32 * |ref|, so the restatement is held to the bound itself.
  * bts_sigmoid_bwd and bts_dropout_apply (K = 4, B = |ref|: one product, nothing is added): dy * y * (1 - y) takes
    three roundings and x * (1 / (1 - rate)) takes three (the subtraction, the reciprocal, the product).  The worst
    case is 3 eps32 |ref| < K and a restatement can sit anywhere below it: held to ROUNDINGS[...] = 3, not to K/4 = 1.
  * bts_vae_sample_fwd / _bwd (K = 8): exp (1 ulp = 2 eps32), two products, one addition: 5 eps32 B in the worst
    case; measured 2.95 on 640 elements.  Held to ROUNDINGS['vae_sample'] = 5.
  * bts_normal (K = 16): the cosine's argument 2 pi u2 lies in [4, 2 pi) for a third of the draws, where one fp32 ulp
    is 2^-21: rounding the product moves the cosine by up to 4 eps32 |sin|.  With logf (2), sqrtf (1), cosf (2) and
    the final product (1) that is 9 eps32 sqrt(-2 ln u1) at most (the root halves logf's share); measured 4.64 with
    numpy's float32 functions.  Held to ROUNDINGS['normal'] = 9.
  * Dense dW and db (K = 8): fma chains over the N <= 9 samples of the batch.  A chain of N terms errs by up to
    N eps32 B, and the maximum over the 257,000 weights of so short a chain comes close to sqrt(N) eps32 B (3.14 at
    N = 9, 1.98 at N = 2), where the long input contractions average their roundings out (0.16 .. 0.98).  Held to
    dense_short_chain_limit(N) = min(N, K/2): the chain's own worst case, or half of K.

The references take every SCALAR argument rounded to fp32, as the C ABI receives it (beta1, beta2, eps, lr_t, gmul,
rate, scale, a, ca, cb), and form 1 - beta from the rounded value (exact in fp32 for beta in [0.5, 1]): a difference
between the fp64 and the fp32 value of a constant is an input, not an error of the kernel.

The loss gradient "through the sigmoid" is dL/dp * p * (1 - p) AT THE fp32 PROBABILITY p the kernel is handed
(decoder.py:60 fuses the sigmoid into the conv; the logit is gone).  The reference therefore differentiates the oracle's
loss with respect to p and multiplies by p (1 - p) in fp64; autograd through sigmoid(logit) would compare against
1 - sigmoid(logit), which differs from 1 - fl32(p) by eps32 / (1 - p) in the upper tail.

MEASURED RESTATEMENT RATIOS (max over elements of |restatement - reference| / (eps32 * B); tests/test_step_kernels_host.py
prints them with -s).  Loss, over the five shapes, both through_sigmoid values and the three gscale values:
  dlogit 3.76 (64x64x72; 3.46 at 96x96x120; <= 1.5 on the small shapes)   dyvae 2.11   dproj mean 1.53   dproj logvar 0.75
  sums I, T 0 (products with a {0,1} label are exact), P 0.06 of eps32 * sum
Adam, 3 steps, gmul 1, 0.125, 2^-16, p0 = 0 and p0 ~ N(0,1):   p 3.40   m 1.70   v 1.86
  (sqrt(v + eps) instead of sqrt(v) + eps: > 16,000 bounds away from p0 = 0; at g = 1e-8, step 1, the updates are
  3.15e-3 lr and 1.0e-6 lr.)
Dense: fwd 0.16 .. 0.98   dx 0.58 .. 1.48   dW 0.19 .. 3.14   db 0 .. 1.41
L2 gradient 1.00   column sums 0.92   moments: mean 0.45, variance 0.03   axpy 0.99   sigmoid_bwd 2.47
dropout_apply 1.06   scalar_lincomb 0.51   sampling fwd 1.61, bwd 2.95   normal 4.64
Generator statistics (n = 2^20, seeds 7 and 1234): every statistic within 2.2 sigma.
"""
import math

import numpy as np
import torch

from oracle import torch_ref as R

EPS32 = 2.0 ** -24
TINY = 2.0 ** -126

K_LOSS_GRAD = 16
K_ADAM = 16
K_DENSE = 8
K_EW = 4
K_L2_GRAD = 4
K_VAE = 8
K_NORMAL = 16
ROUNDINGS = {'sigmoid_bwd': 3, 'dropout_apply': 3, 'vae_sample': 5, 'normal': 9}


def dense_short_chain_limit(n):
    """host limit for dW / db, fma chains over the n samples of the batch (see the docstring)"""
    return min(n, K_DENSE / 2)

F64 = torch.float64
F32 = torch.float32


def f32(v):
    """a python scalar rounded to fp32, as the C ABI receives it"""
    return float(np.float32(v))


def ratio(got, ref, bound):
    """max over elements of (|got - ref| - TINY) / bound; 0 where err <= TINY (also where bound == 0)"""
    err = (got.double() - ref.double()).abs() - TINY
    err = torch.clamp(err, min=0.0)
    if err.numel() == 0:
        return 0.0
    b = torch.as_tensor(bound, dtype=F64).expand_as(err)
    r = torch.where(err > 0, err / b, torch.zeros_like(err))      # err > 0 on a zero bound -> inf
    return float(r.max())


def check(got, ref, bound, k, what):
    """assert |got - ref| <= k * bound + TINY element-wise (bound already carries eps32); prints the measured ratio first"""
    got = got.detach().double().cpu()
    assert not torch.isnan(got).any(), '%s: NaN in the result' % what
    r = ratio(got, ref, bound)
    print('%-44s ratio %.3f of K = %g' % (what, r, k))
    assert r <= k, '%s: error is %.3f x its bound unit (K = %g), max|ref| %.3e' % (what, r, k, float(ref.abs().max()) if ref.numel() else 0)


def fma32(a, b, c):
    """fl32(a * b + c): the product of two fp32 values is exact in fp64"""
    return (a.double() * b.double() + c.double()).float()


# ----------------------------------------------------------------------------------------------------------------
# loss (util.py:13-24)
# ----------------------------------------------------------------------------------------------------------------
# (N, DHW, C, Cx, Lz); the last two lie past loss_partial's (262,144 voxels) and loss_bwd's (1,048,576) grid caps
LOSS_SHAPES_SMALL = [(2, (8, 8, 16), 3, 2, 8), (3, (4, 6, 10), 8, 1, 4), (2, (4, 6, 10), 1, 4, 4)]
LOSS_SHAPE_PAST_PARTIAL = (1, (64, 64, 72), 3, 2, 128)
LOSS_SHAPE_PAST_BWD = (1, (96, 96, 120), 3, 2, 8)
LOSS_SHAPES = LOSS_SHAPES_SMALL + [LOSS_SHAPE_PAST_PARTIAL, LOSS_SHAPE_PAST_BWD]


def loss_inputs(n, dims, c, cx, lz, seed=0):
    """p = fl32(sigmoid(logit)), logit ~ N(0, sd 2) so p reaches both tails; labels {0,1} at rate 0.3"""
    g = torch.Generator().manual_seed(1000 + seed)
    logits = torch.randn((n,) + tuple(dims) + (c,), generator=g, dtype=F32) * 2.0
    p = torch.sigmoid(logits.double()).float()
    y = (torch.rand((n,) + tuple(dims) + (c,), generator=g) < 0.3).float()
    x = torch.randn((n,) + tuple(dims) + (cx,), generator=g, dtype=F32)
    yv = torch.randn((n,) + tuple(dims) + (cx,), generator=g, dtype=F32)
    proj = torch.randn((n, 2 * lz), generator=g, dtype=F32) * 0.5
    return p, y, x, yv, proj


def loss_ref(p, y, x=None, yv=None, proj=None, gs=1.0, through_sigmoid=True):
    """fp64 oracle (R.dice_vae_loss + autograd) and the bounds.  x is None: no VAE terms."""
    c = p.shape[-1]
    gs = f32(gs)
    pd = p.double().requires_grad_(True)
    yd = y.double()
    has_vae = x is not None
    if has_vae:
        lz = proj.shape[1] // 2
        yvd = yv.double().requires_grad_(True)
        prd = proj.double().requires_grad_(True)
        loss = R.dice_vae_loss(x.double(), yd, pd, yvd, prd[:, :lz], prd[:, lz:])
    else:  # the oracle's VAE terms vanish on these: mean(0^2) = 0, 0^2 + exp(0) - 0 - 1 = 0
        z = torch.zeros(1, dtype=F64)
        loss = R.dice_vae_loss(z, yd, pd, z, z, z)
    loss.backward()
    axes = (0, 1, 2, 3)
    pv = pd.detach()
    I, P, T = (pv * yd).sum(axes), (pv * pv).sum(axes), (yd * yd).sum(axes)
    D = P + T + 1.0
    dice = float((1.0 - (2.0 * I + 1.0) / D).mean())
    k1 = -2.0 * gs / (c * D)
    k2 = 2.0 * gs * (2.0 * I + 1.0) / (c * D * D)
    dl = pd.grad * gs
    B = k1.abs() * yd + k2.abs() * pv
    if through_sigmoid:
        dl = dl * pv * (1.0 - pv)
        B = B * pv * (1.0 - pv)
    out = dict(loss=float(loss.detach()), dice=dice, l2=0.0, kl=0.0, dlogit=dl, B_dlogit=EPS32 * B, I=I, P=P, T=T,
               value_bound=4 * EPS32 * 1.0)
    if has_vae:
        xd = x.double()
        mu, lv = proj.double()[:, :lz], proj.double()[:, lz:]
        out['l2'] = float(((xd - yv.double()) ** 2).mean())
        out['kl'] = float((mu ** 2 + torch.exp(lv) - lv - 1.0).mean())
        out['sq'] = float(((xd - yv.double()) ** 2).sum())
        out['klsum'] = float((mu ** 2 + torch.exp(lv) - lv - 1.0).sum())
        out['klabs'] = float((mu ** 2 + torch.exp(lv) + lv.abs() + 1.0).sum())
        out['numel_x'], out['numel_z'] = float(x.numel()), float(mu.numel())
        out['value_bound'] = 4 * EPS32 * (1.0 + 0.1 * out['l2'] + 0.1 * float((mu ** 2 + torch.exp(lv) + lv.abs() + 1.0).mean()))
        out['dyvae'] = yvd.grad * gs
        out['B_dyvae'] = EPS32 * out['dyvae'].abs()
        out['dproj'] = prd.grad * gs
        Bp = out['dproj'].abs().clone()
        Bp[:, lz:] = 0.1 * gs / mu.numel() * (torch.exp(lv) + 1.0)
        out['B_dproj'] = EPS32 * Bp
    return out


def loss_sums_f32(p, y, x, yv, proj):
    """bts_loss_sums: every product rounds once to fp32, the sums run in fp64 -> (3C+4,) float64"""
    axes = (0, 1, 2, 3)
    parts = [(p * y).double().sum(axes), (p * p).double().sum(axes), (y * y).double().sum(axes)]
    if x is not None:
        m = torch.zeros(x.shape[:-1], dtype=F32)
        for c in range(x.shape[-1]):
            d = x[..., c] - yv[..., c]
            m = fma32(d, d, m)
        lz = proj.shape[1] // 2
        mu, lv = proj[:, :lz], proj[:, lz:]
        kl = (mu * mu + torch.exp(lv) - lv - 1.0).double().sum()
        tail = [m.double().sum(), kl, float(x.numel()), float(mu.numel())]
    else:
        tail = [0.0, 0.0, 0.0, 0.0]
    return torch.cat(parts + [torch.tensor([float(t) for t in tail], dtype=F64)])


def loss_value_f64(sums, c, has_vae):
    """bts_loss_value from the raw sums -> (loss, [dice, l2, kl]) as fp32-rounded floats"""
    d = float((1.0 - (2.0 * sums[:c] + 1.0) / (sums[c:2 * c] + sums[2 * c:3 * c] + 1.0)).sum()) / c
    l2 = float(sums[3 * c] / sums[3 * c + 2]) if has_vae else 0.0
    kl = float(sums[3 * c + 1] / sums[3 * c + 3]) if has_vae else 0.0
    return f32(d + 0.1 * l2 + 0.1 * kl), [f32(d), f32(l2), f32(kl)]


def loss_bwd_f32(p, y, x, yv, proj, sums, gs=1.0, through_sigmoid=True):
    """bts_loss_bwd as loss.hip:113-115 states it: k1, k2 in fp64 rounded to fp32, the rest in fp32"""
    c = p.shape[-1]
    gs64 = f32(gs)
    gs32 = torch.tensor(gs64, dtype=F32)
    D = sums[c:2 * c] + sums[2 * c:3 * c] + 1.0
    k1 = (-2.0 / (c * D) * gs64).float()
    k2 = (2.0 * (2.0 * sums[:c] + 1.0) / (c * D * D) * gs64).float()
    g = k1 * y + k2 * p
    if through_sigmoid:
        g = g * (p * (1.0 - p))
    if x is None:
        return g, None, None
    kx = torch.tensor(0.2 / float(sums[3 * c + 2]), dtype=F32) * gs32
    dyv = kx * (yv - x)
    kz = torch.tensor(1.0 / float(sums[3 * c + 3]), dtype=F32) * gs32
    lz = proj.shape[1] // 2
    dproj = torch.empty_like(proj)
    dproj[:, :lz] = (torch.tensor(0.2, dtype=F32) * kz) * proj[:, :lz]
    dproj[:, lz:] = (torch.tensor(0.1, dtype=F32) * kz) * (torch.exp(proj[:, lz:]) - 1.0)
    return g, dyv, dproj


# ----------------------------------------------------------------------------------------------------------------
# metric (util.py:35-57)
# ----------------------------------------------------------------------------------------------------------------
METRIC_SHAPES = [(2, (5, 6, 7), 3), (1, (4, 4, 4), 1), (1, (3, 5, 8), 8), (1, (64, 64, 72), 3)]


def metric_inputs(n, dims, c, seed=0):
    """predictions on the grid {0, .25, .5, .75, 1}, so ties, exact 0.5 maxima (masked out) and all-equal rows are frequent at
    C <= 3; the first voxels plant one of each for any C: an all-equal row above and one at the threshold, a maximum of exactly 0.5,
    a tie of the last two channels"""
    g = torch.Generator().manual_seed(2000 + seed)
    yp = torch.randint(0, 5, (n,) + tuple(dims) + (c,), generator=g).float() * 0.25
    flat = yp.view(-1, c)
    flat[0] = 0.75
    flat[1] = 0.5
    flat[2] = 0.25
    flat[2, -1] = 0.5
    flat[3] = 0.0
    flat[3, -2:] = 1.0
    yt = (torch.rand((n,) + tuple(dims) + (c,), generator=g) < 0.3).float()
    return yt, yp


def metric_ref(yt, yp, channels_last_axes):
    """R.dice_coefficient in the asked data format (channels_first: on the permuted tensor) -> macro, micro, labels, table.
    table[(cell*C + c)*3 + {I,P,T}] holds counts of 0/1 values: exact."""
    if channels_last_axes:
        macro, micro, labels = R.dice_coefficient(yt.double(), yp.double(), 'channels_last')
    else:
        macro, micro, labels = R.dice_coefficient(yt.double().permute(0, 4, 1, 2, 3), yp.double().permute(0, 4, 1, 2, 3),
                                                  'channels_first')
    c = yp.shape[-1]
    on = (labels > 0)
    oh = torch.zeros(yp.shape, dtype=F64)
    oh.scatter_(4, (labels.long() - 1).clamp(min=0).unsqueeze(-1), 1.0)
    oh = oh * on.unsqueeze(-1).double()
    ytd = yt.double()
    axes = (0, 1, 2) if channels_last_axes else (0, 1, 2, 3)
    tab = torch.stack([(oh * ytd).sum(axes), oh.sum(axes), ytd.sum(axes)], dim=-1)      # (W, C, 3) or (C, 3)
    return float(macro), float(micro), labels.to(torch.uint8), tab.reshape(-1)


# ----------------------------------------------------------------------------------------------------------------
# L2 regulariser (train.py:146)
# ----------------------------------------------------------------------------------------------------------------
def l2_ref(p, g, ranges, gs=1.0):
    """-> value, value bound, grad, grad bound unit (eps32 * B, B = |g| + 2 coef gs |p|); coef rounded to fp32"""
    gs = f32(gs)
    pd, gd = p.double(), g.double().clone()
    B = g.double().abs().clone()
    val, mag = 0.0, 0.0
    for off, ln, coef in ranges:
        cf = f32(coef)
        q = pd[off:off + ln]
        val += cf * float((q * q).sum())
        mag += abs(cf) * float((q * q).sum())
        gd[off:off + ln] += 2.0 * cf * gs * q
        B[off:off + ln] += 2.0 * abs(cf) * gs * q.abs()
    return val, EPS32 * abs(val) + 1e-12 * mag + TINY, gd, EPS32 * B


def l2_f32(p, g, ranges, gs=1.0):
    """squares round to fp32, sums in fp64, one rounding; grad = fma(2 coef gs, p, g)"""
    gs32 = torch.tensor(f32(gs), dtype=F32)
    val = 0.0
    g2 = g.clone()
    for off, ln, coef in ranges:
        q = p[off:off + ln]
        val += float(np.float32(coef)) * float((q * q).double().sum())
        k = torch.tensor(2.0, dtype=F32) * torch.tensor(coef, dtype=F32) * gs32
        g2[off:off + ln] = fma32(k.expand_as(q), q, g[off:off + ln])
    return f32(val), g2


# ----------------------------------------------------------------------------------------------------------------
# Adam (util.py:60-84; Keras form: epsilon outside the root, un-corrected)
# ----------------------------------------------------------------------------------------------------------------
def adam_grad(n, seed, gmul):
    """|g| log-uniform in [1e-12, 1e3], random sign, every 97th element exactly 0, divided by gmul"""
    g = torch.Generator().manual_seed(3000 + seed)
    mag = torch.exp(torch.rand(n, generator=g, dtype=F64) * (math.log(1e3) - math.log(1e-12)) + math.log(1e-12))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    out = mag * sign / f32(gmul)
    out[::97] = 0.0
    return out.float()


def adam_scalars(t, lr=1e-4, b1=0.9, b2=0.999, eps=1e-7):
    lr_t = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)      # host, fp64 (optim.hip:3)
    return f32(lr_t), f32(b1), f32(b2), f32(eps)


def adam_ref(p, g, m, v, lr_t, b1, b2, eps, gmul):
    """one step in fp64 from fp32 state, scalars as the ABI receives them -> (p, m, v), (Bp, Bm, Bv) bound units"""
    lr_t, b1, b2, eps, gmul = [f32(s) for s in (lr_t, b1, b2, eps, gmul)]
    p, g, m, v = [t.double() for t in (p, g, m, v)]
    ge = g * gmul
    m2 = b1 * m + (1.0 - b1) * ge
    v2 = b2 * v + (1.0 - b2) * ge * ge
    p2 = p - lr_t * m2 / (torch.sqrt(v2) + eps)
    Bm = b1 * m.abs() + (1.0 - b1) * ge.abs()
    Bp = p.abs() + lr_t * Bm / (torch.sqrt(v2) + eps)
    return (p2, m2, v2), (EPS32 * Bp, EPS32 * Bm, EPS32 * v2)


def adam_f32(p, g, m, v, lr_t, b1, b2, eps, gmul, eps_inside=False):
    """optim.hip:2 in fp32, in the kernel's order.  eps_inside: the WRONG form sqrt(v + eps), for the host test that shows the
    p0 = 0 case tells the two apart."""
    s = [torch.tensor(f32(t), dtype=F32) for t in (lr_t, b1, b2, eps, gmul)]
    lr_t, b1, b2, eps, gmul = s
    one = torch.tensor(1.0, dtype=F32)
    ge = g * gmul
    m2 = b1 * m + (one - b1) * ge
    v2 = b2 * v + (one - b2) * ge * ge
    den = torch.sqrt(v2 + eps) if eps_inside else torch.sqrt(v2) + eps
    return p - lr_t * m2 / den, m2, v2


# ----------------------------------------------------------------------------------------------------------------
# Dense (vae.py:61-64,105-109)
# ----------------------------------------------------------------------------------------------------------------
# (N, in, out, relu); the last lies past dense_bwd_w's grid cap of 2,097,152 weights, the first sits exactly on it
DENSE_SHAPES = [(1, 8192, 256, 0), (9, 1000, 257, 1), (8, 129, 1, 0), (3, 1, 5, 1), (2, 33000, 40, 0), (2, 8200, 257, 1)]


def dense_inputs(n, fin, fout, seed=0):
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn((n, fin), generator=g, dtype=F32)
    w = torch.randn((fin, fout), generator=g, dtype=F32) * 0.1
    b = torch.randn((fout,), generator=g, dtype=F32)
    dy = torch.randn((n, fout), generator=g, dtype=F32)
    return x, w, b, dy


def dense_fwd_ref(x, w, b, relu):
    y = x.double() @ w.double()
    B = x.double().abs() @ w.double().abs()
    if b is not None:
        y = y + b.double()
        B = B + b.double().abs()
    return (torch.relu(y) if relu else y), EPS32 * B


def dense_bwd_ref(x, w, g, old_dx=None, old_dw=None, old_db=None):
    """g = dy through the activation's derivative.  old_*: the destination's contents when the call accumulates."""
    xd, wd, gd = x.double(), w.double(), g.double()
    dx, Bx = gd @ wd.t(), gd.abs() @ wd.abs().t()
    dw, Bw = xd.t() @ gd, xd.abs().t() @ gd.abs()
    db, Bb = gd.sum(0), gd.abs().sum(0)
    if old_dx is not None:
        dx, Bx = dx + old_dx.double(), Bx + old_dx.double().abs()
    if old_dw is not None:
        dw, Bw = dw + old_dw.double(), Bw + old_dw.double().abs()
    if old_db is not None:
        db, Bb = db + old_db.double(), Bb + old_db.double().abs()
    return (dx, dw, db), (EPS32 * Bx, EPS32 * Bw, EPS32 * Bb)


def dense_chunks(fin):
    chunks = min((fin + 127) // 128, 128)
    rpc = (fin + chunks - 1) // chunks
    return (fin + rpc - 1) // rpc, rpc


def dense_fwd_f32(x, w, b, relu):
    """dense.hip:3-4: the input rows split into chunks, an fma chain down each chunk, the chunks added in order, then the bias"""
    n, fin = x.shape
    fout = w.shape[1]
    chunks, rpc = dense_chunks(fin)
    pad = chunks * rpc - fin
    xp = torch.cat([x, torch.zeros((n, pad), dtype=F32)], 1).reshape(n, chunks, rpc)
    wp = torch.cat([w, torch.zeros((pad, fout), dtype=F32)], 0).reshape(chunks, rpc, fout)
    acc = torch.zeros((chunks, n, fout), dtype=F32)
    for k in range(rpc):
        acc = fma32(xp[:, :, k].t().unsqueeze(-1), wp[:, k, :].unsqueeze(1), acc)
    s = torch.zeros((n, fout), dtype=F32)
    for ch in range(chunks):
        s = s + acc[ch]
    if b is not None:
        s = s + b
    return torch.relu(s) if relu else s


def dense_bwd_f32(x, w, g):
    """dW: an fma chain over the samples; db: a plain sum over the samples; dx: 64 lanes stride the outputs with an fma chain
    each, then a halving tree over the lanes (dense.hip:85-114)"""
    n, fin = x.shape
    fout = w.shape[1]
    dw = torch.zeros((fin, fout), dtype=F32)
    db = torch.zeros((fout,), dtype=F32)
    for i in range(n):
        dw = fma32(x[i].unsqueeze(1), g[i].unsqueeze(0), dw)
        db = db + g[i]
    steps = (fout + 63) // 64
    pad = steps * 64 - fout
    wp = torch.cat([w, torch.zeros((fin, pad), dtype=F32)], 1).reshape(fin, steps, 64)
    gp = torch.cat([g, torch.zeros((n, pad), dtype=F32)], 1).reshape(n, steps, 64)
    acc = torch.zeros((n, fin, 64), dtype=F32)
    for s in range(steps):
        acc = fma32(wp[:, s, :].unsqueeze(0), gp[:, s, :].unsqueeze(1), acc)
    h = 32
    while h >= 1:
        acc = acc[..., :h] + acc[..., h:2 * h]
        h //= 2
    return acc[..., 0], dw, db


# ----------------------------------------------------------------------------------------------------------------
# column sums (se.hip) and channel moments (augment.hip): fp64 accumulation, one rounding
# ----------------------------------------------------------------------------------------------------------------
def colsum_ref(x, scale, sum_over_n, old=None):
    """x (N, rows, C) -> out (N, C) or (C,), bound (absolute).  old: the destination's contents when the call accumulates."""
    scale = f32(scale)
    xd = x.double()
    axes = (0, 1) if sum_over_n else (1,)
    v = scale * xd.sum(axes)
    bound = EPS32 * v.abs() + 1e-12 * abs(scale) * xd.abs().sum(axes) + TINY
    if old is not None:
        bound = bound + EPS32 * (old.double().abs() + v.abs())
        v = v + old.double()
    return v, bound


def colsum_f32(x, scale, sum_over_n, old=None):
    axes = (0, 1) if sum_over_n else (1,)
    v = (x.double().sum(axes) * f32(scale)).float()
    return v if old is None else old + v


def moments_ref(x):
    """x (nvox, C) -> mean, var (population), bounds (absolute)"""
    xd = x.double()
    mean = xd.mean(0)
    ex2 = (xd * xd).mean(0)
    var = ((xd - mean) ** 2).mean(0)        # two passes: no cancellation in the reference
    return mean, var, EPS32 * mean.abs() + 1e-12 * xd.abs().mean(0) + TINY, EPS32 * var + 1e-12 * (ex2 + mean * mean) + TINY


def moments_f32(x):
    """augment.hip: E[d^2] - E[d]^2 of d = x - (the first voxel's value) in fp64, clamped at 0, one rounding"""
    xd = x.double()
    d = xd - xd[0]
    m = d.sum(0) / x.shape[0]
    var = ((d * d).sum(0) / x.shape[0] - m * m).clamp(min=0.0)
    return (xd[0] + m).float(), var.float()


# ----------------------------------------------------------------------------------------------------------------
# element-wise kernels (pointwise.hip): K = 4, B = the sum of the absolute terms
# ----------------------------------------------------------------------------------------------------------------
def axpy_ref(y, x, a):
    a = f32(a)
    return y.double() + a * x.double(), EPS32 * (y.double().abs() + abs(a) * x.double().abs())


def axpy_f32(y, x, a):
    return fma32(torch.tensor(f32(a), dtype=F32).expand_as(x), x, y)


def sigmoid_bwd_ref(y, dy):
    r = dy.double() * y.double() * (1.0 - y.double())
    return r, EPS32 * r.abs()


def sigmoid_bwd_f32(y, dy):
    return dy * y * (1.0 - y)


def dropout_apply_ref(x, mask, rate):
    r = R.dropout(x.double(), mask.double(), f32(rate))
    return r, EPS32 * r.abs()


def dropout_apply_f32(x, mask, rate):
    one = torch.tensor(1.0, dtype=F32)
    scale = one / (one - torch.tensor(f32(rate), dtype=F32))
    return torch.where(mask != 0, x * scale, torch.zeros_like(x))


def lincomb_ref(a, b, ca, cb):
    ca, cb = f32(ca), f32(cb)
    r = ca * a.double() + (cb * b.double() if b is not None else 0.0)
    B = abs(ca) * a.double().abs() + (abs(cb) * b.double().abs() if b is not None else 0.0)
    return r, EPS32 * B


def lincomb_f32(a, b, ca, cb):
    r = torch.tensor(f32(ca), dtype=F32) * a
    return r + torch.tensor(f32(cb), dtype=F32) * b if b is not None else r


def vae_sample_ref(proj, eps, dz, old_dproj):
    """-> z, dproj (= old + gradient: bts_vae_sample_bwd ADDS into dproj), bound units"""
    lz = proj.shape[1] // 2
    pd = proj.double().requires_grad_(True)
    z = R.sample(pd[:, :lz], pd[:, lz:], eps.double())
    z.backward(dz.double())
    s = torch.exp(0.5 * proj.double()[:, lz:]) * eps.double()
    Bz = proj.double()[:, :lz].abs() + s.abs()
    dproj = old_dproj.double() + pd.grad
    Bd = old_dproj.double().abs() + pd.grad.abs()
    return z.detach(), EPS32 * Bz, dproj, EPS32 * Bd


def vae_sample_f32(proj, eps, dz, old_dproj):
    lz = proj.shape[1] // 2
    h = torch.tensor(0.5, dtype=F32)
    z = proj[:, :lz] + torch.exp(h * proj[:, lz:]) * eps
    d = old_dproj.clone()
    d[:, :lz] += dz
    d[:, lz:] += dz * h * torch.exp(h * proj[:, lz:]) * eps
    return z, d


# ----------------------------------------------------------------------------------------------------------------
# the counter-based generator (common.h: mix32, u01; pointwise.hip: normal_kernel) -- integer part exact
# ----------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def mix32(z):
    """splitmix64 finaliser on a uint64 array -> the high 32 bits"""
    with np.errstate(over='ignore'):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def u01(seed, i):
    """[0, 1) with 24 bits, as a float32 array (exact); i: uint64 array of counters"""
    base = np.uint64((int(seed) * 0xD1342543DE82EF95) & _M64)
    with np.errstate(over='ignore'):
        z = base + i.astype(np.uint64)
    return (mix32(z) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def dropout_mask_np(n, rate, seed):
    return (u01(seed, np.arange(n, dtype=np.uint64)) >= np.float32(rate)).astype(np.uint8)


def normal_uniforms(n, seed):
    i = np.arange(n, dtype=np.uint64)
    u1 = np.maximum(u01(seed, np.uint64(2) * i), np.float32(5.9604645e-8))
    u2 = u01(seed, np.uint64(2) * i + np.uint64(1))
    return u1, u2


TWO_PI_F32 = float(np.float32(6.28318530718))
NORMAL_MAX = 5.77       # sqrt(-2 ln 2^-24) = 5.768


def normal_ref(n, seed):
    """Box-Muller in fp64 on the kernel's own (u1, u2), with the kernel's fp32 2*pi -> value, bound unit eps32 * sqrt(-2 ln u1)"""
    u1, u2 = normal_uniforms(n, seed)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return r * np.cos(TWO_PI_F32 * u2.astype(np.float64)), EPS32 * r


def normal_f32(n, seed):
    u1, u2 = normal_uniforms(n, seed)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.28318530718) * u2)
