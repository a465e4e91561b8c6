"""-m gpu: the BASELINE shapes themselves (configs[1]: 2ch x 128^3 train step, CLI-default model; configs[4]'s padded
160x192x160 inference grid).  The fp64 oracle cannot run a 128^3 step in test time (the CLI model at 64^3 IS compared with
it: tests/test_model_gpu.py::test_train_step_parity[cli_64]), so full size is covered through size-independent properties:

  * form agreement: at 128^3 the dispatcher picks conv forms the small-grid oracle tests only reach by forcing thresholds
    (upm / k1s / dsc / c2 kernels, unsplit Winograd, the Winograd weight gradient, the streaming 1x1x1 weight gradient).
    One full step with the DEFAULT forms must agree with one step where every conv and weight gradient runs in DIRECT form
    (BTS_WINO=0 BTS_WGW=0 BTS_K1W=0) -- two independent kernel families.  The direct convs are the tiled kernel, every config
    and form of which that a layer runs with BTS_WINO=0 is held to the fp64 oracle by tests/test_tiled_configs_gpu.py (the
    table tests/tiled_cases.py, kept complete by tests/test_tiled_configs_host.py); the direct weight gradients by
    tests/test_wgrad_plan_gpu.py;
  * determinism: two default-form steps from the same state end bitwise identical (no float atomics, fixed-order reductions).

Tolerances: loss <= 1e-5 relative, Dice <= 1e-4, y_pred max-abs <= 1e-4, label map identical outside counted
near-ties (|p-0.5| < 1e-5 or top-2 gap < 1e-5), every variable's gradient <= 1e-3 of that gradient's max-abs -- or 4x
what a one-ulp change of the input volume does to the direct form's own gradient of that variable (two such changes, the
larger effect), or 2x the largest such effect over all variables, when those are larger: the same "may deviate as much as an
equally valid fp32 evaluation does" rule tests/test_model_gpu.py applies with torch-fp32.  scripts/grad_conditioning.py shows
why it is needed: at 64^3 torch-fp32 itself is off by > 1e-3 of max-abs on 22 of the 260 variables (worst 7e-3), the engine's
default forms on 9 (worst 5e-3) and its direct forms on 22 (worst 2e-2) -- deep-level gradients are sums over every voxel
with heavy cancellation, and which ReLUs sit within rounding of zero differs between any two evaluation orders.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

FORM_SWITCHES = ('BTS_WINO', 'BTS_WGW', 'BTS_K1W')
GRAD_TOL = 1e-3
CLI = dict(base_filters=32, reduction=8, depth=4, groups=8)


def _randomise_affine(model, seed):
    """gamma_2 = 0 at init would hide conv1 / conv2 / GN of every block"""
    from bts_amd.tape import bump_weights_epoch
    g = torch.Generator().manual_seed(seed)
    for p in model.trainable_variables:
        if p.name.endswith('gamma'):
            p.t.copy_((1.0 + 0.3 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
        elif p.name.endswith('beta') or p.t.dim() == 1:
            p.t.copy_((0.1 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
    bump_weights_epoch()


def _one_step(direct, x, y, mask, eps):
    """fresh CLI model from a fixed seed, one full train step; returns everything comparable"""
    from bts_amd.layers import _base
    from bts_amd.model import Model
    from bts_amd.util import DiceCoefficient, DiceVAELoss, ScheduledOptim, train_step
    saved = {k: os.environ.get(k) for k in FORM_SWITCHES}
    try:
        for k in FORM_SWITCHES:
            if direct:
                os.environ[k] = '0'
            else:
                os.environ.pop(k, None)
        _base.set_seed(1234)
        model = Model(**CLI)
        model.build((x.shape[0],) + tuple(x.shape[1:4]) + (2,))
        _randomise_affine(model, 99)
        model.encoder.set_dropout_mask(mask)
        model.vae.set_eps(eps)
        opt = ScheduledOptim(1e-4)
        opt(epoch=0)
        lf, df = DiceVAELoss(), DiceCoefficient()
        from bts_amd.tape import GradientTape
        from bts_amd.util import reduce_sum
        with GradientTape() as tape:
            y_pred, y_vae, z_mean, z_logvar = model(x, training=True, inference=False)
            loss = lf(x, y, y_pred, y_vae, z_mean, z_logvar)
            loss = loss + reduce_sum(model.losses)
        macro, micro = df(y, y_pred)
        grads = tape.gradient(loss, model.trainable_variables)
        out = {'loss': float(loss), 'macro': float(macro), 'micro': float(micro), 'y_pred': y_pred.t.clone(),
               'y_vae': y_vae.t.clone(), 'labels': df.last_labels.clone(), 'grads': model.flat_grads.clone(),
               'spans': [(p.name, (p._gview.data_ptr() - model.flat_grads.data_ptr()) // 4, p._gview.numel())
                         for p in model.trainable_variables]}
        opt.apply_gradients(zip(grads, model.trainable_variables), model=model)
        torch.cuda.synchronize()
        out['params'] = model.flat_params.clone()
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_full_size_train_step_forms_agree_and_are_deterministic():
    import bts_amd  # noqa: F401
    from bts_amd.data import synthetic_batch
    dev = torch.device('cuda', 0)
    x, y, mask, eps = synthetic_batch(1, (128, 128, 128), latent=128, seed=1234)
    x, y = x.to(dev), y.to(dev)
    a = _one_step(False, x, y, mask, eps)
    b = _one_step(False, x, y, mask, eps)
    # determinism of the product forms: bitwise
    assert a['loss'] == b['loss'] and torch.equal(a['y_pred'], b['y_pred']) and torch.equal(a['labels'], b['labels'])
    assert torch.equal(a['grads'], b['grads']) and torch.equal(a['params'], b['params'])
    del b
    d = _one_step(True, x, y, mask, eps)
    assert abs(a['loss'] - d['loss']) <= 1e-5 * max(1.0, abs(d['loss'])), (a['loss'], d['loss'])
    assert abs(a['macro'] - d['macro']) <= 1e-4 and abs(a['micro'] - d['micro']) <= 1e-4
    e = float((a['y_pred'] - d['y_pred']).abs().max())
    ev = float((a['y_vae'] - d['y_vae']).abs().max())
    print('128^3: loss %.7f / %.7f, y_pred max |d| %.2e, y_vae max |d| %.2e (|y_vae| max %.2f)' %
          (a['loss'], d['loss'], e, ev, float(d['y_vae'].abs().max())))
    assert e <= 1e-4 and ev <= 1e-4 * max(1.0, float(d['y_vae'].abs().max()))
    yp = d['y_pred']
    top2 = yp.topk(2, dim=-1).values
    amb = ((yp.max(dim=-1).values - 0.5).abs() < 1e-5) | ((top2[..., 0] - top2[..., 1]).abs() < 1e-5)
    n_amb = int(amb.sum())
    print('near-threshold voxels: %d of %d' % (n_amb, amb.numel()))
    assert n_amb <= 1e-3 * amb.numel()
    assert torch.equal(a['labels'][~amb], d['labels'][~amb]), 'argmax label map differs between the conv forms'
    # conditioning yardstick at THIS size (the fp64 oracle cannot provide one): the direct form again on an input moved by
    # one unit in the last place.  Billions of ReLU pre-activations and 1233 near-threshold outputs make the 128^3 gradient
    # of a randomly initialised network far more sensitive than the 16^3..64^3 cases the oracle tests bound with 1e-3.
    qs = [_one_step(True, x * f, y, mask, eps)['grads'] for f in (1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24)]
    errs, sens = [], {}
    for name, off, n in a['spans']:
        ga, gd = a['grads'][off:off + n], d['grads'][off:off + n]
        scale = float(gd.abs().max()) + 1e-30
        sens[name] = max(float((gq[off:off + n] - gd).abs().max()) for gq in qs) / scale
        errs.append((float((ga - gd).abs().max()) / scale, name, scale))
    gsens = max(sens.values())
    l2 = float((a['grads'] - d['grads']).norm() / d['grads'].norm())
    l2q = max(float((gq - d['grads']).norm() / d['grads'].norm()) for gq in qs)
    print('whole flat gradient, relative L2: forms %.3e ; 1-ulp input change %.3e' % (l2, l2q))
    assert l2 <= max(1e-4, 4.0 * l2q)
    errs.sort(reverse=True)
    for e_, name, scale in errs[:12]:
        print('gradient %-34s forms differ by %.3e of its max-abs %.3e (1-ulp input sensitivity %.3e)' %
              (name, e_, scale, sens[name]))
    print('largest 1-ulp sensitivity over all variables: %.3e' % gsens)
    assert errs[0][0] > 0.0, 'both runs took the same kernels: the switches did nothing'
    for e_, name, scale in errs:
        assert e_ <= max(GRAD_TOL, 4.0 * sens[name], 2.0 * gsens), (name, e_, sens[name], gsens)


def test_full_volume_inference_forms_agree():
    """configs[4] grid: 155x190x147 padded to 160x192x160 (test.py:164-178), inference=True skips the VAE (model.py:67-68)"""
    import bts_amd  # noqa: F401
    from bts_amd.layers import _base
    from bts_amd.model import Model
    dev = torch.device('cuda', 0)
    g = torch.Generator().manual_seed(4)
    x = torch.randn((1, 160, 192, 160, 2), generator=g)
    x[:, 155:] = 0
    x[:, :, 190:] = 0
    x[:, :, :, 147:] = 0
    x = x.to(dev)
    outs = []
    for direct in (False, True):
        saved = os.environ.get('BTS_WINO')
        try:
            if direct:
                os.environ['BTS_WINO'] = '0'
            else:
                os.environ.pop('BTS_WINO', None)
            _base.set_seed(77)
            model = Model(**CLI)
            model.build((1, 128, 128, 128, 2))      # weights belong to the training crop (the VAE is tied to it)
            _randomise_affine(model, 5)
            y_pred, a, b, c = model(x, training=False, inference=True)
            assert a is None and b is None and c is None and y_pred.shape == (1, 160, 192, 160, 3)
            torch.cuda.synchronize()
            outs.append(y_pred.t.clone())
        finally:
            if saved is None:
                os.environ.pop('BTS_WINO', None)
            else:
                os.environ['BTS_WINO'] = saved
    e = float((outs[0] - outs[1]).abs().max())
    print('160x192x160 inference: y_pred max |default - direct| %.2e' % e)
    assert 0.0 < e <= 1e-4
    top2 = outs[1].topk(2, dim=-1).values
    amb = ((outs[1].max(dim=-1).values - 0.5).abs() < 1e-5) | ((top2[..., 0] - top2[..., 1]).abs() < 1e-5)
    assert int(amb.sum()) <= 1e-3 * amb.numel()
    assert torch.equal(outs[0].argmax(-1)[~amb], outs[1].argmax(-1)[~amb])
    assert torch.equal((outs[0].max(-1).values > 0.5)[~amb], (outs[1].max(-1).values > 0.5)[~amb])
