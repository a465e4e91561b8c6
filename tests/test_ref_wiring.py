"""CPU: the REFERENCE's own Python (model.py, layers/*.py, util.py) against oracle/torch_ref.py (round-3 verdict, item 8), through what
it computed when imported over the `tensorflow` stand-in of oracle/tf_standin: tests/golden/ref_wiring_*.npz, recorded by
tests/golden/make_ref_wiring.py from a checkout of the reference (see its header).

What this checks: the restatement's WIRING -- block / level / concat order (encoder.py:69-101 incl. the duplicated dense concat,
decoder.py:65-83, vae.py:114-143), the GroupNormalization reshape sequence as written (group_norm.py:83-124: the channels_last
"slab" semantics SURVEY F1 claims), the loss and the metric with their axes (util.py:13-24,35-57), which variables carry an L2
regulariser (sum(model.losses), train.py:146), the Keras tracking order of the variables that `Model.get_weights()` of the product
promises (vae.unproj last), the learning-rate schedule and one Adam step.  What it does NOT check: TensorFlow's arithmetic -- the
stand-in's primitives are this repository's reading of it (conv / transposed-conv literally the oracle's).  Parity stays UNPINNED.

The recorded gradients are kept as three seeded projections and the largest magnitude per variable (the full tensors would not be
small): a gradient within 1e-9 of the reference's elementwise meets both, so the bounds below are necessary conditions of that one.
The checks execute in a CHILD interpreter (minimal environment, read-only scratch working directory) started by
test_reference_wiring_in_a_child_process, so that they see nothing but the repository; in the parent they are skipped."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
IN_CHILD = os.environ.get('BTS_REF_WIRING_CHILD') == '1'
child_only = pytest.mark.skipif(not IN_CHILD, reason='runs in the child process of test_reference_wiring_in_a_child_process')


@pytest.mark.skipif(IN_CHILD, reason='this IS the child')
def test_reference_wiring_in_a_child_process():
    import stat
    import subprocess
    import tempfile
    scratch = tempfile.mkdtemp(prefix='bts_refwiring_')
    os.chmod(scratch, stat.S_IRUSR | stat.S_IXUSR)
    try:
        env = {'PATH': '/usr/bin:/bin', 'HOME': scratch, 'BTS_REF_WIRING_CHILD': '1', 'PYTHONDONTWRITEBYTECODE': '1', 'PYTHONPATH': ROOT,
               'LD_LIBRARY_PATH': os.environ.get('LD_LIBRARY_PATH', '')}
        out = subprocess.run([sys.executable, '-m', 'pytest', '-x', '-q', '-p', 'no:cacheprovider', '--rootdir', os.path.join(ROOT, 'tests'),
                              os.path.abspath(__file__)], cwd=scratch, env=env, capture_output=True, text=True, timeout=900)
        tail = (out.stdout + out.stderr)[-3000:]
        assert out.returncode == 0, tail
        assert '5 passed, 1 skipped' in out.stdout, tail      # (4 wiring cases + schedule/Adam; the skip is this launcher itself)
    finally:
        os.chmod(scratch, stat.S_IRWXU)
        os.rmdir(scratch)


CASES = [
    dict(base_filters=4, groups=2, reduction=2, depth=2),                                         # SURVEY 8c "micro"
    dict(base_filters=8, groups=4, reduction=2, depth=3),                                         # dense concat of three blocks
    dict(base_filters=8, groups=4, reduction=2, depth=3, data_format='channels_first'),           # true channel groups, per-class Dice
    dict(base_filters=8, groups=4, reduction=2, depth=3, downsampling='max', upsampling='linear'),
]
N_PROJ = 3


def case_id(kw):
    return '-'.join('%s' % v for v in kw.values())


def fixture_path(kw):
    return os.path.join(GOLDEN, 'ref_wiring_%s.npz' % case_id(kw).replace('_', ''))


def case_inputs(kw):
    """the volume, labels, dropout mask and eps of one case (channels_first: permuted to NCDHW), fp64"""
    from oracle import torch_ref as R
    cfg = R.default_config(**kw)
    crop = (8, 8, 8) if cfg['depth'] == 2 else (16, 16, 16)
    latent = cfg['base_filters'] * 2 ** (cfg['depth'] - 2)
    x, y, mask, eps = R.synthetic_batch(2, crop, latent=latent, seed=21, dtype=torch.float64)
    if cfg['data_format'] == 'channels_first':
        x, y, mask = (t.permute(0, 4, 1, 2, 3).contiguous() for t in (x, y, mask))
    return cfg, crop, x, y, mask, eps


def draw_values(names, shapes):
    """the value of every variable, in tracking order: gamma ~ 1 + N(0, 0.25), beta ~ N(0, 0.25) (gamma_2 = 0 at init would hide every
    block's conv branch), kernels ~ N(0, 1 / fan_in), biases ~ N(0, 0.01)"""
    g = torch.Generator().manual_seed(5)
    out = []
    for name, shape in zip(names, shapes):
        t = torch.randn(tuple(shape), dtype=torch.float64, generator=g)
        if name == 'gamma':
            t = t * 0.5 + 1.0
        elif name == 'beta':
            t = t * 0.5
        elif len(shape) >= 2:
            t = t / float(np.prod(shape[:-1])) ** 0.5
        else:
            t = t * 0.1
        out.append(t)
    return out


def projections(i, numel):
    """the N_PROJ fixed vectors the gradient of variable i is projected on"""
    g = torch.Generator().manual_seed(1000 + i)
    return torch.randn((N_PROJ, numel), dtype=torch.float64, generator=g)


def load_case(kw):
    z = np.load(fixture_path(kw))
    nd = z['var_ndim']
    flat = list(z['var_shape_flat'])
    shapes, k = [], 0
    for n in nd:
        shapes.append(tuple(int(v) for v in flat[k:k + n]))
        k += n
    return z, [str(s) for s in z['var_names']], shapes


@child_only
@pytest.mark.parametrize('kw', CASES, ids=case_id)
def test_reference_python_on_the_standin_equals_the_oracle(kw):
    import bts_amd  # noqa: F401
    from bts_amd.model import Model as ProductModel
    from oracle import torch_ref as R
    z, rnames, rshapes = load_case(kw)
    cfg, crop, x, y, mask, eps = case_inputs(kw)
    n = x.shape[0]
    rvals = draw_values(rnames, rshapes)
    # ---- variable order: what the product promises for Model.get_weights() (Keras tracking order) ----
    pm = ProductModel(**kw)
    pm.build((n,) + crop + (2,))        # (the engine's memory is NDHWC whatever the public layout)
    pvars = pm.trainable_variables
    assert len(pvars) == len(rshapes), (len(pvars), len(rshapes))
    P = R.ParamSet()
    ref_l2 = R.build_params(cfg, crop, seed=0).l2
    for pv, shape, val in zip(pvars, rshapes, rvals):
        assert tuple(pv.t.shape) == shape, (pv.name, tuple(pv.t.shape), shape)
        P[pm.oracle_name(pv)] = val.clone()
    P.l2.update(ref_l2)
    assert set(P) == set(ref_l2), set(P) ^ set(ref_l2)
    last = [pm.oracle_name(v) for v in pvars[-2:]]
    assert last == ['vae/unproj_k', 'vae/unproj_b'], last            # vae.py:105: created in build(), tracked last
    # ---- forward, training mode, identical draws ----
    yp_o, yv_o, zm_o, zl_o = R.model(x, P, cfg, training=True, inference=False, mask=mask, eps=eps)
    for b, name in ((yp_o, 'y_pred'), (yv_o, 'y_vae'), (zm_o, 'z_mean'), (zl_o, 'z_logvar')):
        a = torch.from_numpy(z[name])
        assert tuple(a.shape) == tuple(b.shape), name
        b = b.detach()
        assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), (name, float((a - b).abs().max()))
    # ---- loss (util.py:13-24), regularisers (train.py:146), metric (util.py:35-57) ----
    df = cfg['data_format']
    loss_r, reg_r, mac_r, mic_r = (float(z[k]) for k in ('loss', 'reg', 'macro', 'micro'))
    loss_o = float(R.dice_vae_loss(x, y, yp_o, yv_o, zm_o, zl_o, data_format=df).detach())
    reg_o = float(R.l2_regularisation(P).detach())
    assert abs(loss_r - loss_o) <= 1e-12 * max(1.0, abs(loss_o))
    assert abs(reg_r - reg_o) <= 1e-12 * max(1e-6, abs(reg_o)), (reg_r, reg_o)
    mac_o, mic_o, _ = R.dice_coefficient(y, yp_o.detach(), data_format=df)
    assert abs(mac_r - float(mac_o)) <= 1e-12 and abs(mic_r - float(mic_o)) <= 1e-12
    # ---- gradients of the reference's graph (torch autograd through the stand-in) against the oracle's ----
    leaves = R.ParamSet()
    leaves.update({k: v.clone().requires_grad_(True) for k, v in P.items()})
    leaves.l2 = P.l2
    out = R.model(x, leaves, cfg, training=True, inference=False, mask=mask, eps=eps)
    g_o = torch.autograd.grad(R.dice_vae_loss(x, y, *out, data_format=df) + R.l2_regularisation(leaves), [leaves[pm.oracle_name(v)] for v in pvars])
    for i, (pv, b) in enumerate(zip(pvars, g_o)):
        # (floor 1e-15: a gradient that is zero in exact arithmetic -- a bias ahead of a GroupNorm -- is left with ~1e-17 of
        # rounding, which differs between the machine that recorded the file and this one)
        tol = 1e-9 * max(1e-6, float(b.abs().max()))
        r = projections(i, b.numel())
        assert np.all(np.abs(z['grad_proj'][i] - (r @ b.reshape(-1)).numpy()) <= tol * r.abs().sum(dim=1).numpy()), pv.name
        assert abs(float(z['grad_absmax'][i]) - float(b.abs().max())) <= tol, pv.name
    # ---- inference mode: VAE branch skipped (model.py:63-68) ----
    assert bool(z['inference_vae_outputs_none'])
    yp_inf = R.model(x, P, cfg, training=False, inference=True)[0]
    assert float((torch.from_numpy(z['y_pred_inference']) - yp_inf.detach()).abs().max()) <= 1e-10
    assert bool(z['training_and_inference_raises'])


@child_only
def test_reference_schedule_and_adam_step_equal_the_oracle():
    """util.py:60-84: ScheduledOptim.__call__(epoch) and one apply_gradients against oracle.scheduled_lr / adam_tf_step"""
    from oracle import torch_ref as R
    z = np.load(os.path.join(GOLDEN, 'ref_wiring_adam.npz'))
    for epoch, lr_r in zip(z['epochs'], z['lr']):
        assert abs(float(lr_r) - R.scheduled_lr(1e-4, int(epoch))) <= 1e-18
    g = torch.Generator().manual_seed(3)
    w = torch.randn(50, dtype=torch.float64, generator=g)
    gr = torch.randn(50, dtype=torch.float64, generator=g) * torch.logspace(-8, 0, 50, dtype=torch.float64)
    p, m, v = w.clone(), torch.zeros(50, dtype=torch.float64), torch.zeros(50, dtype=torch.float64)
    lr = R.scheduled_lr(1e-4, 3)
    for t in (1, 2, 3):
        p, m, v = R.adam_tf_step(p, gr, m, v, t, lr)
        assert float((torch.from_numpy(z['w_after'][t - 1]) - p).abs().max()) <= 1e-15
