#!/usr/bin/env python3
"""Records tests/golden/ref_wiring_*.npz for tests/test_ref_wiring.py (run from the repository root:
python tests/golden/make_ref_wiring.py <checkout of the reference>).

The reference's model.py, layers/*.py and util.py need TensorFlow; they are imported here over the stand-in of oracle/tf_standin
(which refuses to stand in where a real tensorflow is importable), given the variable values of test_ref_wiring.draw_values and the
inputs of test_ref_wiring.case_inputs, and what they compute is written out: the variables' stand-in names and shapes in tracking
order, the four training-mode outputs, loss, regulariser, Dice, per-variable gradient projections and largest magnitudes, the
inference-mode output, and the learning-rate schedule / Adam steps of util.ScheduledOptim.  Nothing of the reference's program text
is recorded.  Run the result in a fresh interpreter: the reference's modules are imported into this one."""
import importlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.dirname(os.path.abspath(__file__))


def _test_module():
    spec = importlib.util.spec_from_file_location('ref_wiring_test', os.path.join(ROOT, 'tests', 'test_ref_wiring.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(ref_dir):
    ref_dir = os.path.abspath(ref_dir)
    T = _test_module()
    sys.path.insert(0, os.path.join(ROOT, 'oracle', 'tf_standin'))
    sys.path.insert(0, ref_dir)
    tf = importlib.import_module('tensorflow')
    assert 'STAND-IN' in (tf.__doc__ or ''), 'a real tensorflow is importable: the stand-in is for images without one'
    model, util = importlib.import_module('model'), importlib.import_module('util')
    assert model.__file__.startswith(ref_dir) and util.__file__.startswith(ref_dir)
    for kw in T.CASES:
        cfg, crop, x, y, mask, eps = T.case_inputs(kw)
        tf.INJECT['gen'].manual_seed(5)
        tf.INJECT['dropout_mask'] = tf.INJECT['eps'] = None
        rm = model.Model(**kw)
        rm(torch.zeros_like(x))                      # built the way train.py:94-96 does: one call on zeros
        rvars = rm.trainable_variables
        names = [w._standin['name'] for w in rvars]
        shapes = [tuple(w.shape) for w in rvars]
        with torch.no_grad():
            for w, v in zip(rvars, T.draw_values(names, shapes)):
                w.copy_(v)
        tf.INJECT['dropout_mask'], tf.INJECT['eps'] = mask, eps
        yp, yv, zm, zl = rm(x, training=True, inference=False)
        df = cfg['data_format']
        loss = util.DiceVAELoss(data_format=df)(x, y, yp, yv, zm, zl)
        reg = sum(rm.losses)
        mac, mic = util.DiceCoefficient(data_format=df)(y, yp.detach())
        grads = torch.autograd.grad(loss + reg, rvars)
        proj = np.stack([(T.projections(i, g.numel()) @ g.reshape(-1)).numpy() for i, g in enumerate(grads)])
        absmax = np.array([float(g.abs().max()) for g in grads])
        inf = rm(x, training=False, inference=True)
        try:
            rm(x, training=True, inference=True)
            raises = False
        except AssertionError:
            raises = True
        np.savez_compressed(T.fixture_path(kw), var_names=np.array(names), var_ndim=np.array([len(s) for s in shapes]),
                            var_shape_flat=np.array([d for s in shapes for d in s]),
                            y_pred=yp.detach().numpy(), y_vae=yv.detach().numpy(), z_mean=zm.detach().numpy(), z_logvar=zl.detach().numpy(),
                            loss=float(loss.detach()), reg=float(reg.detach()), macro=float(mac), micro=float(mic),
                            grad_proj=proj, grad_absmax=absmax,
                            y_pred_inference=inf[0].detach().numpy(),
                            inference_vae_outputs_none=all(o is None for o in inf[1:]), training_and_inference_raises=raises)
        print('wrote', os.path.relpath(T.fixture_path(kw), ROOT))
    # util.py:60-84: the schedule at four epochs and three apply_gradients steps
    opt = util.ScheduledOptim(learning_rate=1e-4)
    epochs = [0, 1, 150, 299]
    lrs = []
    for epoch in epochs:
        opt(epoch=epoch)
        lrs.append(float(opt._get_hyper('learning_rate')))
    g = torch.Generator().manual_seed(3)
    w = torch.randn(50, dtype=torch.float64, generator=g).requires_grad_(True)
    gr = torch.randn(50, dtype=torch.float64, generator=g) * torch.logspace(-8, 0, 50, dtype=torch.float64)
    opt(epoch=3)
    after = []
    for _ in range(3):
        opt.apply_gradients([(gr, w)])
        after.append(w.detach().clone().numpy())
    np.savez_compressed(os.path.join(OUT, 'ref_wiring_adam.npz'), epochs=np.array(epochs), lr=np.array(lrs), w_after=np.stack(after))
    print('wrote tests/golden/ref_wiring_adam.npz')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit('usage: make_ref_wiring.py <checkout of the reference>')
    main(sys.argv[1])
