"""-m gpu: validation in the training dtype (LowPrecisionTrainer.evaluate, fit(eval_dtype=...)) and the command
`python -m bts_amd.train` end to end on a small folder of examples."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import torch_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- evaluate: the set-up of tests/test_lowp_train_gpu.py ----
KW = dict(base_filters=16, groups=8, reduction=2, depth=3)
CROP = (32, 32, 32)
N = 2


def _setup(seed=3, **model_kw):
    import bts_amd  # noqa: F401
    from bts_amd.data import synthetic_batch
    from bts_amd.layers import _base
    from bts_amd.model import Model
    from bts_amd.tape import bump_weights_epoch
    _base.set_seed(seed)
    m = Model(**dict(KW, **model_kw))
    m.build((N,) + CROP + (2,))
    g = torch.Generator().manual_seed(seed + 1)
    for p in m.trainable_variables:
        if p.name.endswith('gamma'):
            p.t.copy_((1.0 + 0.3 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
        elif p.name.endswith('beta') or p.t.dim() == 1:
            p.t.copy_((0.1 * torch.randn(p.t.shape, generator=g)).to(p.t.device))
    bump_weights_epoch()
    latent = KW['base_filters'] * 2 ** (KW['depth'] - 2)
    x, y, mask, eps = synthetic_batch(N, CROP, latent=latent, seed=99)
    return m, x, y, mask, eps


@pytest.mark.parametrize('dtype,loss_lim', [('bfloat16', 5e-3), ('float16', 5e-4)])
def test_evaluate_against_the_fp32_eval_step(dtype, loss_lim):
    """the same forward in 16-bit storage: the limits tests/test_lowp_train_gpu.py states for the step's loss, Dice and label map;
    evaluate leaves parameters and gradients alone and moves the random counters as eval_step does"""
    from bts_amd import train as T
    from bts_amd.lowp_train import LowPrecisionTrainer
    from bts_amd.util import DiceCoefficient, DiceVAELoss
    m, x, y, mask, eps = _setup()
    seeds = (m.vae._seed, m.encoder._seed)
    m.vae.set_eps(eps)
    d32 = DiceCoefficient()
    loss32, macro32, _ = T.eval_step(m, DiceVAELoss(), d32, x, y)
    lab32 = d32.last_labels.clone()
    m.vae.set_eps(eps)
    tr = LowPrecisionTrainer(m, dtype)
    m.flat_grads.normal_()
    g0, p0 = m.flat_grads.clone(), m.flat_params.clone()
    d16 = DiceCoefficient()
    loss16, macro16, _ = tr.evaluate(d16, x, y)
    torch.cuda.synchronize()
    dl = abs(float(loss16) - float(loss32)) / abs(float(loss32))
    mism = float((d16.last_labels != lab32).float().mean())
    print('%s: loss %.6f vs %.6f (rel %.2e), macro Dice %.5f vs %.5f, label changes %.3f %%' %
          (dtype, float(loss16), float(loss32), dl, float(macro16), float(macro32), 100 * mism))
    assert dl <= loss_lim and abs(float(macro16) - float(macro32)) <= 5e-3 and mism <= 1e-2
    assert torch.equal(m.flat_grads, g0) and torch.equal(m.flat_params, p0)
    assert (m.vae._seed, m.encoder._seed) == seeds                 # (eps injected on both engines: nothing was drawn)
    # without an injected eps both engines draw once from the reparameterisation counter and never from the dropout counter
    T.eval_step(m, DiceVAELoss(), DiceCoefficient(), x, y)
    assert (m.vae._seed, m.encoder._seed) == (seeds[0] + 1, seeds[1])
    tr.evaluate(DiceCoefficient(), x, y)
    assert (m.vae._seed, m.encoder._seed) == (seeds[0] + 2, seeds[1])


@pytest.mark.parametrize('dtype', ['bfloat16', 'float16'])
def test_evaluate_is_the_forward_of_the_step(dtype):
    """dropout = 0: step and evaluate run the same forward on the same inputs and eps -> loss and Dice bit for bit"""
    from bts_amd.lowp_train import LowPrecisionTrainer
    from bts_amd.util import DiceCoefficient, ScheduledOptim
    m, x, y, mask, eps = _setup(dropout=0.0)
    tr = LowPrecisionTrainer(m, dtype)
    m.vae.set_eps(eps)
    le, mae, mie = tr.evaluate(DiceCoefficient(), x, y)
    le, mae, mie = float(le), float(mae), float(mie)
    opt = ScheduledOptim(1e-4)
    opt(epoch=0)
    m.vae.set_eps(eps)
    ls, mas, mis = tr.step(opt, DiceCoefficient(), x, y)
    torch.cuda.synchronize()
    assert (le, mae, mie) == (float(ls), float(mas), float(mis))


KW16 = dict(base_filters=16, groups=4, reduction=4, depth=3)
CROP16 = (16, 16, 16)


def test_the_trajectory_does_not_depend_on_the_validating_engine():
    from bts_amd import train as T
    from bts_amd.layers import _base
    from bts_amd.model import Model
    from bts_amd.util import DiceCoefficient, DiceVAELoss, ScheduledOptim
    dev = torch.device('cuda', 0)
    latent = KW16['base_filters'] * 2 ** (KW16['depth'] - 2)
    data = lambda n, seed: [tuple(t.to(dev) for t in R.synthetic_batch(1, CROP16, latent=latent, seed=seed + i)[:2]) for i in range(n)]  # noqa: E731
    train, val = data(3, 100), data(2, 200)
    ends, hists = [], []
    for eval_dtype in (None, 'bfloat16'):
        _base.set_seed(7)
        m = Model(**KW16)
        m.build((1,) + CROP16 + (2,))
        hists.append(T.fit(m, ScheduledOptim(1e-3, n_epochs=4), DiceVAELoss(), DiceCoefficient(), train, val, n_epochs=2, patience=5,
                           log=lambda s: None, compute_dtype='bfloat16', eval_dtype=eval_dtype))
        torch.cuda.synchronize()
        ends.append(m.flat_params.clone())
    assert torch.equal(ends[0], ends[1]), 'max |d| %.3e' % float((ends[0] - ends[1]).abs().max())
    assert [h['train_loss'] for h in hists[0]] == [h['train_loss'] for h in hists[1]]
    # and the 16-bit validation is a validation: next to the fp32 engine's numbers
    for a, b in zip(hists[0], hists[1]):
        assert abs(float(a['val_loss']) - float(b['val_loss'])) <= 5e-3 * abs(float(a['val_loss']))


# ---- the command ----------------------------------------------------------------------------------------------------------------
SIZE = (20, 18, 22, 2)
MODEL_FLAGS = ['--crop_size', '16,16,16', '--base_filters', '16', '--groups', '4', '--reduction', '4', '--depth', '3', '--batch_size', '2']


@pytest.fixture(scope='module')
def folder(tmp_path_factory):
    loc = str(tmp_path_factory.mktemp('dataset'))
    rs = np.random.RandomState(5)
    for sub, n in (('train', 5), ('val', 2)):
        os.makedirs(os.path.join(loc, sub))
        for i in range(n):
            lab = (rs.rand(*SIZE[:3]) * 4).astype(np.int64).astype(np.float32)[..., None]
            np.savez(os.path.join(loc, sub, 'ex%d.npz' % i), x=rs.randn(*SIZE).astype(np.float32), y=lab)
    np.save(os.path.join(loc, 'prepro.npy'), {'size': dict(zip('hwdc', SIZE)), 'norm': {'mean': np.zeros(2), 'std': np.ones(2)}},
            allow_pickle=True)
    return loc


def _argv(folder, out, *more):
    return ['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
            os.path.join(folder, 'prepro.npy'), '--save_folder', out] + MODEL_FLAGS + list(more)


def _run(argv):
    """parse + run in this process from the state a fresh process starts in (the initialiser's generator at its seed)"""
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    from bts_amd.layers import _base
    _base.set_seed(0)
    return T, T.run(T.parse_args(argv))


def _rebuilt(T, out):
    """the model from train_args.pkl alone, as the inference command rebuilds it"""
    from bts_amd.model import Model
    targs = T.load_train_args(out)
    m = Model(**targs['model_args'])
    m.build((1,) + tuple(targs['crop_size']) + (targs['model_args']['in_ch'],))
    meta = T.load_checkpoint(out, m)
    return m, meta


@pytest.mark.parametrize('dtype,fmt', [('float32', 'channels_last'), ('float32', 'channels_first'), ('bfloat16', 'channels_first')])
def test_command_writes_log_checkpoint_and_args(folder, tmp_path, dtype, fmt, capsys):
    out = os.path.join(str(tmp_path), 'run')
    import bts_amd  # noqa: F401
    from bts_amd import train as T
    from bts_amd.layers import _base
    _base.set_seed(0)
    assert T.main(_argv(folder, out, '--n_epochs', '2', '--data_format', fmt, '--dtype', dtype, '--workers', '2')) == 0
    printed = capsys.readouterr().out
    assert 'Train args: ' in printed and '5 training examples.' in printed and '2 validation examples.' in printed
    assert 'Total number of parameters: ' in printed
    lines = open(os.path.join(out, 'train.log')).read().strip().split('\n')
    assert lines[0] == T.LOG_HEADER and len(lines) == 3 and [ln.split(',')[0] for ln in lines[1:]] == ['0', '1']
    assert all(np.isfinite([float(v) for v in ln.split(',')]).all() for ln in lines[1:])
    m, meta = _rebuilt(T, out)
    assert m.data_format == fmt and meta['optimizer']['iterations'] in (3, 6)      # (3 steps per epoch; saved on improvement)
    tensors, _ = T.read_container(os.path.join(out, T.CHECKPOINT_NAME))
    for p in m.trainable_variables:
        assert torch.equal(p.t.cpu(), tensors['var/' + p.name])


def test_rows_are_the_history_and_a_resumed_run_continues(folder, tmp_path):
    out = os.path.join(str(tmp_path), 'run')
    T, res = _run(_argv(folder, out, '--n_epochs', '2', '--data_format', 'channels_last', '--patience', '5'))
    names = ('train_loss', 'train_macro_dice', 'train_micro_dice', 'val_loss', 'val_macro_dice', 'val_micro_dice')
    lines = open(os.path.join(out, 'train.log')).read().strip().split('\n')
    assert [T.log_row(h['epoch'], h['lr'], *[h[k] for k in names]) for h in res['history']] == lines[1:] and len(lines) == 3
    _, meta = T.read_container(os.path.join(out, T.CHECKPOINT_NAME))
    # resumed with conflicting model flags: the folder's train_args.pkl wins, the run starts where the container says
    argv = ['--train_loc', os.path.join(folder, 'train'), '--val_loc', os.path.join(folder, 'val'), '--prepro_loc',
            os.path.join(folder, 'prepro.npy'), '--load_folder', out, '--base_filters', '32', '--depth', '4', '--crop_size', '8,8,8',
            '--data_format', 'channels_first', '--batch_size', '2', '--n_epochs', '3', '--patience', '5']
    import bts_amd  # noqa: F401
    args = T.parse_args(argv)
    assert args.model_args['base_filters'] == 16 and args.model_args['depth'] == 3 and args.crop_size == [16, 16, 16]
    assert args.save_folder == out and args.data_format == 'channels_last'
    seen = []
    real = T.fit

    def spy(model, optimizer, *a, **k):
        seen.append((int(model.epoch.value().numpy()), int(optimizer.iterations)))
        return real(model, optimizer, *a, **k)
    T.fit = spy
    try:
        res2 = T.run(args)
    finally:
        T.fit = real
    assert seen == [(meta['next_epoch'], meta['optimizer']['iterations'])]
    assert [h['epoch'] for h in res2['history']] == list(range(meta['next_epoch'], 3))
    assert res2['model'].encoder.base_filters == 16


def test_one_rank_group_in_a_child_process_gives_the_same_parameters(folder, tmp_path):
    import socket
    plain, grouped = os.path.join(str(tmp_path), 'plain'), os.path.join(str(tmp_path), 'grouped')
    T, _ = _run(_argv(folder, plain, '--n_epochs', '2', '--data_format', 'channels_last', '--dtype', 'bfloat16'))
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    env = dict(os.environ, BTS_FORCE_PG='1', WORLD_SIZE='1', RANK='0', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
               HSA_ENABLE_IPC_MODE_LEGACY='0', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'bts_amd.train'] + _argv(folder, grouped, '--n_epochs', '2', '--data_format', 'channels_last',
                                                                         '--dtype', 'bfloat16'),
                       cwd=ROOT, env=env, timeout=240, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    a, ma = T.read_container(os.path.join(plain, T.CHECKPOINT_NAME))
    b, mb = T.read_container(os.path.join(grouped, T.CHECKPOINT_NAME))
    assert ma['epoch'] == mb['epoch'] and ma['optimizer'] == mb['optimizer']
    assert sorted(k for k in a if k.startswith('var/')) == sorted(k for k in b if k.startswith('var/'))
    for k in a:
        if k.startswith('var/') or k.startswith('adam/'):
            assert torch.equal(a[k], b[k]), k
