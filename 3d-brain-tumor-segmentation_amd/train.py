"""Training-loop shell and checkpoint container (reference train.py:93-216, args.py:176-196).

`fit()` reproduces the reference's epoch loop: optimizer(epoch) schedule call, six tf.keras.metrics.Mean accumulators,
the `train.log` CSV (header train.py:119-126, one row per epoch :186-193), best-validation checkpointing and the
patience rule exactly as written there (:196-208: the epoch that *reaches* `patience` stops, improvements reset it).

Differences, each deliberate:
  * weights: the reference writes Keras HDF5 (`chkpt.hdf5`, train.py:100,201); h5py is not available, so the
    container is safetensors (`chkpt.safetensors`) keyed by the engine's variable names;
  * the reference never saves optimizer state and (SURVEY f-1 caveat) probably not `Model.epoch` either; this
    container persists epoch, Adam m / v / step count and the layers' RNG counters, so a resumed run continues
    bit-exactly (tests/test_train_gpu.py);
  * metric accumulation stays on the device (one scalar add per step) and is read once per epoch -- the reference
    synchronises every step through `.update_state`.

The command (the reference's train.py:219-223 with args.py:86-196):

    python -m bts_amd.train --train_loc DIR/train --val_loc DIR/val --prepro_loc DIR/prepro.npy --save_folder OUT
                            [--dtype bfloat16] [--batch_size 8] [--load_folder OUT] ...

The flags and defaults are the reference's TrainArgParser (args.py:91-143), its two size checks included (args.py:170-174).  --gpu is
accepted and implied: there is no CPU path.  Added: --dtype (training AND validation type), --workers, --resident_gb, --seed, and
the spatial augmentation of the TRAINING examples (add_spatial_arguments: --spatial_prob, --rotate_deg, --zoom_range, --elastic_sigma,
--elastic_spacing; off by default, never applied to --val_loc; data.SpatialConfig), and their intensity augmentation
(add_intensity_arguments: --intensity_aug and the --noise_*, --blur_*, --brightness_*, --contrast_* and --gamma_* flags; off by
default, never applied to --val_loc; data.IntensityConfig), the foreground oversampling of their crops (add_foreground_arguments:
--foreground_prob, --foreground_samples, --foreground_classes; off by default, never applied to --val_loc; data.ForegroundConfig;
stored in train_args.pkl and restored by --load_folder, an older pickle meaning off), and --targets (add_target_arguments: `labels`, the default, trains the
output channels on the disjoint labels as the reference does; `regions` trains them on the nested BraTS regions WT, TC, ET, for both
datasets, and the Dice columns of train.log are then util.RegionDiceCoefficient's; the mode is stored in train_args.pkl, restored by
--load_folder and read by `python -m bts_amd.test`), and the training loss (add_loss_arguments: --loss `dice`, the default, is the
reference's util.DiceVAELoss; `dice_ce` and `dice_focal` add a voxel-wise binary cross-entropy or focal term on the sigmoid outputs,
util.CompoundVAELoss, weighted by --dice_weight and --ce_weight, the focal term shaped by --focal_gamma and --focal_alpha; in both
engines; train_loss and val_loss of train.log are then the compound loss; stored in train_args.pkl and restored by --load_folder).
Examples are the `.npz` files `python -m bts_amd.preprocess` writes; with a process group in the environment (torchrun) every rank
runs the command, takes its shard and rank 0 writes the files.

Deviations:
  * `--downsampling avg` is refused at parse time by name (the reference accepts it and then calls None: no such layer exists);
  * an empty --val_loc is refused (the reference ends in os.listdir(''));
  * an empty --save_folder writes no files (the reference ends in os.mkdir(''));
  * --load_folder reads `crop_size` as the key of the pickled dict it is (args.py:184 asks the dict for an attribute) and resumes
    at the container's `next_epoch` with the optimiser state (see above); the spatial and intensity augmentation flags are restored with the
    crop (a train_args.pkl from before they existed has none of them and means "off");
  * `train_args.pkl` is the plain dict of the arguments (`model_args` with `in_ch`, `crop_size`, ...), written by rank 0 alone.
"""
import argparse
import json
import os
import pickle
import sys

import numpy as np
import torch

from . import parallel
from .tape import Tensor, bump_weights_epoch
from .util import reduce_sum, train_step

LOG_HEADER = ','.join(['epoch', 'lr', 'train_loss', 'train_macro_dice', 'train_micro_dice', 'val_loss',
                       'val_macro_dice', 'val_micro_dice'])                       # train.py:119-126
CHECKPOINT_NAME = 'chkpt.safetensors'                                             # reference: chkpt.hdf5 (train.py:201)
ARGS_NAME = 'train_args.pkl'                                                      # args.py:193-194
FORMAT_VERSION = 2      # 2: Adam moments in the backward-completion order of the flat buffers (model._flatten_parameters, round 3)


class Mean(object):
    """tf.keras.metrics.Mean: float32 running total / count (train.py:109-114)."""

    def __init__(self, name='mean'):
        self.name = name
        self.reset_states()

    def reset_states(self):
        self.total = None
        self.count = 0
        self._host = np.float32(0.0)

    def update_state(self, value):
        if isinstance(value, Tensor):
            value = value.t
        if torch.is_tensor(value):
            v = value.detach().reshape(()).to(torch.float32)
            self.total = v.clone() if self.total is None else self.total + v
        else:
            self._host = np.float32(self._host + np.float32(value))
        self.count += 1

    def result(self):
        """np.float32, like `metric.result().numpy()`; 0.0 before the first update (Keras divides no-NaN)"""
        if self.count == 0:
            return np.float32(0.0)
        tot = self._host
        if self.total is not None:
            tot = np.float32(tot + np.float32(self.total.item()))
        return np.float32(tot / np.float32(self.count))


def log_row(epoch, lr, train_loss, train_macro, train_micro, val_loss, val_macro, val_micro):
    """one `train.log` line, formatted like the reference's str(<float32>.numpy()) fields (train.py:186-193)"""
    f = lambda v: str(np.float32(v))
    return ','.join([str(int(epoch)), f(lr), f(train_loss), f(train_macro), f(train_micro), f(val_loss), f(val_macro),
                     f(val_micro)])


class PatienceTracker(object):
    """train.py:195-208 verbatim: improvement -> save + reset; otherwise stop once `patience` epochs have already
    passed without one (the check precedes the increment, so training runs patience + 1 non-improving epochs)."""

    def __init__(self, patience):
        self.limit = patience
        self.best = 0.0
        self.patience = 0

    def update(self, val_macro_dice):
        """-> 'save' | 'stop' | 'wait'"""
        if val_macro_dice > self.best:
            self.best = val_macro_dice
            self.patience = 0
            return 'save'
        if self.patience == self.limit:
            return 'stop'
        self.patience += 1
        return 'wait'


# ---- checkpoint container ------------------------------------------------------------------------------------------
def write_container(path, tensors, meta):
    """tensors: {name: torch tensor}; meta: JSON-able dict (stored in the safetensors header)"""
    from safetensors.torch import save_file
    save_file({k: v.detach().to('cpu').contiguous() for k, v in tensors.items()}, path,
              metadata={'bts': json.dumps(meta)})


def read_container(path):
    from safetensors import safe_open
    tensors = {}
    with safe_open(path, framework='pt', device='cpu') as f:
        meta = json.loads((f.metadata() or {}).get('bts', '{}'))
        for k in f.keys():
            tensors[k] = f.get_tensor(k)
    return tensors, meta


def _rng_layers(model):
    out = {}
    for name in ('encoder', 'vae'):
        lay = getattr(model, name, None)
        if lay is not None and hasattr(lay, '_seed'):
            out[name] = lay
    return out


_RANK_STRIDE = 0x9E3779B97F4A7C15      # parallel.decorrelate_rng: rank r's counters run at base + r * stride (mod 2^63)


def save_checkpoint(folder, model, optimizer=None, completed=False, tracker=None, datasets=None, write=True):
    """weights by variable name + `epoch`; with an optimizer also Adam m / v (flat order) and its step count.

    Data-parallel runs: EVERY rank calls this (it gathers the per-rank random state: each rank's augmentation generator;
    the dropout / reparameterisation counters are stored rank-independent, as their base value), rank 0 alone passes
    write=True.  A resumed rank r gets back ITS generator state and base + r * stride counters, so all ranks continue the
    uninterrupted trajectory instead of replaying rank 0's draws.

    completed=True (what fit() passes: it saves AFTER the epoch's last step): the container also records
    `next_epoch = epoch + 1`, and a resumed fit() starts there -- the reference restarts at the saved epoch
    (train.py:133-135) but carries no optimizer state; with Adam moments, step count and RNG counters persisted, repeating
    that epoch would apply it twice.  tracker: the PatienceTracker (best / patience persist, so the first resumed epoch cannot
    overwrite a better checkpoint).  datasets: {'train': ds, 'val': ds}; objects with state_dict() (data._Dataset: shuffle
    and augmentation generators) are persisted."""
    tensors = {'var/' + p.name: p.t for p in model.trainable_variables}
    rk = parallel.rank() if getattr(model, '_rng_rank', None) is not None else 0      # offset decorrelate_rng applied, if it ran
    meta = {'format': FORMAT_VERSION, 'epoch': int(model.epoch.value().numpy()), 'n_params': int(model.n_params),
            'rng': {k: (int(v._seed) - rk * _RANK_STRIDE) & 0x7FFFFFFFFFFFFFFF for k, v in _rng_layers(model).items()},
            'rng_is_base': True}
    if completed:
        meta['next_epoch'] = meta['epoch'] + 1
    if tracker is not None:
        meta['tracker'] = {'best': float(tracker.best), 'patience': int(tracker.patience)}
    tr16 = getattr(model, '_trainer16', None)          # fit(compute_dtype=...): the dynamic loss scale is training state too
    if tr16 is not None:
        tr16.settle()           # the last step's overflow decision belongs to the state that is saved
        meta['loss_scale'] = {'dtype': tr16.dtype_name, 'scale': float(tr16.loss_scale), 'clean_steps': int(tr16._clean_steps),
                              'skipped_steps': int(tr16.skipped_steps)}
    local = {}
    for key, ds in (datasets or {}).items():
        if hasattr(ds, 'state_dict'):
            for k, v in ds.state_dict().items():
                local['data/%s/%s' % (key, k)] = v
    per_rank = parallel.gather_objects(local)          # a collective when a process group exists: all ranks are here
    for r, st in enumerate(per_rank):
        for k, v in st.items():
            if k.endswith('/gen'):
                tensors['%s@%d' % (k, r)] = v          # augmentation draws: one stream per rank
            elif r == 0:
                tensors[k] = v                         # the shuffle generator is common to all ranks
    if not write:
        return meta
    if optimizer is not None:
        meta['optimizer'] = {'iterations': int(optimizer.iterations), 'learning_rate': float(optimizer.learning_rate),
                             'init_lr': float(optimizer.init_lr), 'n_epochs': float(optimizer.n_epochs)}
        st = optimizer._state.get(id(model.flat_params))
        if st is not None:
            tensors['adam/m'], tensors['adam/v'] = st[0], st[1]
    os.makedirs(folder, exist_ok=True)
    tmp = os.path.join(folder, CHECKPOINT_NAME + '.tmp')
    write_container(tmp, tensors, meta)
    os.replace(tmp, os.path.join(folder, CHECKPOINT_NAME))
    return meta


def load_checkpoint(folder, model, optimizer=None):
    """inverse of save_checkpoint; the model must be built (same architecture).  Returns the stored meta dict."""
    tensors, meta = read_container(os.path.join(folder, CHECKPOINT_NAME))
    fmt = meta.get('format')
    if fmt not in (1, FORMAT_VERSION):
        raise ValueError('unknown checkpoint format %r' % (fmt,))
    missing = [p.name for p in model.trainable_variables if 'var/' + p.name not in tensors]
    if missing:
        raise KeyError('checkpoint lacks %d variables, e.g. %s' % (len(missing), missing[:3]))
    for p in model.trainable_variables:
        src = tensors['var/' + p.name]
        if tuple(src.shape) != tuple(p.t.shape):
            raise ValueError('shape mismatch for %s: %s vs %s' % (p.name, tuple(src.shape), tuple(p.t.shape)))
        p.t.copy_(src.to(p.t.device))
    model.epoch.assign(int(meta.get('next_epoch', meta.get('epoch', 0))))
    # consumed by the next fit(): PatienceTracker state and the datasets' generator states
    data = {}
    mine = '@%d' % parallel.rank()
    for k, v in tensors.items():
        if not k.startswith('data/'):
            continue
        if '@' in k:                                  # per-rank entries: keep this rank's, under the plain name
            if k.endswith(mine):
                data[k[len('data/'):-len(mine)]] = v
        else:
            data.setdefault(k[len('data/'):], v)
    model._resume = {'tracker': meta.get('tracker'), 'data': data, 'loss_scale': meta.get('loss_scale')}
    for k, lay in _rng_layers(model).items():
        if k in meta.get('rng', {}):
            lay._seed = int(meta['rng'][k])
    if meta.get('rng_is_base'):                       # counters were stored without the rank offset: re-apply this rank's
        model._rng_rank = None
        if parallel.active():
            parallel.decorrelate_rng(model)
    if optimizer is not None and 'optimizer' in meta:
        o = meta['optimizer']
        optimizer.iterations = int(o['iterations'])
        optimizer.learning_rate = float(o['learning_rate'])
        if 'adam/m' in tensors and fmt != FORMAT_VERSION:
            # format 1 stored the Adam moments in the flat order of that build (reference variable order); variables are keyed by name and
            # load fine, the moments cannot be mapped without that order: they restart at zero (and the bias correction with them)
            import warnings
            warnings.warn('checkpoint format %r: weights, epoch and random state restored; Adam moments dropped (flat order changed in '
                          'format %d)' % (fmt, FORMAT_VERSION))
            optimizer.iterations = 0
        elif 'adam/m' in tensors:
            dev = model.flat_params.device
            optimizer._state[id(model.flat_params)] = (tensors['adam/m'].to(dev).contiguous(),
                                                       tensors['adam/v'].to(dev).contiguous())
    bump_weights_epoch()
    return meta


def save_train_args(folder, args_dict):
    """args.py:193-194: the run's arguments as a pickled plain dict (`train_args.pkl`), read back by a resumed run or by
    the inference script to rebuild the model (`model_args`, `crop_size`)"""
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, ARGS_NAME), 'wb') as f:
        pickle.dump(dict(args_dict), f)


def load_train_args(folder):
    with open(os.path.join(folder, ARGS_NAME), 'rb') as f:
        return pickle.load(f)


# ---- the loop -------------------------------------------------------------------------------------------------------
def eval_step(model, loss_fn, dice_fn, x, y):
    """validation iteration, train.py:166-173: forward with training=False, loss incl. regularisers, Dice"""
    y_pred, y_vae, z_mean, z_logvar = model(x, training=False, inference=False)
    loss = loss_fn(x, y, y_pred, y_vae, z_mean, z_logvar)
    loss = loss + reduce_sum(model.losses)
    macro, micro = dice_fn(y, y_pred)
    return loss, macro, micro


def fit(model, optimizer, loss_fn, dice_fn, train_data, val_data, n_epochs, patience=10, save_folder=None,
        train_step_fn=None, eval_step_fn=None, log=print, compute_dtype=None, eval_dtype=None):
    """The reference's `train(args)` from the logging set-up on (train.py:116-216).

    compute_dtype: None / 'float32' = the fp32 engine (util.train_step); 'bfloat16' / 'float16' = the 16-bit-storage engine
    (lowp_train.LowPrecisionTrainer.step: fp32 master weights, fp32 statistics, fp16 with dynamic loss scaling) for the training
    iterations.  That engine evaluates its loss itself: util.DiceVAELoss' (train.py:143-147) unless loss_fn carries a `.spec`
    (util.CompoundVAELoss: a util.LossSpec), in which case the 16-bit trainer is built with that spec -- or rebuilt, if the model
    holds one built for another loss -- and trains and validates on the same compound loss; loss_fn itself is called by the fp32
    steps only.
    eval_dtype: None / 'float32' = validation on the fp32 engine (eval_step), whatever the training type; 'bfloat16' / 'float16' =
    validation through the same 16-bit engine (LowPrecisionTrainer.evaluate: no switch of engines, weight images and allocator
    footprint once per epoch).  Both advance the random counters alike, so the training trajectory is the same either way.

    train_data / val_data: re-iterable collections of (x, y) batches (NDHWC tensors on the device).
    Resumes at `model.epoch` (train.py:133).  Returns the list of per-epoch rows (dicts).  On data-parallel runs every
    rank must call fit() (with the same n_epochs / patience; equally long shards) and iterates its own shard; rank 0 alone writes
    files, and rank 0's validation Dice drives the save / stop decision of all ranks."""
    def trainer16(dtype):
        from .lowp_train import LowPrecisionTrainer
        trainer = getattr(model, '_trainer16', None)
        spec = getattr(loss_fn, 'spec', None)
        if trainer is None or trainer.dtype_name != dtype or trainer.loss_spec != spec:
            trainer = model._trainer16 = LowPrecisionTrainer(model, dtype, loss=spec)
        return trainer
    if train_step_fn is None and compute_dtype not in (None, 'float32'):
        trainer = trainer16(compute_dtype)
        saved = (getattr(model, '_resume', None) or {}).get('loss_scale')
        if saved and saved.get('dtype') == compute_dtype:
            trainer.loss_scale, trainer._clean_steps = float(saved['scale']), int(saved['clean_steps'])
            trainer.skipped_steps = int(saved.get('skipped_steps', 0))
        train_step_fn = lambda x, y: trainer.step(optimizer, dice_fn, x, y)     # noqa: E731
    if eval_step_fn is None and eval_dtype not in (None, 'float32'):
        evaluator = trainer16(eval_dtype)
        eval_step_fn = lambda x, y: evaluator.evaluate(dice_fn, x, y)           # noqa: E731
    tstep = train_step_fn or (lambda x, y: train_step(model, optimizer, loss_fn, dice_fn, x, y))
    estep = eval_step_fn or (lambda x, y: eval_step(model, loss_fn, dice_fn, x, y))
    writer = save_folder is not None and parallel.rank() == 0
    names = ('train_loss', 'train_macro_dice', 'train_micro_dice', 'val_loss', 'val_macro_dice', 'val_micro_dice')
    m = {k: Mean(k) for k in names}
    if writer:
        os.makedirs(save_folder, exist_ok=True)
        with open(os.path.join(save_folder, 'train.log'), 'w') as f:
            f.write(LOG_HEADER + '\n')
    tracker = PatienceTracker(patience)
    resume = getattr(model, '_resume', None)       # left by load_checkpoint
    if resume is not None:
        model._resume = None
        if resume.get('tracker'):
            tracker.best, tracker.patience = float(resume['tracker']['best']), int(resume['tracker']['patience'])
        for key, ds in (('train', train_data), ('val', val_data)):
            st = {k[len(key) + 1:]: v for k, v in resume.get('data', {}).items() if k.startswith(key + '/')}
            if st and hasattr(ds, 'load_state_dict'):
                ds.load_state_dict(st)
    history = []
    for epoch in range(int(model.epoch.value().numpy()), int(n_epochs)):
        log('Epoch {}.'.format(epoch))
        model.epoch.assign(epoch)
        optimizer(epoch=epoch)
        for x, y in train_data:
            loss, macro, micro = tstep(x, y)
            m['train_loss'].update_state(loss)
            m['train_macro_dice'].update_state(macro)
            m['train_micro_dice'].update_state(micro)
        log('Training. Loss: {l: .4f}, Macro Dice: {d1: 1.4f}, Micro Dice: {d2: 1.4f}.'.format(
            l=m['train_loss'].result(), d1=m['train_macro_dice'].result(), d2=m['train_micro_dice'].result()))
        for x, y in val_data:
            loss, macro, micro = estep(x, y)
            m['val_loss'].update_state(loss)
            m['val_macro_dice'].update_state(macro)
            m['val_micro_dice'].update_state(micro)
        log('Validation. Loss: {l: .4f}, Macro Dice: {d1: 1.4f}, Micro Dice: {d2: 1.4f}.'.format(
            l=m['val_loss'].result(), d1=m['val_macro_dice'].result(), d2=m['val_micro_dice'].result()))
        row = {'epoch': epoch, 'lr': np.float32(optimizer.learning_rate)}
        row.update({k: m[k].result() for k in names})
        history.append(row)
        if writer:
            with open(os.path.join(save_folder, 'train.log'), 'a') as f:
                f.write(log_row(epoch, row['lr'], *[row[k] for k in names]) + '\n')
        # The save / stop decision must be the same on every rank: save_checkpoint is a collective (it gathers the per-rank random
        # state) and a rank that stops alone leaves the others in the next gradient exchange.  The built-in DiceCoefficient all-reduces
        # its sums, a custom eval_step_fn / metric need not -- so rank 0's validation Dice decides for all, and whether files are
        # wanted is agreed on as well (a save_folder on rank 0 only is fine)
        val_dice, want_files = float(row['val_macro_dice']), save_folder is not None
        if parallel.active():
            got = parallel.gather_objects((val_dice, want_files))
            val_dice, want_files = got[0][0], any(w for _, w in got)
        action = tracker.update(val_dice)
        if action == 'save':
            if want_files:                       # every rank: the per-rank random state is gathered; rank 0 writes
                save_checkpoint(save_folder, model, optimizer, completed=True, tracker=tracker,
                                datasets={'train': train_data, 'val': val_data}, write=writer)
            log('Saved model weights.')
        elif action == 'stop':
            log('Validation dice has not improved in {} epochs. Stopped training.'.format(patience))
            return history
        for k in names:
            m[k].reset_states()
    return history


# ---- the command ----------------------------------------------------------------------------------------------------
def arg_parser():
    """the flags of the reference's TrainArgParser (args.py:91-143) and ours"""
    p = argparse.ArgumentParser(prog='python -m bts_amd.train', description=__doc__.split('\n')[0])
    p.add_argument('--train_loc', type=str, required=True, help='Folder of .npz training examples.')
    p.add_argument('--prepro_loc', type=str, required=True, help='The prepro.npy written by the preprocessing command.')
    p.add_argument('--val_loc', type=str, default='', help='Folder of .npz validation examples.')
    p.add_argument('--save_folder', type=str, default='', help='Folder for train.log, the checkpoint and train_args.pkl; empty: nothing is written.')
    p.add_argument('--load_folder', type=str, default='', help='Folder of an earlier run to resume; its train_args.pkl decides model and crop.')
    p.add_argument('--lr', type=float, default=1e-4, help='Learning rate at epoch 0 of the polynomial schedule.')
    p.add_argument('--batch_size', type=int, default=1, help='Examples per step (per rank).')
    p.add_argument('--patience', type=int, default=-1, help='Stop after this many epochs without a better validation Dice; -1: never.')
    p.add_argument('--n_epochs', type=int, default=300, help='Last epoch + 1.')
    p.add_argument('--gpu', action='store_true', default=False, help='Accepted for the reference\'s command line; the GPU is always used.')
    p.add_argument('--crop_size', type=str, default='128,128,128', help='Training crop as h,w,d.')
    p.add_argument('--data_format', type=str, dest='model_args.data_format', default='channels_first',
                   choices=['channels_last', 'channels_first'], help='Memory order of the batches the model takes.')
    p.add_argument('--base_filters', type=int, dest='model_args.base_filters', default=32,
                   help='Filters of the first level; doubled per level.')
    p.add_argument('--depth', type=int, dest='model_args.depth', default=4, help='Levels of the encoder.')
    p.add_argument('--l2_scale', type=float, dest='model_args.l2_scale', default=1e-5,
                   help='Weight of the L2 term on every conv kernel.')
    p.add_argument('--dropout', type=float, dest='model_args.dropout', default=0.2, help='Dropout rate on the input volume.')
    p.add_argument('--groups', type=int, dest='model_args.groups', default=8, help='Groups of every GroupNorm.')
    p.add_argument('--reduction', type=int, dest='model_args.reduction', default=8,
                   help='Channel reduction of the squeeze-excitation gates.')
    p.add_argument('--downsampling', type=str, dest='model_args.downsampling', default='conv', choices=['conv', 'max', 'avg'],
                   help='Down-sampler (avg: listed by the reference, built by neither).')
    p.add_argument('--upsampling', type=str, dest='model_args.upsampling', default='conv', choices=['conv', 'linear'],
                   help='Up-sampler.')
    p.add_argument('--out_ch', type=int, dest='model_args.out_ch', default=3, help='Output classes (labels without the background).')
    p.add_argument('--dtype', type=str, default='float32', choices=('float32', 'bfloat16', 'float16'),
                   help='Storage type of activations and weight images in training and validation.')
    p.add_argument('--workers', type=int, default=8, help='Host threads that read the next examples; 0 reads in line.')
    p.add_argument('--resident_gb', type=float, default=None,
                   help='Budget (GB) of examples kept on the device after their first read (default: a quarter of its memory; 0: none).')
    p.add_argument('--seed', type=int, default=0, help='Seed of the shuffle and augmentation generators.')
    return p


SPATIAL_KEYS = ('spatial_prob', 'rotate_deg', 'zoom_range', 'elastic_sigma', 'elastic_spacing')


def add_spatial_arguments(p):
    """the flags of the spatial training augmentation (data.SpatialConfig), a group of their own: arg_parser() stays the reference's
    flag set plus the run's, which tests/golden/train_cli_flags.json is held against"""
    g = p.add_argument_group('spatial augmentation of the training examples')
    g.add_argument('--spatial_prob', type=float, default=0.0,
                   help='Probability that a training example is rotated, zoomed and deformed; 0: off.')
    g.add_argument('--rotate_deg', type=str, default='15', help='Largest rotation in degrees about each axis: a or a0,a1,a2.')
    g.add_argument('--zoom_range', type=str, default='0.9,1.1', help='Zoom is uniform in lo,hi; above 1 magnifies.')
    g.add_argument('--elastic_sigma', type=float, default=0.0,
                   help='Standard deviation, in voxels, of the control-node displacements of the elastic deformation; 0: none.')
    g.add_argument('--elastic_spacing', type=int, default=32, help='Voxels between control nodes of the elastic deformation.')
    return p


INTENSITY_KEYS = ('intensity_aug', 'noise_prob', 'noise_sigma', 'blur_prob', 'blur_sigma', 'blur_channel_prob', 'brightness_prob',
                  'brightness_range', 'contrast_prob', 'contrast_range', 'gamma_prob', 'gamma_range', 'gamma_invert_prob')
_INTENSITY_RANGES = ('noise_sigma', 'blur_sigma', 'brightness_range', 'contrast_range', 'gamma_range')


def add_intensity_arguments(p):
    """the flags of the intensity training augmentation (data.IntensityConfig, whose defaults these are), a group of their own like
    the spatial one"""
    g = p.add_argument_group('intensity augmentation of the training examples')
    g.add_argument('--intensity_aug', action='store_true',
                   help='Gaussian noise, Gaussian blur, brightness, contrast and gamma on the training crops (off by default).')
    g.add_argument('--noise_prob', type=float, default=0.1, help='Probability of Gaussian noise.')
    g.add_argument('--noise_sigma', type=str, default='0,0.1', help='Standard deviation of the noise is uniform in lo,hi.')
    g.add_argument('--blur_prob', type=float, default=0.2, help='Probability of Gaussian blur.')
    g.add_argument('--blur_sigma', type=str, default='0.5,1.0', help='Sigma of the blur, in voxels, is uniform in lo,hi per channel.')
    g.add_argument('--blur_channel_prob', type=float, default=0.5, help='Probability that a channel of a blurred example is blurred.')
    g.add_argument('--brightness_prob', type=float, default=0.15, help='Probability of a multiplicative brightness change.')
    g.add_argument('--brightness_range', type=str, default='0.75,1.25', help='The brightness factor is uniform in lo,hi.')
    g.add_argument('--contrast_prob', type=float, default=0.15, help='Probability of a contrast change.')
    g.add_argument('--contrast_range', type=str, default='0.75,1.25', help='The contrast factor lies in lo,hi (either side of 1 equally likely).')
    g.add_argument('--gamma_prob', type=float, default=0.3, help='Probability of a gamma transform.')
    g.add_argument('--gamma_range', type=str, default='0.7,1.5', help='Gamma lies in lo,hi (either side of 1 equally likely).')
    g.add_argument('--gamma_invert_prob', type=float, default=0.1, help='Probability that a gamma transform acts on the negated image.')
    return p


FOREGROUND_KEYS = ('foreground_prob', 'foreground_samples', 'foreground_classes')


def add_foreground_arguments(p):
    """the flags of the foreground oversampling of the training crops (data.ForegroundConfig), a group of their own like the augmentation
    ones"""
    g = p.add_argument_group('foreground oversampling of the training crops')
    g.add_argument('--foreground_prob', type=float, default=0.0,
                   help='Probability that a training crop is centred on a random voxel of a random foreground class of its example; 0: off.')
    g.add_argument('--foreground_samples', type=int, default=10000,
                   help='Voxels kept per class in an example\'s class-location table (evenly spaced over the class).')
    g.add_argument('--foreground_classes', type=str, default='',
                   help='Classes to choose from, as c0,c1,... out of 0..out_ch-1 (class c is label c+1); empty: all.')
    return p


def add_target_arguments(p):
    """the flag of the target encoding (data.TARGETS), a group of its own like the augmentation ones"""
    g = p.add_argument_group('target encoding')
    g.add_argument('--targets', type=str, default='labels', choices=('labels', 'regions'),
                   help='What the output channels are trained on: the disjoint labels 1, 2, 4 (the reference), or the nested BraTS '
                        'regions whole tumour, tumour core, enhancing tumour (needs --out_ch 3).')
    return p


LOSS_KEYS = ('loss', 'dice_weight', 'ce_weight', 'focal_gamma', 'focal_alpha')
LOSSES = ('dice', 'dice_ce', 'dice_focal')
LOSS_DEFAULTS = {'loss': 'dice', 'dice_weight': 1.0, 'ce_weight': 1.0, 'focal_gamma': 2.0, 'focal_alpha': None}


def add_loss_arguments(p):
    """the flags of the training loss (util.LossSpec), a group of their own like the augmentation ones"""
    g = p.add_argument_group('training loss')
    g.add_argument('--loss', type=str, default=LOSS_DEFAULTS['loss'], choices=LOSSES,
                   help='dice: the reference\'s soft Dice + VAE terms; dice_ce / dice_focal: plus a voxel-wise binary cross-entropy / '
                        'focal term on the sigmoid outputs.')
    g.add_argument('--dice_weight', type=float, default=LOSS_DEFAULTS['dice_weight'], help='Weight of the Dice term (dice_ce, dice_focal).')
    g.add_argument('--ce_weight', type=float, default=LOSS_DEFAULTS['ce_weight'], help='Weight of the cross-entropy / focal term (dice_ce, dice_focal).')
    g.add_argument('--focal_gamma', type=float, default=LOSS_DEFAULTS['focal_gamma'], help='Focusing exponent of the focal term, in [0, 8] (dice_focal).')
    g.add_argument('--focal_alpha', type=float, default=LOSS_DEFAULTS['focal_alpha'],
                   help='Weight alpha of the positive targets and 1 - alpha of the negative ones, in (0, 1) (dice_focal; default: none).')
    return p


def full_parser():
    """what the command parses: arg_parser() and the spatial augmentation, intensity augmentation, foreground, target and loss groups"""
    return add_loss_arguments(add_target_arguments(add_foreground_arguments(add_intensity_arguments(add_spatial_arguments(arg_parser())))))


def _floats(text, counts, flag):
    try:
        vals = [float(v) for v in str(text).split(',')]
    except ValueError:
        vals = []
    if len(vals) not in counts:
        raise ValueError('%s: expected %s comma-separated numbers, got %r' % (flag, ' or '.join(str(n) for n in counts), text))
    return vals


def spatial_config(args):
    """the data.SpatialConfig of the parsed (or unpickled) arguments, None when spatial_prob is 0 or absent"""
    a = args if isinstance(args, dict) else vars(args)
    if not a.get('spatial_prob'):
        return None
    from .data import SpatialConfig
    return SpatialConfig(a['spatial_prob'], rotate_deg=a['rotate_deg'], zoom=a['zoom_range'], elastic_sigma=a['elastic_sigma'],
                         elastic_spacing=a['elastic_spacing'])


def intensity_config(args):
    """the data.IntensityConfig of the parsed (or unpickled) arguments, None when intensity_aug is off or absent"""
    a = args if isinstance(args, dict) else vars(args)
    if not a.get('intensity_aug'):
        return None
    from .data import IntensityConfig
    return IntensityConfig(noise_prob=a['noise_prob'], noise_sigma=a['noise_sigma'], blur_prob=a['blur_prob'], blur_sigma=a['blur_sigma'],
                           blur_channel_prob=a['blur_channel_prob'], brightness_prob=a['brightness_prob'],
                           brightness=a['brightness_range'], contrast_prob=a['contrast_prob'], contrast=a['contrast_range'],
                           gamma_prob=a['gamma_prob'], gamma=a['gamma_range'], gamma_invert_prob=a['gamma_invert_prob'])


def foreground_config(args):
    """the data.ForegroundConfig of the parsed (or unpickled) arguments, None when foreground_prob is 0 or absent; a class outside
    range(out_ch) is refused here"""
    a = args if isinstance(args, dict) else vars(args)
    if not a.get('foreground_prob'):
        return None
    from .data import ForegroundConfig
    cfg = ForegroundConfig(a['foreground_prob'], samples=a.get('foreground_samples', 10000), classes=a.get('foreground_classes') or None)
    cfg.allowed(a['model_args']['out_ch'])
    return cfg


def loss_spec(args):
    """the util.LossSpec of the parsed (or unpickled) arguments, None for `dice` (or no `loss` key: an older pickle) -- the reference's
    loss, which has no weights: a non-default --dice_weight / --ce_weight is refused with it"""
    a = dict(LOSS_DEFAULTS, **{k: v for k, v in (args if isinstance(args, dict) else vars(args)).items() if k in LOSS_DEFAULTS})
    kind, dw, cw = a['loss'], a['dice_weight'], a['ce_weight']
    if kind not in LOSSES:
        raise ValueError('--loss: unknown loss %r, one of %s' % (kind, ', '.join(LOSSES)))
    if kind == 'dice':
        for flag, v in (('--dice_weight', dw), ('--ce_weight', cw)):
            if float(v) != 1.0:
                raise ValueError('%s %r with --loss dice: the reference\'s loss has no weights; use --loss dice_ce or dice_focal' % (flag, v))
        return None
    from .util import LossSpec
    try:                                   # (dice_ce ignores the focal flags)
        return LossSpec(kind, dw, cw, a['focal_gamma'], a['focal_alpha']) if kind == 'dice_focal' else LossSpec(kind, dw, cw)
    except ValueError as e:                # LossSpec names the field first: say which flag set it
        field = str(e).split(' ', 1)[0]
        raise ValueError('--%s: %s' % ({'gamma': 'focal_gamma', 'alpha': 'focal_alpha'}.get(field, field), e))


def parse_args(argv=None):
    """args.py:145-196: model_args.* folded into a dict, crop split, sizes from the prepro dump, the two size checks, --load_folder;
    writes train_args.pkl (rank 0, when there is a save folder)"""
    from .preprocess import load_prepro
    args = full_parser().parse_args(argv)
    deg = _floats(args.rotate_deg, (1, 3), '--rotate_deg')
    args.rotate_deg = deg * 3 if len(deg) == 1 else deg
    args.zoom_range = _floats(args.zoom_range, (2,), '--zoom_range')
    for key in _INTENSITY_RANGES:
        setattr(args, key, _floats(getattr(args, key), (2,), '--' + key))
    try:
        args.foreground_classes = [int(v) for v in args.foreground_classes.split(',')] if args.foreground_classes else None
    except ValueError:
        raise ValueError('--foreground_classes: expected comma-separated integers, got %r' % (args.foreground_classes,))
    args.model_args = {}
    for key in [k for k in vars(args) if k.startswith('model_args.')]:                                    # args.py:24-38
        args.model_args[key.split('.', 1)[1]] = getattr(args, key)
        delattr(args, key)
    args.data_format = args.model_args['data_format']
    if args.model_args['downsampling'] == 'avg':
        raise ValueError("--downsampling avg: the reference lists 'avg' and builds no such layer (its model calls None); use conv or max")
    if not args.val_loc:
        raise ValueError('--val_loc is empty: every epoch validates (train.py:165), a validation folder is needed')
    args.crop_size = [int(s) for s in args.crop_size.split(',')]
    size, _, _ = load_prepro(args.prepro_loc)
    args.prepro_size = [int(s) for s in size]
    if (args.model_args['base_filters'] / 2) % args.model_args['groups'] != 0:                             # args.py:170-171
        raise AssertionError('Base filters must be a multiple of {} for group normalization at lowest spatial level.'.format(
            args.model_args['groups'] * 2))
    if args.model_args['base_filters'] % args.model_args['reduction'] != 0:                                # args.py:173-174
        raise AssertionError('Base filters must be a multiple of {} for squeeze-excitation reduction.'.format(
            args.model_args['reduction']))
    args.model_args['in_ch'] = args.prepro_size[3]
    if args.load_folder:                                                                                   # args.py:180-186
        chkpt_args = load_train_args(args.load_folder)
        args.model_args = chkpt_args['model_args']
        args.crop_size = [int(s) for s in chkpt_args['crop_size']]
        assert isinstance(args.model_args, dict)
        args.data_format = args.model_args['data_format']
        args.save_folder = args.load_folder
        args.spatial_prob = 0.0 if 'spatial_prob' not in chkpt_args else chkpt_args['spatial_prob']      # (an older pickle: off)
        for key in SPATIAL_KEYS[1:]:
            if key in chkpt_args:
                setattr(args, key, chkpt_args[key])
        args.intensity_aug = bool(chkpt_args.get('intensity_aug', False))                                  # (an older pickle: off)
        for key in INTENSITY_KEYS[1:]:
            if key in chkpt_args:
                setattr(args, key, chkpt_args[key])
        args.foreground_prob = chkpt_args.get('foreground_prob', 0.0)                                      # (an older pickle: off)
        for key in FOREGROUND_KEYS[1:]:
            if key in chkpt_args:
                setattr(args, key, chkpt_args[key])
        args.targets = chkpt_args.get('targets', 'labels')                                                 # (an older pickle: labels)
        args.loss = chkpt_args.get('loss', 'dice')                                                         # (an older pickle: dice)
        for key in LOSS_KEYS[1:]:
            setattr(args, key, chkpt_args.get(key, LOSS_DEFAULTS[key]))
    spatial_config(args)                      # (a bad range or probability is refused here, not at the first batch)
    intensity_config(args)
    foreground_config(args)
    loss_spec(args)
    if args.targets == 'regions' and int(args.model_args['out_ch']) != 3:
        raise ValueError('--targets regions trains the three BraTS regions WT, TC, ET: --out_ch must be 3, got %r' %
                         (args.model_args['out_ch'],))
    if args.save_folder and int(os.environ.get('RANK', '0')) == 0:
        save_train_args(args.save_folder, vars(args))
    return args


def run(args):
    """the reference's train(args) (train.py:71-216) -> {'history': fit's rows, 'model', 'optimizer'}"""
    from . import data
    from .model import Model
    from .util import CompoundVAELoss, DiceCoefficient, DiceVAELoss, RegionDiceCoefficient, ScheduledOptim
    if not torch.cuda.is_available():
        raise RuntimeError('python -m bts_amd.train needs a GPU (no CPU fallback exists for the product path)')
    parallel.init_from_env()
    dev = torch.device('cuda', torch.cuda.current_device())        # (init_from_env selected the local rank's)
    if args.resident_gb is None:
        resident = torch.cuda.get_device_properties(dev).total_memory // 4
    else:
        resident = int(args.resident_gb * 1e9)
    sets = []
    targets = getattr(args, 'targets', 'labels')
    spatial, intensity = spatial_config(args), intensity_config(args)
    train_extra = {} if spatial is None else {'spatial': spatial}
    if intensity is not None:
        train_extra['intensity'] = intensity
    foreground = foreground_config(args)
    if foreground is not None:
        train_extra['foreground'] = foreground
    for loc, shuffle, extra in ((args.train_loc, True, train_extra), (args.val_loc, False, {})):
        sets.append(data.prepare_dataset(loc, args.batch_size, args.prepro_size, args.crop_size, args.model_args['out_ch'],
                                         shuffle=shuffle, data_format=args.data_format, seed=args.seed, device=dev,
                                         resident_bytes=resident, workers=args.workers, targets=targets, **extra))
    (train_data, n_train), (val_data, n_val) = sets
    print('{} training examples.'.format(n_train), flush=True)
    print('{} validation examples.'.format(n_val), flush=True)
    model = Model(**args.model_args)
    model.build((1,) + tuple(args.crop_size) + (args.model_args['in_ch'],))
    optimizer = ScheduledOptim(learning_rate=args.lr)              # (n_epochs of the schedule stays 300, as train.py:105 leaves it)
    if args.load_folder:
        load_checkpoint(args.load_folder, model, optimizer)
    if parallel.active():
        parallel.broadcast_parameters(model)
    print('Total number of parameters: {}'.format(int(model.n_params)), flush=True)
    spec = loss_spec(args)
    if spec is None:
        loss_fn = DiceVAELoss(data_format=args.data_format)
        print('Loss: Dice + 0.1 * l2 + 0.1 * kl (the reference\'s).', flush=True)
    else:
        loss_fn = CompoundVAELoss(data_format=args.data_format, spec=spec)
        print('Loss: {} + 0.1 * l2 + 0.1 * kl.'.format(spec.describe()), flush=True)
    dice_fn = (RegionDiceCoefficient if targets == 'regions' else DiceCoefficient)(data_format=args.data_format)
    history = fit(model, optimizer, loss_fn, dice_fn, train_data, val_data, args.n_epochs, patience=args.patience,
                  save_folder=args.save_folder or None, log=lambda s: print(s, flush=True), compute_dtype=args.dtype,
                  eval_dtype=args.dtype)
    return {'history': history, 'model': model, 'optimizer': optimizer}


def main(argv=None):
    args = parse_args(argv)
    print('Train args: {}'.format(args), flush=True)
    ours = not parallel.active()                 # (a group the caller brought up is the caller's to end)
    try:
        run(args)
    finally:
        if ours and parallel.active():
            torch.distributed.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
