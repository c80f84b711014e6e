"""Training the MC-dropout head on cached features, and nested cross-validation down to BISCUIT's thresholds (DESIGN.md section 7
"Head training"): what ``Experiment.train_nested_cv`` and ``thresholds_from_nested_cv`` (``experiment.py:924-1090``) do, for the layers
behind the pooled features only -- Slideflow's ``trainable_layers`` configuration -- with the backbone as imported.

    python -m biscuit_amd.train SLIDE.tfrecords ... --labels CSV --model DIR --out DIR

A cohort's features are computed once (``cache_features``: ``evaluate()``'s input stage, then ``bq_backbone_u8``); each of the
``outer_k * (1 + inner_k)`` trainings then walks that [N, 2048] array on the device (``Engine.head_train_steps``,
``csrc/kernels_train.hip``) and writes its validation table ``tile_predictions_val_epoch1.csv`` with the reference's headers, from
which ``thresholds_from_nested_cv`` takes the thresholds through ``threshold.from_cv`` / ``threshold.apply``.

Augmentation (``--augment xyrjb``, what ``biscuit/hp.py:23`` trains with): ``cache_features(augment=..., views=V)`` also caches V
augmented views of every tile -- ``Engine.augment`` (``bq_augment``, ``csrc/kernels_augment.hip``) with the per-tile draws of
``augment.draw(N, spec, seed, v)`` in front of the stain normaliser -- and epoch ``e`` of a training reads view ``e % V``.
Validation and ``predict`` read the unaugmented features, as Slideflow validates unaugmented.

The reference's schedule (DESIGN.md section 7 "Training schedule"; ``--early-stop``, ``--balance category``, ``--full``): ``fit_head``
scores validation rows every ``validate_on_batch`` steps on the head as it stands (``Engine.head_validate``, ``bq_head_validate``),
``EarlyStop`` ends the training when the smoothed accuracy no longer rises, ``balanced_rows`` draws batches balanced by category,
each fold writes ``results_log.csv``, ``find_cv_early_stop`` reads the folds' stop batches and ``train_full`` trains the model on
every slide for that many steps.  All of it is off by default.

Restated from memory, unpinned against Slideflow: ``TrainParams``' schedule constants and Keras's Adam defaults, the ``k-fold``
split strategy (``kfold``), the directory names, the augmentation's probabilities and order (``augment.py``), the early-stopping
rule and its defaults, and how balanced batches are drawn.

Exit-flow fine-tuning (``--trainable exit``; DESIGN.md section 7 "Exit-flow fine-tuning"): ``cache_activations`` keeps every tile's
``block13_out`` [10, 10, 1024] (``Engine.trunk``; ``--act-cache``: float32 or the engine's own 16-bit form on the device, or pinned
host memory) and each training moves Xception's block 14 together with the head
(``Engine.exit_train_steps``).  Its batch norm runs in one of two modes (``--bn``): ``frozen`` (the default) keeps the imported
moving statistics -- a stated deviation from Slideflow --, ``batch`` is Keras' training mode, as the reference trains: a batch is
normalised by its own statistics, the gradient flows through them and the moving statistics follow the cohort (unpinned).  A fold
then also writes ``exit.npz``; ``exit_engine`` packs the result into an engine.

Out of scope: training blocks 1-13, Slideflow's stain augmentation ``n``, TensorFlow checkpoints, multi-GPU training.
"""
import argparse
import json
import os
from dataclasses import dataclass, field
from statistics import mean
from typing import Optional

import numpy as np

from . import predictions

# the order of the parameter vector the kernels take (include/biscuit_hip.h: bq_head_grad), row-major [K][N]
HEAD_TENSORS = (('hidden_0/kernel', (2048, 1024)), ('hidden_0/bias', (1024,)), ('hidden_1/kernel', (1024, 1024)),
                ('hidden_1/bias', (1024,)), ('logits/kernel', (1024, 2)), ('logits/bias', (2,)))
HEAD_PARAMS = sum(int(np.prod(s)) for _, s in HEAD_TENSORS)            # 3 149 826
# the most rows of one gradient and of one validation check: copies of Engine.HEAD_TRAIN_MAX_ROWS / HEAD_VALIDATE_MAX_ROWS, as
# HEAD_PARAMS is of Engine.HEAD_PARAMS (engine.py loads torch and the library, so neither module imports the other at load)
HEAD_TRAIN_MAX_ROWS, HEAD_VALIDATE_MAX_ROWS = 1024, 4096

# Exit-flow fine-tuning (DESIGN.md section 7 "Exit-flow fine-tuning"): the trainable exit vector's tensors in its order
# (include/biscuit_hip.h: bq_exit_grad), the frozen statistics beside it, and copies of Engine.EXIT_PARAMS / EXIT_MAX_ROWS
_B14 = (('block14_sepconv1', 1024, 1536), ('block14_sepconv2', 1536, 2048))
EXIT_TENSORS = tuple(t for name, cin, cout in _B14 for t in ((f'{name}/depthwise_kernel', (3, 3, cin, 1)), (f'{name}/pointwise_kernel', (1, 1, cin, cout)),
                                                              (f'{name}_bn/gamma', (cout,)), (f'{name}_bn/beta', (cout,))))
EXIT_STATS = tuple(t for name, _, cout in _B14 for t in ((f'{name}_bn/moving_mean', (cout,)), (f'{name}_bn/moving_variance', (cout,))))
EXIT_PARAMS = sum(int(np.prod(s)) for _, s in EXIT_TENSORS)            # 4 748 800
EXIT_MAX_ROWS = 256
ACT_SHAPE = (10, 10, 1024)                   # block13_out of one tile
ACT_BYTES = 4 * int(np.prod(ACT_SHAPE))      # 409 600
TRAINABLE = ('head', 'exit')
BN_MODES = ('frozen', 'batch')
EXIT_FILE = 'exit.npz'

# Keras's Adam defaults and Slideflow's schedule form -- restated from memory, unpinned
ADAM_BETA_1 = 0.9
ADAM_BETA_2 = 0.999
ADAM_EPSILON = 1e-7
LR_STAIRCASE = True

HEAD_FILE = 'head.npz'
MANIFEST_FILE = 'slides.json'
RESULTS_FILE = 'results_log.csv'             # Slideflow's per-model log: what utils.find_cv_early_stop reads

BALANCES = ('none', 'tile', 'slide', 'patient', 'category')
VAL_STREAM = 0x76616c                        # 'val': the stream of the validation rows' order


@dataclass
class TrainParams:
    """The training fields of ``biscuit/hp.py:7-18`` that ``hp.ModelParams`` omits (restated from memory, unpinned where Slideflow
    interprets them: the decay is ``lr * decay ** (step // decay_steps)``, a staircase)."""
    batch_size: int = 128                    # hp.py:7
    epochs: list = field(default_factory=lambda: [1])       # hp.py:8
    optimizer: str = 'Adam'                  # hp.py:14
    learning_rate: float = 1e-4              # hp.py:15
    learning_rate_decay_steps: int = 512     # hp.py:16
    learning_rate_decay: float = 0.98        # hp.py:17
    dropout: float = 0.1                     # hp.py:11
    loss: str = 'sparse_categorical_crossentropy'           # hp.py:18
    augment: str = ''                        # hp.py:23 sets 'xyrjb'; '' trains on the unaugmented features, bit for bit as before
    # The training schedule (DESIGN.md section 7 "Training schedule"), all off by default.  hp.py:9-10 sets early_stop=True with
    # method 'accuracy'; experiment.py:1028-1051 passes validate_on_batch=32, validation_steps=32; the other defaults are Slideflow's,
    # restated from memory, unpinned.
    early_stop: bool = False                 # hp.py:9
    early_stop_method: str = 'accuracy'      # hp.py:10; or 'loss'
    early_stop_patience: int = 0             # epochs before the rule may fire
    ema_observations: int = 20
    ema_smoothing: float = 2
    validate_on_batch: int = 32              # a check every so many steps of an epoch
    validation_steps: int = 32               # batches of validation rows per check
    validation_dropout: bool = False         # True: a check draws the training masks; False: inference mode
    training_balance: str = 'none'           # or 'tile' (the same), 'slide', 'patient', 'category'
    steps_per_epoch_override: Optional[int] = None
    # 'head': the three dense layers on cached features; 'exit': block 14 with them, on cached block13_out (an ActivationCache), under
    # one Adam and one learning rate, batch-norm statistics frozen (DESIGN.md section 7 "Exit-flow fine-tuning"; unpinned)
    trainable: str = 'head'
    # block 14's batch norm under trainable='exit' (DESIGN.md section 7 "Exit-flow fine-tuning", Two modes): 'frozen' keeps the imported
    # moving statistics; 'batch' is Keras' training mode -- batch statistics, gradients through them, moving statistics updated
    bn: str = 'frozen'

    @classmethod
    def nature2022(cls, **fields):
        """The reference's schedule: early stopping by accuracy, batches balanced by category (Slideflow's default)."""
        return cls(**{'early_stop': True, 'early_stop_method': 'accuracy', 'training_balance': 'category', **fields})

    def _check_bn(self):
        if self.bn not in BN_MODES or (self.bn == 'batch' and self.trainable != 'exit'):
            raise ValueError(f"bn is one of {BN_MODES}, and 'batch' goes with trainable='exit' only (the head has no batch norm)")

    def __post_init__(self):
        self._check_bn()                     # at construction already; validate() asks again, the fields being mutable

    def validate(self):
        from . import augment as A
        A.parse(self.augment)
        if self.optimizer != 'Adam' or self.loss != 'sparse_categorical_crossentropy':
            raise ValueError('the head trainer implements Adam on sparse categorical cross-entropy only')
        if not 1 <= int(self.batch_size) <= HEAD_TRAIN_MAX_ROWS or not self.epochs or min(self.epochs) < 1:
            raise ValueError(f'1 <= batch_size <= {HEAD_TRAIN_MAX_ROWS} and at least one epoch')
        if not 0.0 <= self.dropout < 1.0 or not self.learning_rate > 0 or self.learning_rate_decay_steps < 1:
            raise ValueError('dropout in [0, 1), a positive learning rate and decay steps >= 1')
        if self.early_stop_method not in ('accuracy', 'loss') or self.training_balance not in BALANCES:
            raise ValueError(f"early_stop_method is 'accuracy' or 'loss', training_balance one of {BALANCES}")
        if int(self.early_stop_patience) < 0 or int(self.ema_observations) < 1 or not self.ema_smoothing > 0:
            raise ValueError('early_stop_patience >= 0, ema_observations >= 1 and ema_smoothing > 0')
        if int(self.validate_on_batch) < 1 or int(self.validation_steps) < 1:
            raise ValueError('validate_on_batch >= 1 and validation_steps >= 1')
        if self.early_stop and int(self.validation_steps) * int(self.batch_size) > HEAD_VALIDATE_MAX_ROWS:
            raise ValueError(f'a check scores validation_steps x batch_size rows, at most {HEAD_VALIDATE_MAX_ROWS}')
        if self.steps_per_epoch_override is not None and int(self.steps_per_epoch_override) < 1:
            raise ValueError('steps_per_epoch_override is None or at least 1')
        if self.trainable not in TRAINABLE:
            raise ValueError(f'trainable is one of {TRAINABLE}, not {self.trainable!r}')
        if self.trainable == 'exit' and (int(self.batch_size) > EXIT_MAX_ROWS or self.validation_dropout):
            raise ValueError(f"trainable='exit': batch_size <= {EXIT_MAX_ROWS}, and validation in inference mode only")
        self._check_bn()
        return self

    def learning_rate_at(self, step):
        """The learning rate of global step ``step`` (0-based), float64."""
        e = step // self.learning_rate_decay_steps if LR_STAIRCASE else step / self.learning_rate_decay_steps
        return float(self.learning_rate) * float(self.learning_rate_decay) ** e


def flatten_head(w):
    """The six head tensors of a weight dict -> one float32 vector [P] in ``HEAD_TENSORS`` order."""
    parts = []
    for name, shape in HEAD_TENSORS:
        a = np.asarray(w[name], np.float32)
        if a.shape != shape:
            raise ValueError(f'{name}: shape {a.shape}, not {shape}')
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def unflatten_head(vec):
    """A vector [P] -> ``{name: float32 array}`` of the six head tensors (copies)."""
    vec = np.asarray(vec, np.float32).reshape(-1)
    if vec.size != HEAD_PARAMS:
        raise ValueError(f'a head has {HEAD_PARAMS} parameters, not {vec.size}')
    out, at = {}, 0
    for name, shape in HEAD_TENSORS:
        n = int(np.prod(shape))
        out[name] = vec[at:at + n].reshape(shape).copy()
        at += n
    return out


def flatten_exit(w):
    """Block 14's eight trainable tensors of a weight dict -> one float32 vector [P_EXIT] in ``EXIT_TENSORS`` order (the Keras
    shapes are the vector's own layout: D [3][3][C], P [Cin][Cout])."""
    parts = []
    for name, shape in EXIT_TENSORS:
        a = np.asarray(w[name], np.float32)
        if a.shape != shape:
            raise ValueError(f'{name}: shape {a.shape}, not {shape}')
        parts.append(a.reshape(-1))
    return np.concatenate(parts)


def unflatten_exit(vec):
    """A vector [P_EXIT] -> ``{name: float32 array}`` of block 14's eight trainable tensors in their Keras shapes (copies)."""
    vec = np.asarray(vec, np.float32).reshape(-1)
    if vec.size != EXIT_PARAMS:
        raise ValueError(f'the exit vector has {EXIT_PARAMS} parameters, not {vec.size}')
    out, at = {}, 0
    for name, shape in EXIT_TENSORS:
        n = int(np.prod(shape))
        out[name] = vec[at:at + n].reshape(shape).copy()
        at += n
    return out


def exit_bn_stats(w):
    """Block 14's moving statistics of a weight dict -> float32 [7168]: mean1, variance1, mean2, variance2."""
    parts = []
    for name, shape in EXIT_STATS:
        a = np.asarray(w[name], np.float32)
        if a.shape != shape:
            raise ValueError(f'{name}: shape {a.shape}, not {shape}')
        parts.append(a)
    return np.concatenate(parts)


def unflatten_exit_stats(vec):
    """A vector [7168] -> ``{name: float32 array}`` of block 14's four moving-statistics tensors (copies)."""
    vec = np.asarray(vec, np.float32).reshape(-1)
    if vec.size != sum(s[0] for _, s in EXIT_STATS):
        raise ValueError(f'block 14 has {sum(s[0] for _, s in EXIT_STATS)} moving statistics, not {vec.size}')
    out, at = {}, 0
    for name, shape in EXIT_STATS:
        out[name] = vec[at:at + shape[0]].copy()
        at += shape[0]
    return out


def has_exit_stats(tensors):
    """Whether ``tensors`` is a trained block 14 that carries its own moving statistics (``bn='batch'``): all four of them -- or
    none: ValueError for some -- and nothing but block 14's twelve tensors.  A whole model's weight dict is not such a result: its
    block 14 is saved and read as before there were two modes, eight tensors under the engine's statistics."""
    have = [name in tensors for name, _ in EXIT_STATS]
    if any(have) and not all(have):
        raise ValueError('a block 14 carries all four moving statistics or none')
    return all(have) and set(tensors) <= {name for name, _ in EXIT_TENSORS + EXIT_STATS}


def save_exit(path, tensors):
    """``exit.npz``: block 14's eight trained tensors, and its four moving statistics where ``tensors`` has them (``bn='batch'``)."""
    names = EXIT_TENSORS + (EXIT_STATS if has_exit_stats(tensors) else ())
    np.savez(path, **{name: np.asarray(tensors[name], np.float32) for name, _ in names})


def load_exit(path):
    """``save_exit``'s file -> its tensors: eight, or twelve where the file holds the moving statistics."""
    with np.load(path) as z:
        names = EXIT_TENSORS + (EXIT_STATS if has_exit_stats(z.files) else ())
        return {name: z[name] for name, _ in names}


def glorot_head(seed):
    """A seeded Glorot-uniform head, drawn on the host: kernels U(-l, l) with l = sqrt(6 / (fan_in + fan_out)), zero biases."""
    rng = np.random.default_rng([int(seed), 0x676c6f72])
    out = {}
    for name, shape in HEAD_TENSORS:
        if name.endswith('/kernel'):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            out[name] = rng.uniform(-lim, lim, shape).astype(np.float32)
        else:
            out[name] = np.zeros(shape, np.float32)
    return out


def save_head(path, head):
    np.savez(path, **{name: np.asarray(head[name], np.float32) for name, _ in HEAD_TENSORS})


def load_head(path):
    with np.load(path) as z:
        return {name: z[name] for name, _ in HEAD_TENSORS}


# ------------------------------------------------------------------------------------------------------------ feature cache
@dataclass
class FeatureCache:
    """A cohort's pooled features: ``feats`` float32 [N, 2048] (a device tensor; a host array once loaded, until ``to``), per tile
    ``slide_idx`` int64 [N] into ``slides`` (names, in dataset order) and ``loc`` int64 [N, 2].  A tile's row is its index in the
    cohort's tile list: its Philox tile counter in ``evaluate()``, in ``predict`` and in training.  ``views``: None, or float32
    [V, N, 2048] beside ``feats`` -- the features of V augmented views of every tile, which only training reads -- with ``augment``
    (the letters) and ``augment_seed`` that drew them."""
    feats: object
    slide_idx: np.ndarray
    loc: np.ndarray
    slides: list
    views: object = None
    augment: str = ''
    augment_seed: int = 0

    def __len__(self):
        return len(self.slide_idx)

    def rows_of(self, slides):
        """The rows of the named slides, ascending."""
        want = np.zeros(len(self.slides), bool)
        index = {s: i for i, s in enumerate(self.slides)}
        for s in slides:
            want[index[s]] = True
        return np.flatnonzero(want[self.slide_idx]).astype(np.int64)

    def to(self, device):
        import torch
        on = lambda a: torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(device).contiguous()
        self.feats = on(self.feats)
        if self.views is not None:
            self.views = on(self.views)
        return self

    def n_views(self):
        return 0 if self.views is None else int(self.views.shape[0])

    def save(self, path):
        host = lambda a: (a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)).astype(np.float32)
        extra = {} if self.views is None else {'views': host(self.views), 'augment': np.array(self.augment),
                                               'augment_seed': np.array(int(self.augment_seed), np.int64)}
        np.savez(path, feats=host(self.feats), slide_idx=self.slide_idx, loc=self.loc, slides=np.array(self.slides, dtype=str), **extra)

    @staticmethod
    def load(path, device=None):
        with np.load(path) as z:
            c = FeatureCache(z['feats'].astype(np.float32), z['slide_idx'].astype(np.int64), z['loc'].astype(np.int64),
                             [str(s) for s in z['slides']])
            if 'views' in z.files:
                c.views, c.augment, c.augment_seed = z['views'].astype(np.float32), str(z['augment']), int(z['augment_seed'])
        return c.to(device) if device is not None else c


def view_count(letters, views, default=1):
    """The augmented views cached per tile: none without augmentation, else ``views``, ``default`` of them when that is None."""
    return (default if views is None else int(views)) if letters else 0


def cache_features(engine_or_pool, slides, *, normalizer='reinhard_fast', norm_fit=None, batch=256, augment=None, views=None, seed=0):
    """Every tile of ``slides`` through ``evaluate()``'s input stage -- decode, stain normaliser, ``bq_backbone_u8``
    (``featuremap.walk_features``) -> ``FeatureCache`` with the features on the engine's device.  ``augment`` (letters out of
    'xyrjb'; None / '': none) also fills ``views`` [V, N, 2048], V = ``views`` (pass ``max(epochs)``; default 1): view v is every
    tile through ``Engine.augment`` with row ``augment.draw(N, augment, seed, v)[its row]`` in front of the normaliser, computed
    from the same decoded batch as the unaugmented features, which stay exactly what they are without ``augment``.  A tile whose
    JPEG round trip reports its range status raises ``BiscuitHipError``."""
    import torch
    from . import augment as A
    from .featuremap import walk_features
    eng = engine_or_pool.engines[0] if hasattr(engine_or_pool, 'engines') else engine_or_pool
    parts = []
    letters = A.parse(augment)
    V = view_count(letters, views)
    if letters and V < 1:
        raise ValueError('views must be at least 1')
    prepare, view_parts, statuses = None, [[] for _ in range(V)], []
    if V:
        from . import stain
        n_total = sum(int(s.n_tiles) for s in slides)
        tables = [torch.from_numpy(A.draw(n_total, letters, seed, v)).to(eng.device) for v in range(V)]

        def prepare(tiles, g):
            for v in range(V):
                aug, status = eng.augment(tiles, tables[v].index_select(0, g).contiguous())
                view_parts[v].append(eng.backbone_u8(stain.normalise(eng, aug, normalizer, norm_fit)))
                statuses.append(status)
            return tiles
    names, _, loc, _ = walk_features(eng, slides, 0, lambda f, g: parts.append(f), norm_fit, normalizer, False, batch, prepare=prepare)
    feats = torch.cat(parts) if parts else torch.zeros((0, 2048), dtype=torch.float32, device=eng.device)
    if statuses and bool(torch.cat(statuses).ne(0).any()):
        from .engine import BiscuitHipError
        raise BiscuitHipError('cache_features: the augmenter reported a tile outside the JPEG round trip\'s exact range')
    stacked = None
    if V:
        stacked = torch.stack([torch.cat(p) if p else torch.zeros((0, 2048), dtype=torch.float32, device=eng.device) for p in view_parts]).contiguous()
    order = [s.name for s in slides]
    index = {s: i for i, s in enumerate(order)}
    if len(index) != len(order):
        raise ValueError('slide names must be unique')
    return FeatureCache(feats.contiguous(), np.array([index[n] for n in names], np.int64), loc, order, stacked, letters, int(seed) if V else 0)


def cached_features(engine, slides, path, *, augment=None, views=None, seed=0, activations=False, store='f32', **kw):
    """``--cache FILE``: ``cache_features(engine, slides, augment=..., views=..., seed=..., **kw)``, kept in ``path`` (.npz; None: not
    kept) -- loaded from there when the file exists, with its views, otherwise computed and saved.  SystemExit for a file that holds
    other slides or was made with another augmentation, number of views or seed.  ``activations`` (``--trainable exit``): an
    ``ActivationCache`` through ``cache_activations`` instead, built under ``store`` (``--act-cache``), and SystemExit for a file
    without activations; a file that exists keeps the form it was saved in, and goes to pinned host memory for ``store='host'``."""
    from . import augment as A
    letters = A.parse(augment)
    n_views = view_count(letters, views)
    if not path or not os.path.exists(path):
        try:
            if activations:
                kw = dict(kw, store=store)
            cache = (cache_activations if activations else cache_features)(engine, slides, augment=letters, views=n_views or None, seed=seed, **kw)
        except ValueError as e:
            if not activations:
                raise
            raise SystemExit(str(e)) from None
        if path:
            cache.save(path)
        return cache
    try:
        cache = ActivationCache.load(path, engine.device, host=store == 'host') if activations else FeatureCache.load(path, engine.device)
    except ValueError as e:
        raise SystemExit(f'--cache {e}') from None
    if cache.slides != [s.name for s in slides] or len(cache) != sum(int(s.n_tiles) for s in slides):
        raise SystemExit(f'--cache {path}: holds other slides than the ones given')
    if (cache.augment, cache.n_views()) != (letters, n_views) or (letters and cache.augment_seed != int(seed)):
        raise SystemExit(f'--cache {path}: made with augment {cache.augment!r}, {cache.n_views()} view(s), seed {cache.augment_seed}, '
                         f'not with {letters!r}, {n_views}, {int(seed)}')
    return cache


# ------------------------------------------------------------------------------------------------------------ activation cache
ACT_STORES = ('f32', 'packed', 'host', 'auto')      # --act-cache (DESIGN.md section 7 "Exit-flow fine-tuning", Sizes)
ACT_TORCH = {'f16': 'float16', 'bf16': 'bfloat16', 'f32': 'float32'}


def _acts_to_numpy(a):
    """An activation tensor or array -> ``(numpy array, type name)``; bfloat16, which numpy lacks, as its raw ``uint16``."""
    import torch
    if not torch.is_tensor(a):
        a = np.asarray(a)
        return (a, 'f16') if a.dtype == np.float16 else (a.astype(np.float32), 'f32')
    a = a.detach().cpu()
    if a.dtype == torch.bfloat16:
        return a.contiguous().view(torch.int16).numpy().view(np.uint16), 'bf16'
    return a.numpy(), ('f16' if a.dtype == torch.float16 else 'f32')


def _acts_from_numpy(a, act_type):
    """``_acts_to_numpy``'s inverse: float32 stays the numpy array it always was; the 16-bit forms become host tensors of their type."""
    import torch
    if act_type == 'f32':
        return a.astype(np.float32)
    if act_type == 'bf16':
        return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.bfloat16)
    if act_type == 'f16':
        return torch.from_numpy(np.ascontiguousarray(a, np.float16))
    raise ValueError(f'act_type {act_type!r} is none of f32, f16, bf16')


@dataclass
class ActivationCache(FeatureCache):
    """A ``FeatureCache`` that also holds what block 14 reads: ``acts`` [N, 10, 10, 1024] (``block13_out`` per tile; a host array
    once loaded, until ``to``) and, with augmentation, ``act_views`` [V, N, 10, 10, 1024] beside ``views``.  ``feats`` / ``views``
    are ``Engine.exit_features`` of them under the imported block 14, so everything that reads a ``FeatureCache`` works on it
    unchanged; ``trainable='exit'`` trains on ``acts``.  The activations are float32 on the device (``store='f32'``), the engine's
    own 16-bit type on the device (``'packed'``), or either in pinned host memory (``'host'``); a 16-bit tensor holds the engine's
    stored values and ``act_mul``, a power of two, takes them to the network's: ``acts.float() * act_mul`` is the float32 cache
    exactly, so whatever is computed from any form has the same bits."""
    acts: object = None
    act_views: object = None
    act_mul: float = 1.0

    def to(self, device):
        """Features to ``device``; the activations too, in their own type -- unless they lie in pinned host memory, where they stay."""
        import torch

        def on(a):
            t = torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
            return t if (not t.is_cuda and t.is_pinned()) else t.to(device).contiguous()
        FeatureCache.to(self, device)
        self.acts = on(self.acts)
        if self.act_views is not None:
            self.act_views = on(self.act_views)
        return self

    def pin(self):
        """The activations into pinned host memory, in their own type (``store='host'`` of a cache that was loaded)."""
        import torch
        pinned = lambda a: a if (not a.is_cuda and a.is_pinned()) else torch.empty(a.shape, dtype=a.dtype, pin_memory=True).copy_(a)
        tensor = lambda a: torch.as_tensor(np.asarray(a)) if not torch.is_tensor(a) else a
        self.acts = pinned(tensor(self.acts))
        if self.act_views is not None:
            self.act_views = pinned(tensor(self.act_views))
        return self

    def save(self, path):
        host = lambda a: (a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)).astype(np.float32)
        acts, act_type = _acts_to_numpy(self.acts)
        extra = {} if self.views is None else {'views': host(self.views), 'act_views': _acts_to_numpy(self.act_views)[0],
                                               'augment': np.array(self.augment), 'augment_seed': np.array(int(self.augment_seed), np.int64)}
        if act_type != 'f32':        # a float32 cache is the file it always was
            extra.update(act_type=np.array(act_type), act_mul=np.array(float(self.act_mul), np.float64))
        np.savez(path, feats=host(self.feats), acts=acts, slide_idx=self.slide_idx, loc=self.loc,
                 slides=np.array(self.slides, dtype=str), **extra)

    @staticmethod
    def load(path, device=None, host=False):
        """``host``: the activations into pinned host memory (``pin``) instead of onto ``device``."""
        with np.load(path) as z:
            if 'acts' not in z.files:
                raise ValueError(f'{path}: a feature cache, not an activation cache (no acts)')
            act_type = str(z['act_type']) if 'act_type' in z.files else 'f32'
            c = ActivationCache(z['feats'].astype(np.float32), z['slide_idx'].astype(np.int64), z['loc'].astype(np.int64),
                                [str(s) for s in z['slides']], acts=_acts_from_numpy(z['acts'], act_type),
                                act_mul=float(z['act_mul']) if 'act_mul' in z.files else 1.0)
            if 'views' in z.files:
                c.views, c.act_views = z['views'].astype(np.float32), _acts_from_numpy(z['act_views'], act_type)
                c.augment, c.augment_seed = str(z['augment']), int(z['augment_seed'])
        if host:
            c.pin()
        return c.to(device) if device is not None else c


def act_row_bytes(store='f32', dtype='f16'):
    """The bytes one tile's activations take under ``store``: 409 600 as float32, 204 800 in a 16-bit engine's own type; ``'host'``
    keeps the 16-bit form of a 16-bit engine (``dtype``) and float32 of an f32 one.  ValueError for ``'packed'`` on an f32 engine."""
    if store not in ('f32', 'packed', 'host'):
        raise ValueError(f'store is one of {ACT_STORES}, not {store!r}')
    if dtype not in ACT_TORCH:
        raise ValueError(f'dtype is one of {sorted(ACT_TORCH)}, not {dtype!r}')
    if store == 'packed' and dtype == 'f32':
        raise ValueError("store='packed' keeps block13_out as the engine stores it, in 16 bits: an f32 engine stores it in 32, so a "
                         "16-bit cache would not be lossless (use --act-cache f32 or host, or a 16-bit engine)")
    return ACT_BYTES if store == 'f32' or dtype == 'f32' else ACT_BYTES // 2


def activation_cache_bytes(n_tiles, views=0, store='f32', dtype='f16'):
    """The bytes of an ``ActivationCache``'s activations: ``n_tiles x act_row_bytes(store, dtype) x (1 + views)`` -- 409 600 per
    tile and view as float32 -- on the device, or for ``'host'`` in pinned host memory."""
    return int(n_tiles) * act_row_bytes(store, dtype) * (1 + int(views))


def check_activation_memory(n_tiles, views, free_bytes, store='f32', dtype='f16'):
    """ValueError naming both figures when the activations of ``n_tiles`` tiles and ``views`` views under ``store`` do not fit
    ``free_bytes`` -- the device's, or for ``'host'`` the host's."""
    need = activation_cache_bytes(n_tiles, views, store, dtype)
    if need > int(free_bytes):
        where, other = ('the host', 'fewer tiles, fewer views') if store == 'host' else \
            ('the device', ('--act-cache packed (half the bytes, on a 16-bit engine) or ' if store == 'f32' else '') +
             '--act-cache host (pinned host memory, gathered per step)')
        raise ValueError(f'cache_activations: {int(n_tiles)} tiles x {act_row_bytes(store, dtype)} bytes x (1 + {int(views)} views) = {need} '
                         f'bytes of activations, but {where} has {int(free_bytes)} bytes free ({other}, or --trainable head)')
    return need


def choose_act_store(store, dtype, n_tiles, views, free_bytes, host_free=None):
    """The store ``cache_activations`` builds -> ``'f32'``, ``'packed'`` or ``'host'``.  ``'auto'`` takes the first of float32 on the
    device, packed on the device (a 16-bit engine's only) and host that fits -- ``free_bytes`` of the device, ``host_free`` of the
    host (None: not looked at) -- and the others are themselves; ValueError from ``act_row_bytes`` / ``check_activation_memory``
    for ``'packed'`` on an f32 engine and for a store that does not fit."""
    if store not in ACT_STORES:
        raise ValueError(f'store is one of {ACT_STORES}, not {store!r}')
    if store == 'auto':
        fits = lambda st: activation_cache_bytes(n_tiles, views, st, dtype) <= int(free_bytes)
        store = 'f32' if fits('f32') else 'packed' if dtype != 'f32' and fits('packed') else 'host'
    check_activation_memory(n_tiles, views, free_bytes if store != 'host' else (1 << 62 if host_free is None else host_free), store, dtype)
    return store


def host_free_bytes():
    """The host's available physical memory, None where the system does not say."""
    try:
        return int(os.sysconf('SC_AVPHYS_PAGES')) * int(os.sysconf('SC_PAGE_SIZE'))
    except (ValueError, OSError, AttributeError):
        return None


def cache_activations(engine_or_pool, slides, *, normalizer='reinhard_fast', norm_fit=None, batch=256, augment=None, views=None, seed=0,
                      store='f32'):
    """``cache_features``' walk with ``Engine.trunk`` in the place of ``backbone_u8`` -> ``ActivationCache``: every tile's
    ``block13_out`` (and V augmented views of it, drawn as ``cache_features`` draws them), and the features
    ``Engine.exit_features`` gives them under the engine's imported block 14.  ``store`` (``ACT_STORES``): ``'f32'`` keeps float32
    on the engine's device; ``'packed'`` the engine's own 16-bit tensor (``trunk(packed=True)``) there, half the bytes and the same
    numbers; ``'host'`` that form -- float32 on an f32 engine -- in pinned host memory, each batch copied out asynchronously behind
    the trunk; ``'auto'`` the first of the three that fits (``choose_act_store``; logged).  Before anything is read the activations'
    bytes are compared with the free memory of their place (``check_activation_memory``)."""
    import torch
    from . import augment as A
    from .featuremap import walk_features
    eng = engine_or_pool.engines[0] if hasattr(engine_or_pool, 'engines') else engine_or_pool
    letters = A.parse(augment)
    V = view_count(letters, views)
    if letters and V < 1:
        raise ValueError('views must be at least 1')
    order = [s.name for s in slides]
    index = {s: i for i, s in enumerate(order)}
    if len(index) != len(order):
        raise ValueError('slide names must be unique')
    n_total = sum(int(s.n_tiles) for s in slides)
    asked, store = store, choose_act_store(store, eng.dtype, n_total, V, torch.cuda.mem_get_info(eng.device)[0], host_free_bytes())
    if asked == 'auto':
        import logging
        logging.getLogger(__name__).info('cache_activations: --act-cache auto took %r (%d bytes)', store,
                                         activation_cache_bytes(n_total, V, store, eng.dtype))
    packed = store != 'f32' and eng.dtype != 'f32'
    place = dict(pin_memory=True) if store == 'host' else dict(device=eng.device)
    elt = getattr(torch, ACT_TORCH[eng.dtype]) if packed else torch.float32
    acts = torch.empty((n_total,) + ACT_SHAPE, dtype=elt, **place)
    act_views = torch.empty((V, n_total) + ACT_SHAPE, dtype=elt, **place) if V else None
    muls, at = set(), [0] * (V + 1)

    def trunk(tiles):
        if not packed:
            return eng.trunk(tiles)
        a, mul = eng.trunk(tiles, packed=True)
        muls.add(mul)
        return a

    def keep(dst, k, g, a):
        """Batch ``a`` of the walk into ``dst``: at its indices on the device; into host memory behind the batches before it --
        the walk hands out every tile in order, so the indices are the next ``len(a)`` -- as one asynchronous copy."""
        if store == 'host':
            dst[at[k]:at[k] + len(a)].copy_(a, non_blocking=True)
            at[k] += len(a)
        else:
            dst.index_copy_(0, g, a)
    prepare, statuses = None, []
    if V:
        from . import stain
        tables = [torch.from_numpy(A.draw(n_total, letters, seed, v)).to(eng.device) for v in range(V)]

        def prepare(tiles, g):
            for v in range(V):
                aug, status = eng.augment(tiles, tables[v].index_select(0, g).contiguous())
                keep(act_views[v], v + 1, g, trunk(stain.normalise(eng, aug, normalizer, norm_fit)))
                statuses.append(status)
            return tiles
    names, _, loc, _ = walk_features(eng, slides, 0, lambda a, g: keep(acts, 0, g, a), norm_fit, normalizer, False, batch,
                                     prepare=prepare, stage=trunk)
    assert store != 'host' or all(k == n_total for k in at), (at, n_total)
    if statuses and bool(torch.cat(statuses).ne(0).any()):
        from .engine import BiscuitHipError
        raise BiscuitHipError('cache_activations: the augmenter reported a tile outside the JPEG round trip\'s exact range')
    assert len(muls) <= 1, muls
    mul = muls.pop() if muls else 1.0
    e = torch.from_numpy(flatten_exit(eng.weights)).to(eng.device)
    stats = torch.from_numpy(exit_bn_stats(eng.weights)).to(eng.device)
    every = torch.arange(n_total, dtype=torch.int64, device=eng.device)
    feats = eng.exit_features_all(e, stats, acts, every, act_mul=mul) if n_total else torch.zeros((0, 2048), dtype=torch.float32, device=eng.device)
    stacked = None
    if V:
        stacked = torch.stack([eng.exit_features_all(e, stats, act_views[v], every, act_mul=mul) for v in range(V)]).contiguous() if n_total else \
            torch.zeros((V, 0, 2048), dtype=torch.float32, device=eng.device)
    return ActivationCache(feats.contiguous(), np.array([index[n] for n in names], np.int64), loc, order, stacked, letters,
                           int(seed) if V else 0, acts=acts, act_views=act_views, act_mul=mul)


# ------------------------------------------------------------------------------------------------------------ the schedule
class EarlyStop:
    """Slideflow's early-stopping rule over the values of successive validation checks (restated from memory, unpinned; DESIGN.md
    section 7 "Training schedule" is the definition).  The first ``ema_observations`` values are collected, and their mean seeds the
    moving average ``ema`` when the last of them arrives (None until then); from then on ``ema = value k + ema (1 - k)`` with
    ``k = ema_smoothing / (1 + ema_observations)``.  After every check the averages shift, ``two <- one <- ema``.  ``update`` says
    stop when ``epoch >= patience``, the average of two checks back exists and the new one has not improved on it: ``ema <= two``
    for ``'accuracy'``, ``ema >= two`` for ``'loss'``."""

    def __init__(self, method='accuracy', patience=0, ema_observations=20, ema_smoothing=2):
        if method not in ('accuracy', 'loss') or int(ema_observations) < 1:
            raise ValueError("method is 'accuracy' or 'loss', ema_observations at least 1")
        self.method, self.patience, self.observations = method, int(patience), int(ema_observations)
        self.k = float(ema_smoothing) / (1 + self.observations)
        self.values, self.ema, self.one, self.two = [], None, None, None

    @classmethod
    def of(cls, params):
        return cls(params.early_stop_method, params.early_stop_patience, params.ema_observations, params.ema_smoothing)

    def update(self, value, epoch):
        value = float(value)
        if self.ema is None:
            self.values.append(value)
            if len(self.values) >= self.observations:
                self.ema = float(np.mean(self.values))
        else:
            self.ema = value * self.k + self.ema * (1 - self.k)
        stop = self.ema is not None and self.two is not None and int(epoch) >= self.patience and \
            (self.ema <= self.two if self.method == 'accuracy' else self.ema >= self.two)
        self.two, self.one = self.one, self.ema
        return bool(stop)


def epoch_order(count, n, seed, epoch):
    """The first ``n`` entries of an epoch's stream of positions 0 .. count - 1: ``default_rng([seed, epoch]).permutation(count)``
    -- the whole of it for n = count, as ``train_head`` always walked -- continued past its end with the permutations of
    ``default_rng([seed, epoch, k])``, k = 1, 2, ..."""
    parts, k = [], 0
    while k * count < n:
        parts.append(np.random.default_rng([int(seed), int(epoch)] + ([k] if k else [])).permutation(int(count)))
        k += 1
    return np.concatenate(parts)[:int(n)] if parts else np.zeros(0, np.int64)


def slide_probabilities(slide_idx, labels, patients, balance):
    """``(slides, p)``: the distinct values of ``slide_idx``, ascending, and the probability with which a balanced draw picks each.
    ``'category'``: every class equally likely and its slides equally likely within it (a slide's class is its first row's label);
    ``'slide'``: every slide equally likely; ``'patient'``: every patient equally likely and their slides equally likely within them
    (``patients``: a patient per row; None: every slide is its own patient)."""
    slides, first = np.unique(slide_idx, return_index=True)
    if balance == 'slide' or (balance == 'patient' and patients is None):
        return slides, np.full(len(slides), 1.0 / len(slides))
    if balance == 'category':
        group = np.asarray(labels)[first]
    elif balance == 'patient':
        group = np.asarray(patients)[first]
    else:
        raise ValueError(f"a balanced draw is by 'slide', 'patient' or 'category', not {balance!r}")
    _, inverse, counts = np.unique(group, return_inverse=True, return_counts=True)
    return slides, 1.0 / (len(counts) * counts[inverse].astype(np.float64))


def balanced_rows(rows, slide_idx, labels, patients, balance, n, seed, epoch, state=None):
    """``n`` draws for epoch ``epoch`` -> int64 [n] positions into ``rows`` (``slide_idx``, ``labels`` and ``patients`` hold one
    entry per row).  ``'none'`` and ``'tile'`` are ``epoch_order(len(rows), n, seed, epoch)``.  Otherwise each draw first picks a
    slide with the fixed probability of ``slide_probabilities`` -- ``default_rng([seed, epoch, 0x62616c]).choice`` -- and then takes
    that slide's next tile from the slide's own permutation ``default_rng([seed, 0x74696c, slide]).permutation``, walked cyclically:
    no tile of a slide repeats before all its tiles were drawn.  ``state`` (a dict, changed in place; None: a fresh walk) carries
    every slide's offset from one epoch to the next."""
    if balance in ('none', 'tile'):
        return epoch_order(len(rows), n, seed, epoch)
    slide_idx = np.asarray(slide_idx, np.int64).reshape(-1)
    if len(slide_idx) != len(rows) or len(np.asarray(labels).reshape(-1)) != len(rows) or len(rows) < 1:
        raise ValueError('balanced_rows: a slide and a label for each of at least one row')
    slides, p = slide_probabilities(slide_idx, labels, patients, balance)
    picks = np.random.default_rng([int(seed), int(epoch), 0x62616c]).choice(len(slides), size=int(n), p=p)
    state = {} if state is None else state
    out = np.empty(int(n), np.int64)
    for j, s in enumerate(slides):
        mine = np.flatnonzero(picks == j)
        if not len(mine):
            continue
        at = np.flatnonzero(slide_idx == s)
        walk = at[np.random.default_rng([int(seed), 0x74696c, int(s)]).permutation(len(at))]
        start = int(state.get(int(s), 0))
        out[mine] = walk[(start + np.arange(len(mine))) % len(at)]
        state[int(s)] = (start + len(mine)) % len(at)
    return out


@dataclass
class FitResult:
    """What ``fit_head`` returns: the head tensor dict, the training losses float32 [steps], ``checks`` -- ``(step, val_loss,
    val_acc, ema)`` per validation check, ``step`` the steps done by then, ``ema`` None before it is seeded --, ``early_stop_batch``
    (the steps done when the rule fired; None if it never did), the steps done in all and the epochs it was trained under
    (``max(params.epochs)``: what ``results_log.csv`` names the model by)."""
    head: dict
    losses: np.ndarray
    checks: list
    early_stop_batch: Optional[int]
    steps: int
    epochs: int = 1
    exit: Optional[dict] = None              # trainable='exit': block 14's eight trained tensors; bn='batch': and its four moving statistics


# ------------------------------------------------------------------------------------------------------------ training
def _rows_and_labels(cache, rows, labels, bad_labels, bad_rows):
    """``(rows int64 [n], labels [n])`` of a training or validation set, n >= 1; ValueError with the caller's texts otherwise."""
    rows, labels = np.asarray(rows, np.int64).reshape(-1), np.asarray(labels).reshape(-1)
    if len(rows) < 1 or len(labels) != len(rows) or not np.isin(labels, (0, 1)).all():
        raise ValueError(bad_labels)
    if rows.min() < 0 or rows.max() >= len(cache):
        raise ValueError(bad_rows)
    return rows, labels


def _plan_epoch(p, cache, rows, labels, slide_idx, patients, seed, epoch, state):
    """One epoch's batches end to end -> ``(at int64: rows of the features ``fit_head`` trains on, y uint8)``."""
    draws = len(rows) if p.steps_per_epoch_override is None else int(p.steps_per_epoch_override) * int(p.batch_size)
    order = balanced_rows(rows, slide_idx, labels, patients, p.training_balance, draws, seed, epoch, state)
    return rows[order] + (epoch % (cache.n_views() or 1)) * len(cache), labels[order].astype(np.uint8)


def fit_head(engine, cache, rows, labels, *, val_rows=None, val_labels=None, slide_idx=None, patients=None, init='model', params=None,
             seed=None):
    """Train the head on ``cache.feats[rows]`` with ``labels`` (0/1 per row) under ``params``' schedule -> ``FitResult``.
    ``init='model'`` starts from the engine's imported head, ``'glorot'`` from ``glorot_head(seed)`` (a dict starts from that).

    An epoch is ``ceil(len(rows) / batch_size)`` steps over ``len(rows)`` draws, the last batch short, or exactly
    ``steps_per_epoch_override`` full batches; the draws are ``balanced_rows`` (``slide_idx``: the slide of each row, default the
    cache's; ``patients``: a patient per row, for ``'patient'``), which without balancing is the permutation of
    ``default_rng([seed, epoch])``.  The dropout pass counter is the global step.  A cache with ``views`` [V, N, 2048] trains epoch
    ``e`` on view ``e % V``: the views are read as one [V N, 2048] array at rows ``rows + (e % V) N``.

    With ``val_rows`` / ``val_labels`` an epoch runs as segments of ``validate_on_batch`` steps (the last one short), each one
    ``Engine.head_train_steps`` call, and after every segment one ``Engine.head_validate`` call scores the next
    ``min(validation_steps * batch_size, len(val_rows))`` rows of a cyclic walk of ``default_rng([seed, 0x76616c]).permutation(val_rows)``
    on the unaugmented features, at rate ``dropout`` if ``validation_dropout`` else 0, with pass = the global step; the host reads
    its 16 bytes, the one synchronisation per check.  The checks change nothing in the training; with ``early_stop`` their accuracy
    or loss feeds ``EarlyStop``, and the training ends where it says stop.  A training or validation loss that is not finite raises
    ``BiscuitHipError``.

    With ``params.trainable == 'exit'`` block 14 trains with the head under the same schedule and one Adam: ``cache`` must be an
    ``ActivationCache`` (``cache_activations``), a segment is one ``Engine.exit_train_steps`` call on ``cache.acts`` (``act_views``
    as [V N, 10, 10, 1024] when there are views) in whichever form and place the cache keeps them (``act_mul`` with them), and a check goes through ``Engine.exit_validate`` on the unaugmented activations
    at rate 0, in calls of at most 256 rows whose sums are added in order on the device, read once.  Block 14 starts from the
    engine's imported tensors, or from a dict ``init`` that also carries them (``EXIT_TENSORS``' names, beside the head's); its
    moving statistics are the engine's and stay.  The result's ``exit`` holds the trained tensors (None for ``'head'``).

    With ``params.bn == 'batch'`` a training step normalises block 14 by its batch's own statistics (``exit_train_steps(...,
    bn='batch')``) and the moving statistics are state beside the parameters: they start from ``init``'s where it names them, else
    from the engine's, follow every step, and every check scores with the current ones.  A check, like every prediction, stays in
    inference mode.  The result's ``exit`` then also holds the four statistics tensors (``EXIT_STATS``' names)."""
    import torch
    from .engine import BiscuitHipError
    p = (params or TrainParams()).validate()
    seed = int(engine.hp.seed if seed is None else seed)
    rows, labels = _rows_and_labels(cache, rows, labels, 'train_head: at least one row and a 0/1 label for each',
                                    'train_head: a row outside the cache')
    if isinstance(init, dict):
        start = init
    elif init == 'model':
        start = engine.weights
    elif init == 'glorot':
        start = glorot_head(seed)
    else:
        raise ValueError("init is 'model', 'glorot' or a head tensor dict")
    dev, B = engine.device, int(p.batch_size)
    validating = val_rows is not None and len(val_rows) > 0
    if validating:
        refusal = 'fit_head: a 0/1 label for each validation row, every one inside the cache'
        val_rows, val_labels = _rows_and_labels(cache, val_rows, val_labels, refusal, refusal)
        n_val = min(int(p.validation_steps) * B, len(val_rows))
        if n_val > HEAD_VALIDATE_MAX_ROWS:
            raise ValueError(f'a check scores validation_steps x batch_size rows, at most {HEAD_VALIDATE_MAX_ROWS}')
        # the walk, and its first n_val entries once more behind it: every window of a cyclic walk is then one slice
        walk = np.random.default_rng([seed, VAL_STREAM]).permutation(len(val_rows))
        walk = np.concatenate([walk, walk[:n_val]])
        val_at, val_y = torch.from_numpy(val_rows[walk]).to(dev), torch.from_numpy(val_labels[walk].astype(np.uint8)).to(dev)
        stopper, val_rate = EarlyStop.of(p), float(p.dropout) if p.validation_dropout else 0.0
    if p.training_balance not in ('none', 'tile'):
        slide_idx = np.asarray(cache.slide_idx[rows] if slide_idx is None else slide_idx, np.int64).reshape(-1)
    exit_mode = p.trainable == 'exit'
    if exit_mode:
        # block 14 starts from `init` where it names its tensors, else from the imported model; its statistics are the engine's, frozen
        if not isinstance(cache, ActivationCache) or cache.acts is None:
            raise ValueError("trainable='exit' trains on an ActivationCache (cache_activations), not on a FeatureCache")
        exit_start = init if isinstance(init, dict) and EXIT_TENSORS[0][0] in init else engine.weights
        stats_start = exit_start if p.bn == 'batch' and all(name in exit_start for name, _ in EXIT_STATS) else engine.weights
        bn_stats = torch.from_numpy(exit_bn_stats(stats_start)).to(dev)      # bn='batch': state, updated in place by every step
        w = torch.from_numpy(np.concatenate([flatten_exit(exit_start), flatten_head(start)])).to(dev)
        feats = cache.act_views.reshape((-1,) + ACT_SHAPE) if cache.n_views() else cache.acts
    else:
        w = torch.from_numpy(flatten_head(start)).to(dev)
        feats = cache.views.reshape(-1, cache.views.shape[-1]) if cache.n_views() else cache.feats
    m, v, g = torch.zeros_like(w), torch.zeros_like(w), torch.empty_like(w)
    losses, checks, step, stopped, state = [], [], 0, None, {}
    for epoch in range(int(max(p.epochs))):
        at, y = _plan_epoch(p, cache, rows, labels, slide_idx, patients, seed, epoch, state)
        steps = -(-len(at) // B)
        at, y = torch.from_numpy(at).to(dev), torch.from_numpy(y).to(dev)
        seg = int(p.validate_on_batch) if validating else steps
        for a in range(0, steps, seg):
            b = min(a + seg, steps)
            lr = [p.learning_rate_at(step + i) for i in range(b - a)]
            if exit_mode:
                losses.append(engine.exit_train_steps(w, m, v, bn_stats, feats, at[a * B:b * B], y[a * B:b * B], B, step, seed, lr,
                                                      rate=p.dropout, b1=ADAM_BETA_1, b2=ADAM_BETA_2, eps=ADAM_EPSILON, grad=g,
                                                      act_mul=cache.act_mul, bn=p.bn))
            else:
                losses.append(engine.head_train_steps(w, m, v, feats, at[a * B:b * B], y[a * B:b * B], B, step, seed, lr, rate=p.dropout,
                                                      b1=ADAM_BETA_1, b2=ADAM_BETA_2, eps=ADAM_EPSILON, grad=g))
            step += b - a
            if not validating:
                continue
            c0 = len(checks) * n_val % len(val_rows)
            if exit_mode:            # calls of up to 256 rows, their sums added in order on the device
                stats = torch.zeros(2, dtype=torch.float64, device=dev)
                for q in range(c0, c0 + n_val, EXIT_MAX_ROWS):
                    e = min(q + EXIT_MAX_ROWS, c0 + n_val)
                    stats += engine.exit_validate(w, bn_stats, cache.acts, val_at[q:e], val_y[q:e], step, seed, act_mul=cache.act_mul)[0]
            else:
                stats, _, _ = engine.head_validate(w, cache.feats, val_at[c0:c0 + n_val], val_y[c0:c0 + n_val], step, seed, rate=val_rate)
            stats = stats.cpu().numpy()
            val_loss, val_acc = float(stats[0]) / n_val, float(stats[1]) / n_val
            if not np.isfinite(val_loss):
                raise BiscuitHipError(f'fit_head: the validation loss after step {step} is not finite (a feature that is not finite, '
                                      'or a diverged run)')
            stop = stopper.update(val_acc if p.early_stop_method == 'accuracy' else val_loss, epoch)
            checks.append((step, val_loss, val_acc, stopper.ema))
            if stop and p.early_stop:
                stopped = step
                break
        if stopped is not None:
            break
    losses = np.concatenate([t.cpu().numpy() for t in losses])
    if not np.isfinite(losses).all():
        raise BiscuitHipError(f'train_head: the loss of step {int(np.flatnonzero(~np.isfinite(losses))[0])} is not finite '
                              '(a feature that is not finite, or a diverged run)')
    if exit_mode:
        host = w.cpu().numpy()
        trained = unflatten_exit(host[:EXIT_PARAMS])
        if p.bn == 'batch':
            trained.update(unflatten_exit_stats(bn_stats.cpu().numpy()))
        return FitResult(unflatten_head(host[EXIT_PARAMS:]), losses, checks, stopped, step, int(max(p.epochs)), trained)
    return FitResult(unflatten_head(w.cpu().numpy()), losses, checks, stopped, step, int(max(p.epochs)))


def train_head(engine, cache, rows, labels, *, init='model', params=None, seed=None):
    """``fit_head`` without validation -> ``(head tensor dict, losses float32 [steps])``: under the default schedule each epoch
    walks a permutation from ``numpy.random.default_rng([seed, epoch])`` in batches of ``params.batch_size``, the last one short, as
    one ``Engine.head_train_steps`` call per epoch."""
    fit = fit_head(engine, cache, rows, labels, init=init, params=params, seed=seed)
    return fit.head, fit.losses


def head_engine(engine, head):
    """A fresh engine of ``engine``'s configuration whose head is ``head`` (through ``weights.pack_blob``, like any other)."""
    from .engine import Engine
    return Engine({**engine.weights, **{name: np.asarray(head[name], np.float32) for name, _ in HEAD_TENSORS}}, hp=engine.hp,
                  dtype=engine.dtype, max_batch=engine.max_batch, max_mc=engine.max_mc, device=engine.device.index, act_exp=engine.act_exp)


def predict(engine, cache, rows, head=None, mc_n=30, seed=None, *, y_true=None, outcome='cohort', save_dir=None,
            table_name=predictions.VAL_NAME):
    """The tile table of ``cache``'s rows ``rows`` under ``head`` (None: the engine's own): ``Engine.mc_head`` on the cached features
    with the rows as per-tile Philox indices, ``mc_n`` passes -> ``predictions.tile_frame``'s DataFrame (Slideflow's headers);
    written through ``predictions.write_tile_table`` into ``save_dir`` when given.  ``y_true``: 0/1 per slide of the cache (a
    sequence in ``cache.slides`` order or a dict by name; default 0)."""
    import torch
    seed = int(engine.hp.seed if seed is None else seed)
    rows = np.asarray(rows, np.int64).reshape(-1)
    if len(rows) and (rows.min() < 0 or rows.max() >= len(cache)):
        raise ValueError('predict: a row outside the cache')
    if int(mc_n) > engine.max_mc:
        raise ValueError(f'predict: mc_n {mc_n} above the engine\'s max_mc {engine.max_mc}')
    eng = engine if head is None else head_engine(engine, head)
    try:
        means, stds = [], []
        ridx = torch.from_numpy(rows).to(eng.device)
        for a in range(0, len(rows), eng.max_batch):
            r = ridx[a:a + eng.max_batch].contiguous()
            mu, sd = eng.mc_head(cache.feats.index_select(0, r).contiguous(), int(mc_n), seed, tile_idx0=0, tile_idx=r)
            means.append(mu.cpu().numpy()); stds.append(sd.cpu().numpy())
    finally:
        if eng is not engine:
            eng.close()
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros((0, 2), np.float32)
    if y_true is None:
        y_slide = np.zeros(len(cache.slides), np.int64)
    elif isinstance(y_true, dict):
        y_slide = np.array([int(y_true[s]) for s in cache.slides], np.int64)
    else:
        y_slide = np.asarray(y_true, np.int64)
    sidx = cache.slide_idx[rows]
    df = predictions.tile_frame(outcome, [cache.slides[i] for i in sidx], y_slide[sidx], cat(means), cat(stds), cache.loc[rows])
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        predictions.write_tile_table(df, save_dir, table_name, outcome)
    return df


class HeadTrainer:
    """The trainer ``train_cv`` calls per fold: ``(train_rows, val_rows, seed) -> (validation table, head, FitResult)`` --
    ``fit_head`` on the training rows (with the validation rows for its checks when ``params.early_stop`` is set), ``predict`` on
    the validation rows.  ``patients`` (slide -> patient; a slide missing from it is its own) serves ``training_balance='patient'``."""

    def __init__(self, engine, cache, slide_labels, *, params=None, init='model', mc_n=None, outcome='cohort', patients=None):
        self.engine, self.cache, self.params, self.init, self.outcome = engine, cache, params, init, outcome
        self.mc_n = int(mc_n or engine.hp.uq_n)
        self.y_slide = np.array([int(slide_labels[s]) for s in cache.slides], np.int64)
        names = sorted({(patients or {}).get(s, s) for s in cache.slides})
        self.patient_of_slide = np.array([names.index((patients or {}).get(s, s)) for s in cache.slides], np.int64)
        self.losses, self.fits = [], []

    def fit(self, train_rows, val_rows, seed, params=None):
        """``fit_head`` over ``train_rows``; ``val_rows`` (None: no checks) are the rows its validation checks walk."""
        sidx = self.cache.slide_idx
        val = {} if val_rows is None else {'val_rows': val_rows, 'val_labels': self.y_slide[sidx[val_rows]]}
        fit = fit_head(self.engine, self.cache, train_rows, self.y_slide[sidx[train_rows]], slide_idx=sidx[train_rows],
                       patients=self.patient_of_slide[sidx[train_rows]], init=self.init, params=self.params if params is None else params,
                       seed=seed, **val)
        self.losses.append(fit.losses)
        self.fits.append(fit)
        return fit

    def __call__(self, train_rows, val_rows, seed):
        fit = self.fit(train_rows, val_rows if (self.params or TrainParams()).early_stop else None, seed)
        cache = self.cache if fit.exit is None else exit_feature_cache(self.engine, self.cache, fit.exit, val_rows)
        table = predict(self.engine, cache, val_rows, fit.head, self.mc_n, seed, y_true=self.y_slide, outcome=self.outcome)
        return table, fit.head, fit


def exit_feature_cache(engine, cache, exit_tensors, rows):
    """A ``FeatureCache`` over ``cache``'s tiles whose features at ``rows`` are ``Engine.exit_features`` of the cached activations
    under ``exit_tensors`` (a trained block 14; its moving statistics its own where it carries them -- ``bn='batch'`` --, else the
    engine's): what ``predict`` reads after ``trainable='exit'``.
    The other rows keep the imported block 14's features."""
    import torch
    rows = torch.from_numpy(np.asarray(rows, np.int64).reshape(-1)).to(engine.device)
    feats = cache.feats.clone()
    if len(rows):
        e = torch.from_numpy(flatten_exit(exit_tensors)).to(engine.device)
        stats = torch.from_numpy(exit_bn_stats(exit_tensors if has_exit_stats(exit_tensors) else engine.weights)).to(engine.device)
        feats.index_copy_(0, rows, engine.exit_features_all(e, stats, cache.acts, rows, act_mul=cache.act_mul))
    return FeatureCache(feats, cache.slide_idx, cache.loc, cache.slides)


def exit_engine(engine, exit_tensors, head, tiles=None, headroom_min=1.0):
    """A fresh engine of ``engine``'s configuration whose block 14 is ``exit_tensors`` and whose head is ``head`` (through
    ``weights.pack_blob``, like ``head_engine``; the moving statistics ``exit_tensors`` carries, if any, fold in with them), with
    ``engine``'s activation exponents reused.  The exponents were calibrated on the
    imported block 14: with ``tiles`` (uint8 [n, 299, 299, 3] on the device) one ``f16_headroom`` check runs on them, and
    ``F16RangeError`` says so when the trained block 14 saturates f16 or leaves less than ``headroom_min`` x of its range."""
    from .engine import Engine, F16RangeError
    names = EXIT_TENSORS + (EXIT_STATS if has_exit_stats(exit_tensors) else ())
    w = {**engine.weights, **{name: np.asarray(exit_tensors[name], np.float32) for name, _ in names},
         **{name: np.asarray(head[name], np.float32) for name, _ in HEAD_TENSORS}}
    eng = Engine(w, hp=engine.hp, dtype=engine.dtype, max_batch=engine.max_batch, max_mc=engine.max_mc, device=engine.device.index,
                 act_exp=engine.act_exp)
    if tiles is not None and len(tiles):
        room = eng.f16_headroom(tiles)
        if any(room['saturated'].values()) or room['headroom'] < float(headroom_min):
            eng.close()
            worst = max(room['max_abs'], key=room['max_abs'].get)
            raise F16RangeError(f'exit_engine: the trained block 14 has left the calibrated f16 range ({worst}: max |activation| as stored '
                                f'{room["max_abs"][worst]:.6g}, headroom {room["headroom"]:.3g}); calibrate again on the trained weights '
                                '(Engine.calibrate), or use dtype bf16 / f32')
    return eng


# ------------------------------------------------------------------------------------------------------------ cross-validation
def kfold(patients, labels, k, seed):
    """Slideflow's ``k-fold`` strategy, restated from memory (unpinned): the patients of each class, sorted by name, are shuffled by
    one generator ``numpy.random.default_rng(seed)`` (classes in sorted order) and dealt round-robin into ``k`` folds, each class
    starting where the previous one stopped.  ``labels``: patient -> class.  -> ``k`` sorted lists of patients; ValueError unless
    every class has at least ``k`` patients, so that every class is in every fold."""
    patients = sorted(set(patients))
    k = int(k)
    if k < 2:
        raise ValueError('k-fold needs k >= 2')
    rng = np.random.default_rng(seed)
    folds, at = [[] for _ in range(k)], 0
    for c in sorted({labels[p] for p in patients}):
        names = [p for p in patients if labels[p] == c]
        if len(names) < k:
            raise ValueError(f'class {c!r} has {len(names)} patients, fewer than k = {k}')
        for i in rng.permutation(len(names)):
            folds[at % k].append(names[int(i)])
            at += 1
    return [sorted(f) for f in folds]


def _patient_labels(slide_labels, patients):
    """{patient: label}; ValueError for a patient whose slides disagree."""
    out = {}
    for s, y in slide_labels.items():
        p = patients.get(s, s)
        if out.setdefault(p, y) != y:
            raise ValueError(f'patient {p!r} has slides of both classes')
    return out


def fold_dir(out, label, k):
    return os.path.join(out, f'{label}-kfold{k}')


def write_results_log(path, model_name, fit, epochs):
    """``results_log.csv`` of one trained model, the file ``utils.find_cv_early_stop`` reads (``utils.py:164-187``): one row with
    ``model_name`` (ending in ``epoch{E}``), ``steps``, and ``val_loss`` / ``val_acc`` of the last validation check (empty without
    one); the column ``early_stop_batch`` is there only when the rule fired, since the reference tests for the column itself.  The
    AUROC / AP columns of Slideflow's log are not written (``metrics.py`` computes those from the tables)."""
    import pandas as pd
    last = fit.checks[-1] if fit.checks else (None, None, None, None)
    row = {'model_name': f'{model_name}-epoch{int(epochs)}', 'steps': int(fit.steps), 'val_loss': last[1], 'val_acc': last[2]}
    if fit.early_stop_batch is not None:
        row['early_stop_batch'] = int(fit.early_stop_batch)
    pd.DataFrame([row]).to_csv(path, index=False)


def find_cv_early_stop(out, label, k=3):
    """``utils.find_cv_early_stop`` (``utils.py:164-187``) over ``OUT/LABEL-kfold1 .. k``: ``round(mean(...))`` of the folds'
    ``early_stop_batch`` (Python's ``round``: a half goes to the even neighbour), None unless every fold's ``results_log.csv``
    has the column."""
    import pandas as pd
    found = []
    for j in range(1, int(k) + 1):
        path = os.path.join(fold_dir(out, label, j), RESULTS_FILE)
        if not os.path.exists(path):
            return None
        res = next(pd.read_csv(path).iterrows())[1]
        if 'early_stop_batch' in res:
            found.append(int(res['early_stop_batch']))
    return round(mean(found)) if found and len(found) == int(k) else None


def train_full(cache, slide_labels, out, label, *, stop_batch, trainer, seed=0):
    """Step 5 of ``Experiment.run`` (``experiment.py:887-905``): the model the paper evaluates, trained on every labelled slide of
    the cache with ``steps_per_epoch_override=stop_batch`` (what ``find_cv_early_stop`` detected) and no validation, under the
    ``HeadTrainer``'s other settings -> the directory ``OUT/LABEL_FULL`` with ``head.npz``, ``slides.json`` and ``results_log.csv``."""
    from dataclasses import replace
    if int(stop_batch) < 1:
        raise ValueError('train_full: stop_batch is at least 1')
    train_s = sorted(s for s in cache.slides if s in slide_labels)
    params = replace(trainer.params or TrainParams(), early_stop=False, steps_per_epoch_override=int(stop_batch))
    fit = trainer.fit(cache.rows_of(train_s), None, int(seed), params=params)
    d = os.path.join(out, f'{label}_FULL')
    os.makedirs(d, exist_ok=True)
    save_head(os.path.join(d, HEAD_FILE), fit.head)
    if fit.exit is not None:
        save_exit(os.path.join(d, EXIT_FILE), fit.exit)
    with open(os.path.join(d, MANIFEST_FILE), 'w') as f:
        json.dump({'training': train_s, 'validation': []}, f)
    write_results_log(os.path.join(d, RESULTS_FILE), f'{label}_FULL', fit, fit.epochs)
    return d


def train_cv(cache, slide_labels, out, label, k, trainer, *, patients=None, seed=0, restrict=None, outcome='cohort'):
    """``k``-fold cross-validation by patient over the cache's labelled slides (``restrict``: only these patients): fold ``j``
    trains on the other folds' slides and validates on its own -> ``OUT/LABEL-kfoldJ/tile_predictions_val_epoch1.csv`` with
    ``head.npz`` (when the trainer returns a head) and ``slides.json`` (the training and validation slides) beside it.
    ``trainer(train_rows, val_rows, seed)`` -> ``(tile table, head or None)`` or ``(tile table, head, FitResult)``: a
    ``HeadTrainer``, whose third value also writes ``results_log.csv`` (``write_results_log``) under the model name
    ``...-epoch{fit.epochs}``: a trainer that builds its own ``FitResult`` sets ``epochs`` there (1 if it does not; the trainer's
    ``params`` are not looked at).  -> the fold directories."""
    patients = patients or {}
    slide_labels = {s: slide_labels[s] for s in cache.slides if s in slide_labels}
    plabel = _patient_labels(slide_labels, patients)
    if restrict is not None:
        plabel = {p: y for p, y in plabel.items() if p in set(restrict)}
    folds = kfold(list(plabel), plabel, k, seed)
    by_patient = {}
    for s in slide_labels:
        by_patient.setdefault(patients.get(s, s), []).append(s)
    dirs = []
    for j, val_p in enumerate(folds, 1):
        val_s = sorted(s for p in val_p for s in by_patient[p])
        train_s = sorted(s for f in folds if f is not val_p for p in f for s in by_patient[p])
        fold_seed = int(np.random.SeedSequence([*(int(v) for v in np.atleast_1d(seed)), j]).generate_state(1, np.uint32)[0])
        table, head, *fit = trainer(cache.rows_of(train_s), cache.rows_of(val_s), fold_seed)
        d = fold_dir(out, label, j)
        os.makedirs(d, exist_ok=True)
        predictions.write_tile_table(table, d, predictions.VAL_NAME, outcome)
        if head is not None:
            save_head(os.path.join(d, HEAD_FILE), head)
        if fit and getattr(fit[0], 'exit', None) is not None:
            save_exit(os.path.join(d, EXIT_FILE), fit[0].exit)
        if fit:
            write_results_log(os.path.join(d, RESULTS_FILE), os.path.basename(d), fit[0], fit[0].epochs)
        with open(os.path.join(d, MANIFEST_FILE), 'w') as f:
            json.dump({'training': train_s, 'validation': val_s}, f)
        dirs.append(d)
    return dirs


def train_nested_cv(cache, slide_labels, out, label, trainer, *, outer_k=3, inner_k=5, patients=None, seed=0, outcome='cohort'):
    """``Experiment.train_nested_cv`` (``experiment.py:1053-1090``) and the outer folds it expects: ``LABEL-kfoldK`` for K = 1 ..
    ``outer_k``, and over the training patients of each an inner ``inner_k``-fold ``LABEL-kK-kfoldJ``.  -> every directory."""
    patients = patients or {}
    dirs = train_cv(cache, slide_labels, out, label, outer_k, trainer, patients=patients, seed=seed, outcome=outcome)
    for K, d in enumerate(list(dirs), 1):
        with open(os.path.join(d, MANIFEST_FILE)) as f:
            train_s = json.load(f)['training']
        dirs += train_cv(cache, slide_labels, out, f'{label}-k{K}', inner_k, trainer, patients=patients, seed=[int(seed), K],
                         restrict={patients.get(s, s) for s in train_s}, outcome=outcome)
    return dirs


def check_nested_split(slide_labels, patients, outer_k, inner_k, seed):
    """The splits ``train_nested_cv`` will make, made without training anything: ValueError where a patient has slides of both
    classes or a class has fewer patients than folds, in the outer split or in any inner one."""
    patients = patients or {}
    plabel = _patient_labels(slide_labels, patients)
    for K, val in enumerate(kfold(list(plabel), plabel, outer_k, seed), 1):
        inner = {p: y for p, y in plabel.items() if p not in set(val)}
        try:
            kfold(list(inner), inner, inner_k, [int(seed), K])
        except ValueError as e:
            raise ValueError(f'inner split of outer fold {K}: {e}') from None


def _cv_frames(out, label, k, outcome, patients):
    """``utils.df_from_cv``: the ``k`` validation tables of ``LABEL-kfold1 .. k``, renamed, with a patient column; None when one is
    missing."""
    dfs = []
    for j in range(1, k + 1):
        path = os.path.join(fold_dir(out, label, j), predictions.VAL_NAME)
        if not os.path.exists(path):
            return None
        df = predictions.load_tile_predictions(path, outcome)
        if 'patient' not in df.columns:
            df['patient'] = df['slide'].map(lambda s: patients.get(s, s))
        dfs.append(df)
    return dfs


def thresholds_from_nested_cv(out, label, *, outcome='cohort', patients=None, outer_k=3, inner_k=5, id=None, threshold_params=None,
                              slides=()):
    """``Experiment.thresholds_from_nested_cv`` (``experiment.py:924-1026``) over the tables ``train_nested_cv`` wrote: per outer
    fold, tile_uq from the inner folds (``threshold.from_cv``), then slide_uq and the prediction thresholds, applied to the outer
    fold's validation table at the patient and the slide level.  An outer fold whose tables are missing is skipped.  ``patients``:
    slide -> patient (a slide missing from it is its own patient; ``slides`` names further slides to cover).  -> ``(frame with the
    columns id, n_slides, fold, uq, patient_auc, patient_uq_perc, slide_auc, slide_uq_perc; {'tile_uq', 'slide_uq', 'slide_pred'}:
    the folds' means, None without a fold)``."""
    import pandas as pd
    from . import threshold
    patients = dict(patients or {})
    id = label if id is None else id
    rows, all_tile, all_slide, all_pred = [], [], [], []
    for K in range(1, outer_k + 1):
        val_path = os.path.join(fold_dir(out, label, K), predictions.VAL_NAME)
        dfs = _cv_frames(out, f'{label}-k{K}', inner_k, outcome, patients)
        if dfs is None or not os.path.exists(val_path):
            continue
        tile_df = predictions.load_tile_predictions(val_path, outcome)
        pmap = {s: patients.get(s, s) for df in dfs + [tile_df] for s in pd.unique(df['slide'])}
        pmap.update({s: patients.get(s, s) for s in slides})
        params = threshold_params if threshold_params is not None else {'tile_pred': 'detect', 'slide_pred': 'detect', 'plot': False,
                                                                        'patients': pmap}
        tile_uq = threshold.from_cv(dfs, tile_uq='detect', slide_uq=None, **params)['tile_uq']
        th = threshold.from_cv(dfs, tile_uq=tile_uq, slide_uq='detect', **params)
        all_tile.append(tile_uq); all_slide.append(th['slide_uq']); all_pred.append(th['slide_pred'])
        by_level = {}
        for level in ('patient', 'slide'):
            res, _ = threshold.apply(tile_df, plot=False, patients=pmap, level=level, **th)
            by_level[level] = (res['auc'], res['percent_incl'])
        manifest = os.path.join(fold_dir(out, label, K), MANIFEST_FILE)
        n_slides = None
        if os.path.exists(manifest):
            with open(manifest) as f:
                man = json.load(f)
            n_slides = len(man['training']) + len(man['validation'])
        rows.append({'id': id, 'n_slides': n_slides, 'fold': K, 'uq': 'include', 'patient_auc': by_level['patient'][0],
                     'patient_uq_perc': by_level['patient'][1], 'slide_auc': by_level['slide'][0], 'slide_uq_perc': by_level['slide'][1]})
    frame = pd.DataFrame(rows, columns=['id', 'n_slides', 'fold', 'uq', 'patient_auc', 'patient_uq_perc', 'slide_auc', 'slide_uq_perc'])
    return frame, {'tile_uq': mean(all_tile) if all_tile else None, 'slide_uq': mean(all_slide) if all_slide else None,
                   'slide_pred': mean(all_pred) if all_pred else None}


# ------------------------------------------------------------------------------------------------------------ command line
def read_labels(path):
    """``--labels CSV``: columns slide, label and optionally patient; the two label values, sorted, become 0 and 1.
    -> ``(slide -> 0/1, slide -> patient, [the two values])``."""
    import pandas as pd
    try:
        df = pd.read_csv(path, dtype=str)
    except (OSError, ValueError) as e:
        raise SystemExit(f'--labels {path}: {e}') from None
    if 'slide' not in df.columns or 'label' not in df.columns:
        raise SystemExit(f'--labels {path}: needs the columns slide and label')
    values = sorted(set(df['label']))
    if len(values) != 2:
        raise SystemExit(f'--labels {path}: exactly two label values, not {values}')
    labels = {s: values.index(v) for s, v in zip(df['slide'], df['label'])}
    patients = dict(zip(df['slide'], df['patient'])) if 'patient' in df.columns else {}
    return labels, patients, values


def arg_parser():
    ap = argparse.ArgumentParser(prog='python -m biscuit_amd.train', description=__doc__.split('\n\n')[0])
    ap.add_argument('tfrecords', nargs='+', help='Slideflow *.tfrecords, one per slide')
    ap.add_argument('--labels', required=True, help='CSV with slide,label[,patient]')
    ap.add_argument('--model', required=True, help='Slideflow model directory: the backbone (and, with --init model, the head to start from)')
    ap.add_argument('--out', required=True)
    ap.add_argument('--label', default='EXP', help='experiment label: the prefix of the fold directories')
    ap.add_argument('--outcome', default='cohort')
    ap.add_argument('--init', default='model', choices=['model', 'glorot'])
    ap.add_argument('--epochs', type=int, default=1)
    ap.add_argument('--outer-k', type=int, default=3)
    ap.add_argument('--inner-k', type=int, default=5)
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--mc', type=int, default=None, help='MC-dropout passes of the validation tables (default: uq_n of the model, 30)')
    ap.add_argument('--dtype', default='f16', choices=['f16', 'bf16', 'f32'])
    ap.add_argument('--augment', default='', metavar='SPEC', help="training augmentation, letters out of 'xyrjb' (the paper's models: xyrjb); "
                    'default: none')
    ap.add_argument('--views', type=int, default=None, metavar='V', help='augmented views cached per tile; epoch e trains on view e %% V '
                    '(default: --epochs)')
    ap.add_argument('--cache', default=None, metavar='FILE', help='the feature cache (.npz): loaded when it exists, otherwise computed and saved')
    ap.add_argument('--early-stop', nargs='?', const='accuracy', default=None, choices=['accuracy', 'loss'], metavar='METHOD',
                    help="stop a training when the smoothed validation accuracy (or 'loss') no longer improves (the paper's models: accuracy)")
    ap.add_argument('--balance', default='none', choices=list(BALANCES), metavar='KIND',
                    help="training batches balanced by 'category' (the paper's models), 'patient' or 'slide'; default: none")
    ap.add_argument('--validate-on-batch', type=int, default=32, metavar='N', help='with --early-stop: a validation check every N steps')
    ap.add_argument('--validation-steps', type=int, default=32, metavar='N', help='with --early-stop: batches of validation tiles per check')
    ap.add_argument('--trainable', default='head', choices=list(TRAINABLE), help="'head' (default): the three dense layers on cached "
                    "features; 'exit': Xception's block 14 with them, on cached block13_out (409 600 bytes per tile and view on the device), "
                    'batch-norm statistics frozen; each fold then also writes exit.npz')
    ap.add_argument('--bn', default='frozen', choices=list(BN_MODES), help="with --trainable exit, block 14's batch norm: 'frozen' (default) "
                    "keeps the imported moving statistics; 'batch' is Keras' training mode, as the reference trains -- a batch normalised "
                    'by its own statistics, gradients through them, moving statistics updated and written into exit.npz')
    ap.add_argument('--full', action='store_true', help='after the cross-validation, train the model on every slide for the number of '
                    'steps at which the outer folds stopped early (needs --early-stop) -> OUT/LABEL_FULL')
    ap.add_argument('--act-cache', default='f32', choices=list(ACT_STORES), metavar='STORE', help="with --trainable exit, where and how "
                    "block13_out is cached: 'f32' (default) float32 on the device; 'packed' the engine's own 16-bit tensor on the device, "
                    "half the bytes and bit for bit the same results (--dtype f16 / bf16); 'host' that form in pinned host memory, each "
                    "step's rows gathered onto the device; 'auto' the first of the three that fits")
    return ap


def main(argv=None):
    args = arg_parser().parse_args(argv)
    try:
        if args.act_cache != 'auto':
            act_row_bytes(args.act_cache, args.dtype)
    except ValueError as e:
        raise SystemExit(f'--act-cache: {e}') from None
    if args.epochs < 1 or args.outer_k < 2 or args.inner_k < 2:
        raise SystemExit('--epochs >= 1, --outer-k >= 2 and --inner-k >= 2')
    if args.validate_on_batch < 1 or args.validation_steps < 1:
        raise SystemExit('--validate-on-batch >= 1 and --validation-steps >= 1')
    if args.bn == 'batch' and args.trainable != 'exit':
        raise SystemExit('--bn batch trains block 14: it needs --trainable exit')
    if args.full and not args.early_stop:
        raise SystemExit('--full trains for the steps at which the folds stopped early: it needs --early-stop')
    from . import augment as A
    try:
        letters = A.parse(args.augment)
    except ValueError as e:
        raise SystemExit(f'--augment: {e}') from None
    n_views = view_count(letters, args.views, args.epochs)
    if letters and n_views < 1:
        raise SystemExit('--views >= 1')
    if args.cache and not args.cache.endswith('.npz'):
        args.cache += '.npz'                 # (the name numpy.savez writes to)
    if not os.path.isdir(args.model):
        raise SystemExit(f'--model {args.model}: not a directory')
    missing = [p for p in args.tfrecords if not os.path.exists(p)]
    if missing:
        raise SystemExit(f'no such file: {missing[0]}')
    labels, patients, values = read_labels(args.labels)
    names = [os.path.splitext(os.path.basename(p))[0] for p in args.tfrecords]
    unlabelled = [n for n in names if n not in labels]
    if unlabelled:
        raise SystemExit(f'--labels {args.labels}: no label for slide {unlabelled[0]!r}')
    try:
        check_nested_split({n: labels[n] for n in names}, patients, args.outer_k, args.inner_k, args.seed)
    except ValueError as e:
        raise SystemExit(str(e)) from None
    from .__main__ import load_model_weights, model_hp_from
    from .engine import Engine
    from .featuremap import _first_records
    from .inference import slides_from_tfrecords
    w, model_params = load_model_weights(args.model, None)
    hp, norm_fit = model_hp_from(model_params, None)
    slides = slides_from_tfrecords(list(args.tfrecords), labels, patients or None, gpu_unfilter=False)
    act_exp = None
    if args.dtype == 'f16' and any(s.n_tiles for s in slides):
        first = next(s for s in slides if s.n_tiles)
        probe, _ = _first_records(first, min(16, first.n_tiles), hp.tile_px)
        act_exp, _ = Engine.calibrate(w, probe, hp=hp, norm_fit=norm_fit, normalizer=hp.normalizer)
    mc_n = int(args.mc or hp.uq_n)
    eng = Engine(w, hp=hp, dtype=args.dtype, max_batch=256, max_mc=mc_n, act_exp=act_exp)
    try:
        cache = cached_features(eng, slides, args.cache, normalizer=hp.normalizer, norm_fit=norm_fit, augment=letters, views=n_views or None,
                                seed=args.seed, activations=args.trainable == 'exit', store=args.act_cache)
        try:
            params = TrainParams(epochs=[args.epochs], dropout=hp.dropout, augment=letters, early_stop=bool(args.early_stop),
                                 trainable=args.trainable, bn=args.bn,
                                 early_stop_method=args.early_stop or 'accuracy', training_balance=args.balance,
                                 validate_on_batch=args.validate_on_batch, validation_steps=args.validation_steps).validate()
            trainer = HeadTrainer(eng, cache, labels, params=params, init=args.init, mc_n=mc_n, outcome=args.outcome, patients=patients)
            dirs = train_nested_cv(cache, labels, args.out, args.label, trainer, outer_k=args.outer_k, inner_k=args.inner_k,
                                   patients=patients, seed=args.seed, outcome=args.outcome)
        except ValueError as e:
            raise SystemExit(str(e)) from None
        full = None
        if args.full:
            stop_batch = find_cv_early_stop(args.out, args.label, k=args.outer_k)
            if stop_batch is None:
                print(f'--full: not every one of the {args.outer_k} outer folds stopped early, so no stop batch is detected and no '
                      'full model is trained')
            else:
                full = {'stop_batch': stop_batch, 'dir': train_full(cache, labels, args.out, args.label, stop_batch=stop_batch,
                                                                    trainer=trainer, seed=args.seed)}
    finally:
        eng.close()
    from .errors import ThresholdError
    try:
        frame, th = thresholds_from_nested_cv(args.out, args.label, outcome=args.outcome, patients=patients, outer_k=args.outer_k,
                                              inner_k=args.inner_k)
    except ThresholdError as e:
        raise SystemExit(f'the validation tables are written under {args.out}, but no thresholds: {e} (threshold.from_cv found none in '
                         'any inner fold of an outer fold: too few slides, or none predicted wrongly)') from None
    frame.to_csv(os.path.join(args.out, 'nested_cv.csv'), index=False)
    th = {k: (None if v is None else float(v)) for k, v in th.items()}
    schedule = {}                            # (only what the new flags asked for: without them the files are what they were)
    if args.early_stop:
        schedule.update(early_stop=args.early_stop, validate_on_batch=args.validate_on_batch, validation_steps=args.validation_steps)
    if args.balance != 'none':
        schedule['balance'] = args.balance
    if args.full:
        schedule['full'] = full
    if args.bn != 'frozen':
        schedule['bn'] = args.bn
    with open(os.path.join(args.out, 'thresholds.json'), 'w') as f:
        json.dump({'thresholds': th, 'label_values': values, 'outer_k': args.outer_k, 'inner_k': args.inner_k, 'seed': args.seed,
                   'augment': letters, 'views': n_views, **schedule}, f, indent=1)
    print(json.dumps({'tiles': len(cache), 'slides': len(cache.slides), 'folds': len(dirs), 'thresholds': th,
                      **({'full': full} if args.full else {})}))


if __name__ == '__main__':
    main()
