"""Host-side mirror of the reference's Keras object surface for the hot path.

`get_model(...)` has the signature of `conv-hybrid-model.ipynb c7:1-11` (plus the notebook
globals INPUT_SHAPE / len(char_to_num) as explicit kwargs) and returns a `Model` exposing what
the reference notebooks touch: `model(x, training=...)`, `compile`, `fit` with Keras-style
callbacks, `optimizer.learning_rate / .weight_decay`, `save_weights`, `summary`.

All arithmetic runs in libishara_hip.so (hand-written HIP for gfx950) through the C ABI in
include/ishara_hip.h; torch-ROCm tensors are only containers for device memory and the source
of the current stream.  There is no CPU path: constructing a Model with a device requires the
built library and a GPU.
"""
from __future__ import annotations

import contextlib
import copy
import ctypes as C
import math
from typing import Tuple,  Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._handle import Handle
from ._lib import stream as _stream

PAD_TOKEN_IDX = 59  # c1:5


class _Scalar:
    """Mimics the `tf.Variable` hypers the reference callbacks read (`.numpy()`, c11:64-65)."""

    def __init__(self, v): self.v = float(v)
    def numpy(self): return np.float32(self.v)
    def assign(self, v): self.v = float(v.v if isinstance(v, _Scalar) else v)
    def __float__(self): return self.v
    def __mul__(self, o): return _Scalar(self.v * float(o))
    __rmul__ = __mul__
    def __repr__(self): return f"{self.v:g}"


class Optimizer:
    """Lookahead(RectifiedAdam(sma_threshold=4), sync_period=5) — c7:68-69.  The update itself is
    one fused HIP kernel over the flat parameter buffer (csrc/optimizer.hip).

    `global_clipnorm` (Keras' argument; torch's clip_grad_norm_(params, max_norm)): the gradient of a step is scaled so that its global L2 norm
    is at most this value.  `skip_nonfinite` (what torch's GradScaler does for an overflowed step): a step whose gradient holds a NaN or Inf
    leaves parameters and optimizer slots untouched.  `accumulate_steps` = k: `train_on_batch` sums the gradients of k microbatches and
    applies their mean as one step.  All three act on the device (csrc/grad_ops.hip) without a host synchronise; at their defaults the
    training step is the code path it was without them.

    `use_ema`, `ema_momentum`, `ema_overwrite_frequency` (Keras' arguments) and `ema_warmup`: an exponential moving average of the trainable
    weights, updated on the device behind every applied step (csrc/weight_avg.hip): avg += (1 - momentum) * (theta - avg); with
    `ema_warmup` the momentum of update n + 1 is min(momentum, (1 + n) / (10 + n)) (tf.train.ExponentialMovingAverage's num_updates);
    every `ema_overwrite_frequency` updates the weights are overwritten with the average.  A skipped step leaves the average alone.  The
    average is read through Model.ema_weights / averaged_weights / evaluate(averaged=True) / save_weights(averaged=True) / finalize_ema.

    `awp_delta`, `awp_eps`, `awp_start_step`, `awp_relative`: adversarial weight perturbation in `train_on_batch` (csrc/awp.hip).  With
    `awp_delta` set, a step whose number `iterations` has reached `awp_start_step` takes the gradient, moves every weight tensor W by
    awp_delta * g_W / (||g_W|| + awp_eps) (with `awp_relative` by awp_delta * ||W|| * g_W / (||g_W|| + awp_eps)), runs forward and backward
    again at the moved weights with the same dropout masks, puts the weights back bit for bit and steps on the second gradient.  The
    recipes' "AWP from epoch E" is awp_start_step = E * steps_per_epoch.  Both training-mode forwards update the BatchNorm moving
    statistics, as a Keras model called twice does.  The step is read through Model.awp_stats / awp_scales; None (the default) is the
    step without any of it.

    `param_groups`: a list of {"match": pattern or [patterns], "lr_scale": 1.0, "weight_decay_scale": 1.0, "trainable": True}.  The
    patterns are fnmatch.fnmatchcase patterns over the names of the trainable entries (Keras-style: ".../kernel", "/bias", "/gamma",
    "/beta"); the first matching group wins, an unmatched entry keeps the defaults, a pattern that matches no trainable entry raises.  A
    tensor steps with learning_rate * lr_scale and weight_decay * weight_decay_scale (one fp32 product each); with trainable False it
    is frozen: the step writes nothing to it or its slots, and its gradient counts neither in the global norm, nor in the non-finite
    guard, nor in AWP's norms (csrc/optimizer.hip; train_state.no_decay_groups builds the usual no-decay group).  Model.param_groups()
    shows the resolution.  None (the default) is the step without any of it.  Limits: the backward pass still computes a frozen tensor's
    gradient (skipping those GEMMs is a later change); the BatchNorm moving statistics of a frozen block keep updating in training mode,
    unlike Keras' trainable = False; equality with a TensorFlow run is unpinned, and no accuracy effect is measured (there is neither a
    dataset nor trained weights).

    `mwer_nbest`, `mwer_beam_width`, `mwer_weight`, `mwer_ctc_weight`, `mwer_temperature`, `mwer_normalise`, `mwer_start_step`:
    minimum-risk (MWER) training over the beam's n-best list (ishara_amd/mwer.py).  With `mwer_nbest` > 0, a step whose number
    `iterations` has reached `mwer_start_step` runs, inside Model.loss_and_gradients, the prefix beam search (width `mwer_beam_width`, no
    LM) on the step's logits, the exact CTC score of every hypothesis, the posterior of the list at `mwer_temperature` and the expected
    edit distance to the label (divided by the label's length with `mwer_normalise`), and takes the gradient of
    mwer_ctc_weight * CTC + mwer_weight * mean_b risk_b; the loss returned stays the CTC loss of the label.  A hypothesis longer than
    max_label_len leaves the list.  AWP's two passes, accumulation, clipping, skipped steps, EMA and parameter groups compose unchanged.
    Model.mwer_stats() reads the last step's mean risk.  0 (the default) is the step without any of it.  No accuracy effect is measured.

    `kd_weight`, `kd_temperature`, `kd_ctc_weight`, `kd_normalise`, `kd_start_step`: knowledge distillation from a teacher
    (ishara_amd/kd.py; Model.set_teacher attaches one, train_on_batch(teacher_logits=) takes precomputed rows).  With `kd_weight` > 0, a
    step whose number `iterations` has reached `kd_start_step` runs the teacher in inference mode on the step's input and takes, inside
    Model.loss_and_gradients, the gradient of kd_ctc_weight * CTC + kd_weight * tau^2 * mean_b KL_b, KL_b the KL divergence of the
    student's from the teacher's class posteriors at temperature tau = `kd_temperature`, summed over the clip's T frames (with
    `kd_normalise` their mean); the loss returned stays the CTC loss of the label.  With `mwer_nbest` > 0 as well, both terms ride in one
    backward call and the CTC term carries kd_ctc_weight * mwer_ctc_weight.  AWP's two passes (the teacher runs once), accumulation,
    clipping, skipped steps, EMA and parameter groups compose unchanged.  Model.kd_stats() reads the last step's mean KL.  0 (the default)
    is the step without any of it.  No accuracy effect is measured."""

    def __init__(self, learning_rate=1e-3, weight_decay=0.0, global_clipnorm=None, skip_nonfinite=False, accumulate_steps=1,
                 use_ema=False, ema_momentum=0.99, ema_overwrite_frequency=None, ema_warmup=False,
                 awp_delta=None, awp_eps=1e-4, awp_start_step=0, awp_relative=False, param_groups=None,
                 mwer_nbest=0, mwer_beam_width=8, mwer_weight=1.0, mwer_ctc_weight=0.01, mwer_temperature=1.0, mwer_normalise=True,
                 mwer_start_step=0, kd_weight=0.0, kd_temperature=2.0, kd_ctc_weight=1.0, kd_normalise=True, kd_start_step=0):
        self._lr = _Scalar(learning_rate)
        # The reference assigns `.weight_decay` on the Lookahead wrapper (c11:64), which is not
        # one of its hyper-parameters, so RectifiedAdam keeps weight_decay=0.
        # `apply_weight_decay=True` turns the assigned value into a real decoupled decay.
        self._wd = _Scalar(weight_decay)
        self.apply_weight_decay = False
        self.iterations = 0
        self.global_clipnorm = global_clipnorm
        self.skip_nonfinite = skip_nonfinite
        self.accumulate_steps = accumulate_steps
        self.use_ema = use_ema
        self.ema_momentum = ema_momentum
        self.ema_overwrite_frequency = ema_overwrite_frequency
        self.ema_warmup = ema_warmup
        self.awp_delta = awp_delta
        self.awp_eps = awp_eps
        self.awp_start_step = awp_start_step
        self.awp_relative = awp_relative
        self.param_groups = param_groups
        self.mwer_nbest = mwer_nbest
        self.mwer_beam_width = mwer_beam_width
        self.mwer_weight = mwer_weight
        self.mwer_ctc_weight = mwer_ctc_weight
        self.mwer_temperature = mwer_temperature
        self.mwer_normalise = mwer_normalise
        self.mwer_start_step = mwer_start_step
        self.kd_weight = kd_weight
        self.kd_temperature = kd_temperature
        self.kd_ctc_weight = kd_ctc_weight
        self.kd_normalise = kd_normalise
        self.kd_start_step = kd_start_step

    def kd_options(self) -> dict:
        """the five kd_* options as a checked dict (ishara_amd/kd.py check_options)"""
        from . import kd
        return kd.check_options(**{k: getattr(self, k) for k in kd.OPTION_NAMES})

    def mwer_options(self) -> dict:
        """the seven mwer_* options as a checked dict (ishara_amd/mwer.py check_options)"""
        from . import mwer
        return mwer.check_options(**{k: getattr(self, k) for k in mwer.OPTION_NAMES})

    def group_options(self):
        """None, or the checked parameter groups: [{"match": [patterns], "lr_scale", "weight_decay_scale", "trainable"}]"""
        from . import train_state as TS
        return TS.check_param_groups(self.param_groups)

    def awp_options(self):
        """(delta or None, eps, start step, relative), checked"""
        d, e, start = self.awp_delta, self.awp_eps, self.awp_start_step

        def positive_f32(v):       # what the kernel is handed: 1e39 is inf and 1e-50 is 0 as float32
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                return False
            with np.errstate(over="ignore", under="ignore"):
                f = float(np.float32(v))
            return math.isfinite(f) and f > 0
        if d is not None and not positive_f32(d):
            raise ValueError(f"awp_delta must be None or a finite number > 0 (as float32), got {d!r}")
        if not positive_f32(e):
            raise ValueError(f"awp_eps must be a finite number > 0 (as float32), got {e!r}")
        if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or start < 0:
            raise ValueError(f"awp_start_step must be an integer >= 0, got {start!r}")
        return None if d is None else float(d), float(e), int(start), bool(self.awp_relative)

    def ema_options(self):
        """(use_ema, momentum, overwrite frequency or 0, warmup), checked"""
        m, every = self.ema_momentum, self.ema_overwrite_frequency
        if isinstance(m, bool) or not isinstance(m, (int, float, np.integer, np.floating)) or not 0.0 <= float(np.float32(m)) < 1.0:
            raise ValueError(f"ema_momentum must be a number in [0, 1) (as float32), got {m!r}")
        if every is not None and (isinstance(every, bool) or not isinstance(every, (int, np.integer)) or not 1 <= every <= 2 ** 31 - 1):
            raise ValueError(f"ema_overwrite_frequency must be None or an integer >= 1, got {every!r}")
        return bool(self.use_ema), float(m), 0 if every is None else int(every), bool(self.ema_warmup)

    def train_options(self):
        """(accumulate_steps, clip norm or 0.0, skip_nonfinite), checked"""
        k, clip = self.accumulate_steps, self.global_clipnorm
        if not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"accumulate_steps must be an integer >= 1, got {k!r}")
        if clip is not None and not (float(clip) > 0 and math.isfinite(float(clip))):
            raise ValueError(f"global_clipnorm must be a finite value > 0 or None, got {clip!r}")
        return int(k), 0.0 if clip is None else float(clip), bool(self.skip_nonfinite)

    @property
    def learning_rate(self): return self._lr
    @learning_rate.setter
    def learning_rate(self, v): self._lr.assign(v)
    lr = learning_rate
    @property
    def weight_decay(self): return self._wd
    @weight_decay.setter
    def weight_decay(self, v): self._wd.assign(v)


class History:
    def __init__(self):
        self.history: Dict[str, List[float]] = {}
        self.epoch: List[int] = []


class Callback:
    """Keras-style callback base (on_epoch_begin/end receive (epoch, logs))."""
    model = None
    def set_model(self, model): self.model = model
    def on_train_begin(self, logs=None): pass
    def on_train_end(self, logs=None): pass
    def on_epoch_begin(self, epoch, logs=None): pass
    def on_epoch_end(self, epoch, logs=None): pass
    def on_train_batch_end(self, batch, logs=None): pass


class LearningRateScheduler(Callback):
    """tf.keras.callbacks.LearningRateScheduler(fn(epoch) -> lr) — c11:55."""

    def __init__(self, schedule, verbose=0):
        self.schedule, self.verbose = schedule, verbose

    def on_epoch_begin(self, epoch, logs=None):
        lr = float(self.schedule(epoch))
        self.model.optimizer.learning_rate = lr
        if self.verbose:
            print(f"Epoch {epoch + 1}: LearningRateScheduler setting learning rate to {lr}.")


def lrfn(current_step, num_warmup_steps, lr_max, num_cycles=0.50, num_training_steps=50, warmup_method="exp"):
    """c11:1-11."""
    if current_step < num_warmup_steps:
        if warmup_method == "log":
            return lr_max * 0.10 ** (num_warmup_steps - current_step)
        return lr_max * 2 ** -(num_warmup_steps - current_step)
    progress = float(current_step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress))) * lr_max


def _keras_init(name: str, shape, g: np.random.Generator) -> np.ndarray:
    """Keras default initialisers for the layers of c5/c7 (glorot_uniform kernels, zeros biases,
    (1,0) norms, BatchNorm moving (0,1))."""
    leaf = name.rsplit("/", 1)[-1]
    if leaf in ("bias", "beta", "moving_mean"):
        return np.zeros(shape, np.float32)
    if leaf in ("gamma", "moving_variance"):
        return np.ones(shape, np.float32)
    if leaf == "depthwise_kernel" or name.endswith("depthwise_conv/kernel"):
        k, c = shape
        lim = math.sqrt(6.0 / (k * c + k))
    elif name.endswith("_eca/kernel"):
        lim = math.sqrt(6.0 / 10.0)
    else:
        lim = math.sqrt(6.0 / (shape[0] + shape[1]))
    return g.uniform(-lim, lim, size=shape).astype(np.float32)


class Model(Handle):
    def __init__(self, cfg: _lib.Config, device: Optional[str] = "cuda:0", seed: int = 0):
        self._create_handle(cfg)
        self.T, self.F, self.C = cfg.frames, cfg.features, cfg.num_classes
        self.optimizer = Optimizer()
        self.loss = "ctc"
        self.stop_training = False
        self._step_seed = seed * 7919 + 17
        self._steps = 0
        self._micro = 0            # microbatches already summed into the accumulator of the running cycle
        self._grad_acc = None      # [n_train] f32, allocated by the first accumulating cycle
        self._gstats = None        # the 16-byte ishara_grad_stats record (4 x int32 storage) and the workspace of its kernel
        self._gstats_ws = None
        self._skipped_seen = 0
        self._ema_avg = None       # [n_train] f32 moving average of params[:n_train], allocated by the first step with optimizer.use_ema
        self._ema_rec = None       # the 16-byte ishara_ema_state record (2 x int64 storage)
        self._ema_swapped = False  # inside averaged_weights(): params[:n_train] and _ema_avg have changed places
        self._awp_backup = None    # [n_train] f32 copy of params[:n_train] while they are perturbed, allocated by the first step AWP is active in
        self._mwer = None          # the buffers of minimum-risk training, allocated by the first step it is active in
        self._kd = None            # the buffers of distillation (kl_frame, kl_clip), allocated by the first step it is active in
        self._teacher = None       # what set_teacher attached: ("models", [Model], weights, mode) or ("callable", fn); never saved
        self._kd_rows = None       # the teacher's rows of the (micro)batch in flight: AWP's second pass reuses them
        self._awp = None           # with it: the segment table, the scale array, the record, the workspace and the two loss tensors
        self._pg = None            # parameter groups: the segment table, the device rows, the workspace, allocated by the first step with optimizer.param_groups
        self._pg_key = None        # the canonical text of the groups the rows were resolved from (None: the option is off)
        self._pg_seen = None       # a deep copy of optimizer.param_groups as it was then: an equal value needs no second look
        if device is not None:
            self._to_device(device, seed)

    # ------------------------------------------------------------------ device state
    def _to_device(self, device, seed):
        self._bind_device(device)
        self._loss_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._nll_buf = torch.zeros(self.max_batch, dtype=torch.float32, device=self.device)
        g = np.random.default_rng(seed)
        self.set_weights({name: _keras_init(name, shape, g) for name, shape, _, _ in self.entries})

    # ------------------------------------------------------------------ weights
    def get_weights(self) -> Dict[str, np.ndarray]:
        flat = self.params.detach().cpu().numpy()
        return {n: flat[o:o + int(np.prod(s))].reshape(s).copy() for n, s, o, _ in self.entries}

    def get_gradients(self) -> Dict[str, np.ndarray]:
        flat = self.grads.detach().cpu().numpy()
        return {n: flat[o:o + int(np.prod(s))].reshape(s).copy() for n, s, o, t in self.entries if t}

    def set_weights(self, weights: Dict[str, np.ndarray], reset_optimizer: bool = True):
        flat = self.params.detach().cpu().numpy().copy()
        for n, s, o, _ in self.entries:
            if n in weights:
                w = np.asarray(weights[n], dtype=np.float32)
                if tuple(w.shape) != tuple(s):
                    raise ValueError(f"{n}: expected shape {s}, got {w.shape}")
                flat[o:o + w.size] = w.reshape(-1)
        self.params.copy_(torch.from_numpy(flat))
        if reset_optimizer:
            self.opt_m.zero_(); self.opt_v.zero_()
            self.opt_slow.copy_(self.params[:self.n_train])     # Lookahead slow weights start at theta_0
            self.optimizer.iterations = 0
            self._lib.ishara_optimizer_set_iterations(self._h, 0)
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")

    def save_weights(self, path: str, averaged: bool = False):
        """model.save_weights (c9:10).  `*.h5` / `*.hdf5`: the Keras-2 save_weights HDF5 layout, written through the image's HDF5
        library (keras_h5.py); anything else: .npz keyed by the library's Keras-style names.  averaged: the file holds ema_weights()
        (the moving average of the trainable weights, the live BatchNorm statistics) in place of get_weights()."""
        weights = self.ema_weights() if averaged else self.get_weights()
        if path.endswith((".h5", ".hdf5")):
            from . import keras_h5
            keras_h5.save_weights_h5(path, weights, [(n, tuple(s)) for n, s, _, _ in self.entries])
            return
        np.savez(path if path.endswith(".npz") else path + ".npz", **weights)

    def load_weights(self, path: str):
        """model.load_weights: a Keras-2 `.h5` weights file (matched by layer / weight order and shape, like by_name=False) or the .npz."""
        if path.endswith((".h5", ".hdf5")):
            from . import keras_h5
            self.set_weights(keras_h5.load_weights_h5(path, [(n, tuple(s)) for n, s, _, _ in self.entries]))
            return
        with np.load(path if path.endswith(".npz") else path + ".npz") as z:
            self.set_weights({k: z[k] for k in z.files})

    def save_keras_weights(self, path: str):
        """Ordered list of `keras_model.get_weights()` as arr_0.. (keras_interchange.py)."""
        from . import keras_interchange as K
        K.save_keras_npz(path, self.get_weights(), [(n, tuple(s)) for n, s, _, _ in self.entries])

    def load_keras_weights(self, path: str):
        from . import keras_interchange as K
        self.set_weights(K.load_keras_npz(path, [(n, tuple(s)) for n, s, _, _ in self.entries]))

    def count_params(self): return self.n_total

    def summary(self, print_fn=print):
        """model.summary() (c7:83), grouped per layer prefix."""
        groups: Dict[str, int] = {}
        for n, s, _, _ in self.entries:
            top = n.split("/")[0]
            groups[top] = groups.get(top, 0) + int(np.prod(s))
        print_fn('Model: "ishara_hip"')
        print_fn("=" * 65)
        for k, v in groups.items():
            print_fn(f" {k:<44s}{v:>12,d}")
        print_fn("=" * 65)
        print_fn(f"Total params: {self.n_total:,}")
        print_fn(f"Trainable params: {self.n_train:,}")
        print_fn(f"Non-trainable params: {self.n_total - self.n_train:,}")

    # ------------------------------------------------------------------ forward
    def _as_input(self, x) -> torch.Tensor:
        x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
        if x.dim() == 2:
            x = x[None]
        if x.shape[1:] != (self.T, self.F):
            raise ValueError(f"expected input [B,{self.T},{self.F}], got {tuple(x.shape)}")
        return x.to(self.device, torch.float32).contiguous()

    def _as_frame_lengths(self, frame_lengths, B: int) -> Optional[torch.Tensor]:
        """`frame_lengths` (tensor, array or list; None passes through) as a contiguous int32 [B] tensor on the model's device.  Shape and
        dtype are checked; the values never are (reading a device tensor would synchronise): the kernels clamp them to [0, T]."""
        if frame_lengths is None:
            return None
        if self._cfg.dtype == _lib.F16:
            raise _lib.IsharaError("frame_lengths: the f16 model takes none (it is the TFLite export's graph, which has no mask)")
        t = frame_lengths if isinstance(frame_lengths, torch.Tensor) else torch.as_tensor(np.asarray(frame_lengths))
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool or t.ndim != 1 or t.shape[0] != B:
            raise ValueError(f"frame_lengths must be {B} integers (one per clip of the batch), got {tuple(t.shape)} {t.dtype}")
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def __call__(self, x, training: bool = False, seed: Optional[int] = None, frame_lengths=None) -> torch.Tensor:
        """model(x, training=...).  frame_lengths [B]: clip b has that many real frames and the rest of its T rows is padding — the
        attention keys, the ECA mean and the Squeeze-Excite mean leave the padding out (the mask the reference's layers take, DESIGN §2
        "Frame lengths"); everything else, BatchNorm statistics included, sees the padded frames as without lengths."""
        x = self._as_input(x)
        B = x.shape[0]
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch}")
        fl = self._as_frame_lengths(frame_lengths, B)
        logits = torch.empty((B, self.T, self.C), dtype=torch.float32, device=self.device)
        if seed is None:
            seed = (self._step_seed + 0x9E3779B1 * self._steps) & 0xFFFFFFFF
        if fl is None:
            _lib.check(self._lib.ishara_forward(self._h, _lib.ptr(x), B, _lib.ptr(logits), 1 if training else 0,
                                                C.c_uint32(seed), _stream()), "ishara_forward")
        else:
            _lib.check(self._lib.ishara_forward_ex(self._h, _lib.ptr(x), B, _lib.ptr(logits), 1 if training else 0,
                                                   C.c_uint32(seed), _lib.ptr(fl), _stream()), "ishara_forward_ex")
        self._last_x = x          # keep the input alive: the stem weight gradient re-reads it
        self._last_fl = fl        # and the lengths: the backward pass is handed the same array
        return logits

    predict = __call__

    def compile(self, loss=None, optimizer=None):
        """model.compile(loss=CTCLoss, optimizer=Lookahead(RAdam)) — c7:70.  Only that pair exists
        in the HIP library; `loss`/`optimizer` are accepted for signature parity."""
        if optimizer is not None and isinstance(optimizer, Optimizer):
            self.optimizer = optimizer
        return self

    # ------------------------------------------------------------------ training
    def loss_and_gradients(self, x, y, seed: Optional[int] = None, loss_scale: float = 1.0, frame_lengths=None, teacher_logits=None):
        """forward(training=True) + CTCLoss + backward.  Returns (loss tensor[1], logits).  frame_lengths: as in __call__, for both passes;
        the CTC loss keeps logit_length = T (c6:3) — a per-clip loss is ctc_loss(..., frame_lengths=).  teacher_logits: with distillation
        active (optimizer.kd_weight > 0 and kd_start_step reached), fp32 [B,T,C] rows on the device that stand in for the attached
        teacher; otherwise not looked at."""
        kd = self._kd_begin_step()
        rows = None
        if kd is not None:      # the teacher runs in front of the student's training forward, once per (micro)batch
            rows = self._kd_rows if self._kd_rows is not None else self._teacher_rows(x, frame_lengths, teacher_logits)
        logits = self(x, training=True, seed=seed, **_fl_kw(frame_lengths))
        fl = self._last_fl
        y = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(self.device, torch.int64).contiguous()
        B = logits.shape[0]
        if y.shape != (B, self._cfg.max_label_len):
            raise ValueError(f"labels must be [B,{self._cfg.max_label_len}] padded with {self.C - 1}")
        mw = self._mwer_begin_step(B)
        if kd is not None:
            self._kd_loss_backward(kd, mw, rows, logits, y, B, loss_scale, fl)
        elif mw is not None:
            self._mwer_loss_backward(mw, logits, y, B, loss_scale, fl)
        elif fl is None:
            _lib.check(self._lib.ishara_loss_backward(self._h, _lib.ptr(logits), _lib.ptr(y), B, _lib.ptr(self._loss_buf),
                                                      _lib.ptr(self._nll_buf), C.c_float(loss_scale), _stream()), "ishara_loss_backward")
        else:
            _lib.check(self._lib.ishara_loss_backward_ex(self._h, _lib.ptr(logits), _lib.ptr(y), B, _lib.ptr(self._loss_buf), _lib.ptr(self._nll_buf),
                                                         C.c_float(loss_scale), _lib.ptr(fl), _stream()), "ishara_loss_backward_ex")
        return self._loss_buf, logits

    def apply_gradients(self):
        """The optimizer step on `grads`.  With optimizer.global_clipnorm or .skip_nonfinite set: the statistics of `grads`, then the step
        that reads them (no all-reduce here: train_on_batch places it in front of the statistics).  Accumulation is train_on_batch's."""
        k, clip, skip = self.optimizer.train_options()
        self._not_while_averaged("apply_gradients")
        if k > 1 or self._micro:
            raise ValueError("apply_gradients steps on one gradient; with accumulate_steps > 1 drive the cycle through train_on_batch")
        if clip > 0.0 or skip:
            src = self.grads[:self.n_train]
            self._launch_grad_stats(src, 1.0, clip)
            self._apply_gradients_ex(src, skip)
            return
        wd = float(self.optimizer.weight_decay) if self.optimizer.apply_weight_decay else 0.0
        ema = self._ema_begin_step()
        pg = self._pg_begin_step()
        if pg is None:
            _lib.check(self._lib.ishara_optimizer_step(self._h, C.c_float(float(self.optimizer.learning_rate)), C.c_float(wd), _stream()),
                       "ishara_optimizer_step")
        else:
            self._step_groups(pg, wd, None, None, False)
        if ema:
            self._ema_update(ema, None, False)
        self.optimizer.iterations += 1
        self._steps += 1

    def train_on_batch(self, x, y, seed: Optional[int] = None, allreduce: bool = True, frame_lengths=None, teacher_logits=None) -> torch.Tensor:
        """One Keras train_step (c12): forward, CTC, backward, [RCCL grad all-reduce], update.
        Returns the device loss tensor (no host sync).  `allreduce=False` skips the gradient exchange (bench.py's diagnostic
        of the exposed all-reduce time; replicas diverge — never for training).

        With `optimizer.global_clipnorm`, `.skip_nonfinite` or `.accumulate_steps` > 1 set, a call is one microbatch of a cycle of
        k = accumulate_steps: forward, CTC, backward (loss_scale 1/world), the gradient added into an accumulator (k > 1); the k-th call then
        all-reduces the accumulator once, takes the statistics of the summed gradient with grad_scale = 1/k (after the all-reduce, so
        every rank sees the same norm) and steps the optimizer on gradient * coef.  `_steps` and `optimizer.iterations` advance once per
        cycle; microbatch j draws its dropout masks from seed index `_steps * k + j`.  The bucketed all-reduce overlap
        (parallel.overlap_enabled) applies only when accumulate_steps == 1; otherwise the accumulator is reduced in one piece.  Still no
        host sync: `grad_stats()` reads the record when asked.

        `frame_lengths` [B]: per-clip frame counts of this (micro)batch, as in __call__; every path above takes them.

        With `optimizer.awp_delta` set and `optimizer.iterations` >= `awp_start_step`, the gradient of every (micro)batch on every path
        above is the adversarial one (_loss_and_gradients_step: two passes around ishara_awp_perturb / ishara_awp_restore); the loss
        returned is the first pass's, the all-reduce stays where it is, behind the second pass.

        With `optimizer.kd_weight` > 0 and `optimizer.iterations` >= `kd_start_step`, the gradient of every (micro)batch on every path above
        carries the distillation term (ishara_amd/kd.py).  The teacher of set_teacher runs once per call, in inference mode on the step's
        stream, in front of the student's forward; AWP's second pass reuses its rows.  `teacher_logits` (fp32 [B,T,C] on the device: an
        offline-cached teacher) stands in for it."""
        from . import parallel
        k, clip, skip = self.optimizer.train_options()
        self._not_while_averaged("train_on_batch")
        if k > 1 or clip > 0.0 or skip or self._micro:
            return self._train_microbatch(x, y, seed, allreduce, k, clip, skip, frame_lengths, teacher_logits)
        world = parallel.world_size()
        if not allreduce:
            loss = self._loss_and_gradients_step(x, y, seed, 1.0 / world, frame_lengths, teacher_logits=teacher_logits)
            self.apply_gradients()
            return loss
        overlap = world > 1 and parallel.overlap_enabled()
        if overlap:
            self.enable_grad_buckets()
        if seed is None and world > 1:
            # replicas share the weight-initialisation seed but draw independent dropout / drop-path masks for their shards,
            # like the reference's replicas (tf.distribute / nn.DataParallel keep per-replica RNG streams)
            seed = ((self._step_seed + 0x9E3779B1 * self._steps) ^ (parallel.rank() * 0x85EBCA6B)) & 0xFFFFFFFF
        loss = self._loss_and_gradients_step(x, y, seed, 1.0 / world, frame_lengths, teacher_logits=teacher_logits)
        if overlap:
            parallel.allreduce_buckets_(self)          # ranges of the gradient reduced on a side stream as the backward pass finishes them
        elif world > 1:
            parallel.allreduce_sum_(self.grads[:self.n_train])
        self.apply_gradients()
        return loss

    def _train_microbatch(self, x, y, seed, allreduce, k, clip, skip, frame_lengths=None, teacher_logits=None) -> torch.Tensor:
        """microbatch `_micro` of a cycle of k; the k-th one ends the cycle with all-reduce, statistics and the step"""
        from . import parallel
        world = parallel.world_size()
        if self._micro >= k:
            raise ValueError(f"accumulate_steps was lowered to {k} in the middle of a cycle ({self._micro} microbatches summed)")
        overlap = allreduce and k == 1 and world > 1 and parallel.overlap_enabled()
        if overlap:
            self.enable_grad_buckets()
        if seed is None:
            seed = (self._step_seed + 0x9E3779B1 * (self._steps * k + self._micro)) & 0xFFFFFFFF
            if world > 1:
                seed = (seed ^ (parallel.rank() * 0x85EBCA6B)) & 0xFFFFFFFF
        loss = self._loss_and_gradients_step(x, y, seed, 1.0 / world, frame_lengths, ends_cycle=self._micro + 1 >= k, teacher_logits=teacher_logits)
        src = self.grads[:self.n_train]
        if k > 1:
            if self._grad_acc is None:
                self._grad_acc = torch.empty(self.n_train, dtype=torch.float32, device=self.device)
            _lib.check(self._lib.ishara_gradient_accumulate(self._h, _lib.ptr(self._grad_acc), _lib.ptr(src), self.n_train,
                                                            1 if self._micro == 0 else 0, _stream()), "ishara_gradient_accumulate")
            self._micro += 1
            if self._micro < k:
                return loss
            src = self._grad_acc
        if overlap:
            parallel.allreduce_buckets_(self)
        elif allreduce and world > 1:
            parallel.allreduce_sum_(src)
        self._launch_grad_stats(src, 1.0 / k, clip)
        self._apply_gradients_ex(src, skip)
        self._micro = 0
        return loss

    def _launch_grad_stats(self, src: torch.Tensor, grad_scale: float, clip: float):
        """norm / coef / nonfinite of `src` into the device record (allocated, zeroed, on first use)"""
        if self._gstats is None:
            self._gstats = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._gstats_ws = torch.empty(int(self._lib.ishara_grad_stats_workspace_bytes(self.n_train)), dtype=torch.uint8, device=self.device)
        self._mask_frozen(src)         # a frozen tensor's gradient counts neither in the norm nor in the non-finite guard
        _lib.check(self._lib.ishara_gradient_stats(self._h, _lib.ptr(src), src.numel(), C.c_float(grad_scale), C.c_float(clip),
                                                   _lib.ptr(self._gstats), _lib.ptr(self._gstats_ws), _stream()), "ishara_gradient_stats")

    def _apply_gradients_ex(self, src: torch.Tensor, skip: bool):
        self._not_while_averaged("the optimizer step")
        wd = float(self.optimizer.weight_decay) if self.optimizer.apply_weight_decay else 0.0
        ema = self._ema_begin_step()
        pg = self._pg_begin_step()
        if pg is None:
            _lib.check(self._lib.ishara_optimizer_step_ex(self._h, C.c_float(float(self.optimizer.learning_rate)), C.c_float(wd), _lib.ptr(src),
                                                          _lib.ptr(self._gstats), 1 if skip else 0, _stream()), "ishara_optimizer_step_ex")
        else:
            self._step_groups(pg, wd, src, self._gstats, skip)
        if ema:
            self._ema_update(ema, self._gstats, skip)
        self.optimizer.iterations += 1
        self._steps += 1

    # ------------------------------------------------------------------ optimizer parameter groups (csrc/optimizer.hip)
    def _pg_begin_step(self):
        """In front of a (micro)batch and of an optimizer step: None when optimizer.param_groups is None (and then nothing of the feature is
        touched, allocated or launched), else the device tables.  The groups are resolved against the entry names and the 16-byte rows
        uploaded only when the option changed by value since the last look; a change in the middle of an accumulation cycle, or inside
        averaged_weights(), is refused."""
        raw = self.optimizer.param_groups
        if raw is None and self._pg_key is None:
            return None
        if self._pg_key is not None and type(raw) is type(self._pg_seen) and raw == self._pg_seen:      # unchanged by value: no check, no JSON
            return self._pg
        from . import train_state as TS
        groups = self.optimizer.group_options()
        key = None if groups is None else TS.param_groups_json(groups)
        if key != self._pg_key:
            self._not_while_averaged("a change of optimizer.param_groups")
            if self._micro:
                raise ValueError(f"optimizer.param_groups changed in the middle of an accumulation cycle ({self._micro} microbatches summed)")
            if key is not None:
                seg, rows = TS.param_group_rows(self.entries, self.n_train, groups)
                S = len(rows)
                if self._pg is None:
                    ws_bytes = int(self._lib.ishara_param_groups_workspace_bytes(self.n_train, S))
                    if ws_bytes < 0:
                        _lib.check(-1, "ishara_param_groups_workspace_bytes")
                    self._pg = dict(seg=torch.from_numpy(seg).to(self.device), S=S, rows=torch.empty(4 * S, dtype=torch.int32, device=self.device),
                                    ws=torch.empty(ws_bytes, dtype=torch.uint8, device=self.device), frozen=False)
                self._pg["rows"].copy_(torch.from_numpy(rows.view(np.int32).copy()))
                self._pg["frozen"] = bool((rows["frozen"] != 0).any())
            self._pg_key = key
        self._pg_seen = copy.deepcopy(raw)
        return None if key is None else self._pg

    def _step_groups(self, pg, wd: float, src, gstats, skip: bool):
        _lib.check(self._lib.ishara_optimizer_step_groups(self._h, C.c_float(float(self.optimizer.learning_rate)), C.c_float(wd), _lib.ptr(src),
                                                          _lib.ptr(gstats), 1 if skip else 0, _lib.ptr(pg["seg"]), _lib.ptr(pg["rows"]), pg["S"],
                                                          _lib.ptr(pg["ws"]), _stream()), "ishara_optimizer_step_groups")

    def _mask_frozen(self, g: torch.Tensor):
        """g = +0.0 over the frozen tensors: one launch, only when the groups freeze something"""
        pg = self._pg_begin_step()
        if pg is None or not pg["frozen"]:
            return
        _lib.check(self._lib.ishara_gradient_mask_groups(self._h, _lib.ptr(g), self.n_train, _lib.ptr(pg["seg"]), _lib.ptr(pg["rows"]), pg["S"],
                                                         _lib.ptr(pg["ws"]), _stream()), "ishara_gradient_mask_groups")

    def param_groups(self) -> Dict[str, dict]:
        """{trainable entry name: {lr_scale, weight_decay_scale, trainable}} as optimizer.param_groups resolves (all defaults when it is None)"""
        from . import train_state as TS
        return TS.resolve_param_groups(self.entries, self.optimizer.group_options())

    # ------------------------------------------------------------------ minimum-risk training over the beam's n-best (ishara_amd/mwer.py)
    def _mwer_begin_step(self, B: int):
        """The checked mwer_* options when this step adds the risk term (optimizer.mwer_nbest > 0 and optimizer.iterations has reached
        mwer_start_step), else None (and then nothing of it is touched, allocated or launched).  The first such step allocates the
        buffers: the n-best list, its scores, the weights, the beam search's and the gradient stage's workspaces, for max_batch clips."""
        o = self.optimizer
        if not o.mwer_nbest:
            return None
        opts = o.mwer_options()
        if opts["mwer_nbest"] == 0 or o.iterations < opts["mwer_start_step"]:
            return None
        from . import ctc_beam, mbr, mwer
        N, W, L = opts["mwer_nbest"], opts["mwer_beam_width"], self._cfg.max_label_len
        if L > mwer.MAX_TARGET_LEN:
            raise ValueError(f"minimum-risk training takes targets of at most {mwer.MAX_TARGET_LEN} symbols, max_label_len is {L}")
        key = (N, W)
        if self._mwer is None or self._mwer["key"] != key:
            ctc_beam.check_device_args(self.C, self.T, W, N)
            Bm, T, dev = self.max_batch, self.T, self.device
            i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
            max_len = min(mwer.MAX_HYP_LEN, L)        # a hypothesis longer than every label leaves the list: it sizes the lattice workspace
            self._mwer = dict(key=key, max_len=max_len, idx=torch.empty((Bm, N, T), **i32), len=torch.empty((Bm, N), **i32), score=torch.empty((Bm, N), **f32),
                              logp=torch.empty((Bm, N), **f32), status=torch.empty((Bm, N), **i32), tgt=torch.empty((Bm, L), **i32),
                              dist=torch.empty((Bm, N), **i32), post=torch.empty((Bm, N), **f32), risk=torch.empty((Bm,), **f32),
                              coef=torch.empty((Bm, N), **f32), tlen=torch.empty((Bm,), **i32), it=torch.empty((1,), **f32),
                              beam_ws=torch.empty(max(ctc_beam.workspace_bytes(self._lib, Bm, T, self.C, W), 4), dtype=torch.uint8, device=dev),
                              grad_ws=torch.empty(mwer.workspace_bytes(self._lib, Bm, T, N, max_len), dtype=torch.uint8, device=dev), B=0)
        self._mwer["it"].fill_(mbr.inverse_temperature(opts["mwer_temperature"]))
        return opts

    def _mwer_loss_backward(self, opts: dict, logits, y, B: int, loss_scale: float, fl) -> None:
        """search (no LM) -> exact scores -> weights -> ishara_loss_backward_nbest, all on the current stream; nothing waits"""
        m, lib, st = self._mwer, self._lib, _stream()
        N, T = m["key"][0], self.T
        self._mwer_prepare(opts, logits, y, B)
        _lib.check(lib.ishara_loss_backward_nbest(self._h, _lib.ptr(logits), _lib.ptr(y), B, _lib.ptr(self._loss_buf), _lib.ptr(self._nll_buf),
                                                  C.c_float(loss_scale * opts["mwer_ctc_weight"]), _lib.ptr(fl), _lib.ptr(m["idx"]), _lib.ptr(m["len"]), N, T,
                                                  m["max_len"], _lib.ptr(m["coef"]), C.c_float(loss_scale * opts["mwer_weight"]), _lib.ptr(m["grad_ws"]), st),
                   "ishara_loss_backward_nbest")
        m["B"] = B

    def _mwer_prepare(self, opts: dict, logits, y, B: int) -> None:
        """the n-best list of the step's logits, its exact scores and the weights coef, into the buffers of _mwer_begin_step"""
        from . import ctc_beam, mwer
        m, lib, st = self._mwer, self._lib, _stream()
        N, W = m["key"]
        T, Cn, L = self.T, self.C, self._cfg.max_label_len
        ctc_beam.launch(lib, logits, B, T, Cn, W, N, None, 0.0, 0.0, m["beam_ws"], m["idx"], m["len"], m["score"], st, ex=True)
        _lib.check(lib.ishara_ctc_score_nbest(_lib.ptr(logits), B, T, Cn, Cn - 1, _lib.ptr(m["idx"]), _lib.ptr(m["len"]), N, T, None, _lib.ptr(m["logp"]),
                                              _lib.ptr(m["status"]), st), "ishara_ctc_score_nbest")
        # a slot the gradient stage will not take (longer than max_len) is not live for the weights either; the labels' padding (the blank
        # C - 1) becomes the targets' 59
        m["status"][:B] = torch.where(m["len"][:B] > m["max_len"], torch.full_like(m["status"][:B], mwer.STATUS_LONG), m["status"][:B])
        m["tgt"][:B] = torch.where(y == Cn - 1, torch.full_like(y, PAD_TOKEN_IDX), y).to(torch.int32)
        mwer.launch_weights(lib, m["idx"], m["len"], m["logp"], m["status"], B, N, T, m["tgt"], L, m["it"], 1 if opts["mwer_normalise"] else 0,
                            m["dist"], m["post"], m["risk"], m["coef"], m["tlen"], st)

    def mwer_stats(self) -> Dict[str, float]:
        """The last step that added the risk term, read on request (one device-to-host copy): risk, the mean expected distance of the
        batch's clips that have a live hypothesis; top_distance, the mean plain edit distance of the first slot over the clips where it
        is live; live_slots, how many slots of the batch are live; clips, how many clips have one."""
        if self._mwer is None or not self._mwer["B"]:
            raise _lib.IsharaError("mwer_stats: no step has run with minimum-risk training (optimizer.mwer_nbest > 0 and mwer_start_step reached)")
        m = self._mwer
        B = m["B"]
        risk, dist = m["risk"][:B].cpu().numpy().astype(np.float64), m["dist"][:B].cpu().numpy()
        has, top = np.isfinite(risk), dist[:, 0] >= 0
        return dict(risk=float(risk[has].mean()) if has.any() else float("nan"), top_distance=float(dist[top, 0].mean()) if top.any() else float("nan"),
                    live_slots=int((dist >= 0).sum()), clips=int(has.sum()))

    # ------------------------------------------------------------------ knowledge distillation from a teacher (ishara_amd/kd.py)
    def set_teacher(self, teacher, weights=None, mode: str = "log-linear"):
        """Attaches the teacher of optimizer.kd_weight > 0.  `teacher`: a Model with this model's T, C and input features (any width, depth
        or dtype); a list of 1..8 such models, fused per batch by ensemble.combine_logits with `weights` (None: uniform) and `mode`
        ("log-linear" or "linear"); or a callable (x [B,T,F] fp32 on the device, frame_lengths or None) -> fp32 [B,T,C] device tensor of
        logits or log-probabilities.  None detaches.  The teacher is not part of save_state."""
        if teacher is None:
            self._teacher = None
            return self
        if isinstance(teacher, Model) or (isinstance(teacher, (list, tuple)) and all(isinstance(t, Model) for t in teacher)):
            from . import ensemble
            models = [teacher] if isinstance(teacher, Model) else list(teacher)
            if not 1 <= len(models) <= ensemble.MAX_MODELS:
                raise ValueError(f"{len(models)} teacher models: the fusion takes 1..{ensemble.MAX_MODELS}")
            for i, t in enumerate(models):
                if (t.T, t.C, t.F) != (self.T, self.C, self.F):
                    raise ValueError(f"teacher {i} has (T, C, F) = {(t.T, t.C, t.F)}, the student {(self.T, self.C, self.F)}: distillation needs the same "
                                     "frames, alphabet and input features")
                if getattr(t, "device", None) != getattr(self, "device", None):
                    raise ValueError(f"teacher {i} lives on {getattr(t, 'device', None)}, the student on {getattr(self, 'device', None)}")
            md = {"log-linear": "log_linear", "log_linear": "log_linear", "linear": "linear"}.get(mode)
            if md is None:
                raise ValueError(f"mode must be 'log-linear' or 'linear', got {mode!r}")
            if len(models) == 1 and weights is not None:
                ensemble.normalise_weights(weights, 1)
            w = ensemble.normalise_weights(weights, len(models)) if len(models) > 1 else None
            self._teacher = ("models", models, w, md)
        elif callable(teacher):
            if weights is not None:
                raise ValueError("weights belong to a list of teacher models, not to a callable")
            self._teacher = ("callable", teacher)
        else:
            raise ValueError(f"teacher must be a Model, a list of Models, a callable or None, got {type(teacher).__name__}")
        return self

    def _kd_begin_step(self):
        """The checked kd_* options when this step adds the distillation term (optimizer.kd_weight > 0 and optimizer.iterations has reached
        kd_start_step), else None (and then nothing of it is touched, allocated or launched).  The first such step allocates kl_frame
        and kl_clip for max_batch clips."""
        o = self.optimizer
        if not o.kd_weight:
            return None
        opts = o.kd_options()
        if opts["kd_weight"] == 0 or o.iterations < opts["kd_start_step"]:
            return None
        if self._kd is None:
            f32 = dict(dtype=torch.float32, device=self.device)
            self._kd = dict(kl_frame=torch.empty((self.max_batch, self.T), **f32), kl_clip=torch.empty((self.max_batch,), **f32), B=0, mean=False)
        return opts

    def _teacher_rows(self, x, frame_lengths, teacher_logits) -> torch.Tensor:
        """The teacher's rows [B,T,C] fp32 of this (micro)batch on the current stream, in inference mode: teacher_logits when given, else
        one forward of every attached model (fused by combine_logits when there are several), or one call of the callable."""
        x = self._as_input(x)
        B = x.shape[0]
        want = (B, self.T, self.C)
        if teacher_logits is None and self._teacher is None:
            raise _lib.IsharaError("distillation is on (optimizer.kd_weight > 0 and kd_start_step reached) but no teacher is attached: call "
                                   "set_teacher(...) or pass teacher_logits= (a restored state holds the options, never the teacher)")
        with torch.no_grad():
            if teacher_logits is not None:
                rows, what = teacher_logits, "teacher_logits"
            elif self._teacher[0] == "callable":
                rows, what = self._teacher[1](x, self._as_frame_lengths(frame_lengths, B)), "the teacher's output"
            else:
                _, models, w, md = self._teacher
                outs = [t(x, training=False, **({} if frame_lengths is None or t._cfg.dtype == _lib.F16 else dict(frame_lengths=frame_lengths))) for t in models]
                if len(outs) == 1:
                    rows, what = outs[0], "the teacher's logits"
                else:
                    from . import ensemble
                    rows, what = ensemble.combine_logits(outs, w, md), "the fused teachers' rows"
        if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != want or rows.dtype != torch.float32 or rows.device != self.device:
            got = f"{tuple(rows.shape)} {rows.dtype} on {rows.device}" if isinstance(rows, torch.Tensor) else type(rows).__name__
            raise ValueError(f"{what} must be a float32 {list(want)} tensor on {self.device}, got {got}")
        return rows.detach().contiguous()

    def _kd_loss_backward(self, opts: dict, mw: Optional[dict], rows, logits, y, B: int, loss_scale: float, fl) -> None:
        """ishara_loss_backward_kd on the current stream: the CTC kernel, the n-best stage when minimum-risk training is active as well
        (its search, scores and weights first), then the distillation stage; nothing waits"""
        from . import kd as KD
        k = self._kd
        tau = opts["kd_temperature"]
        ctc_scale = loss_scale * opts["kd_ctc_weight"]
        stage = _lib.KdStage(rows.data_ptr(), KD.inverse_temperature(tau), 1 if opts["kd_normalise"] else 0, loss_scale * opts["kd_weight"] * tau,
                             k["kl_frame"].data_ptr(), k["kl_clip"].data_ptr())
        nb = None
        if mw is not None:
            m = self._mwer
            self._mwer_prepare(mw, logits, y, B)
            ctc_scale *= mw["mwer_ctc_weight"]
            nb = C.byref(_lib.NbestStage(m["idx"].data_ptr(), m["len"].data_ptr(), m["key"][0], self.T, m["max_len"], m["coef"].data_ptr(),
                                         loss_scale * mw["mwer_weight"], m["grad_ws"].data_ptr()))
        _lib.check(self._lib.ishara_loss_backward_kd(self._h, _lib.ptr(logits), _lib.ptr(y), B, _lib.ptr(self._loss_buf), _lib.ptr(self._nll_buf),
                                                     C.c_float(ctc_scale), _lib.ptr(fl), C.byref(stage), nb, _stream()), "ishara_loss_backward_kd")
        if mw is not None:
            self._mwer["B"] = B
        k["B"], k["mean"] = B, bool(opts["kd_normalise"])

    def kd_stats(self) -> Dict[str, float]:
        """The last step that added the distillation term, read on request (one device-to-host copy): kl, the batch's mean of the clips'
        KL(teacher || student) at the step's temperature (per frame with kd_normalise, summed over the T frames without); per_frame,
        which of the two; clips, the batch size."""
        if self._kd is None or not self._kd["B"]:
            raise _lib.IsharaError("kd_stats: no step has run with distillation (optimizer.kd_weight > 0 and kd_start_step reached)")
        B = self._kd["B"]
        kl = self._kd["kl_clip"][:B].cpu().numpy().astype(np.float64)
        return dict(kl=float(kl.mean()), per_frame=self._kd["mean"], clips=int(B))

    # ------------------------------------------------------------------ adversarial weight perturbation (csrc/awp.hip)
    def _awp_begin_step(self):
        """In front of a (micro)batch of train_on_batch: the checked AWP options when the perturbation is configured and the step number has
        reached awp_start_step, else None (and then nothing of it is touched, allocated or launched).  The first active step allocates
        the backup of the trainable prefix, the segment table (one segment per trainable entry), the scale array, the 16-byte record, the
        workspace and the two loss tensors; nothing of it needs initialising."""
        opts = self.optimizer.awp_options()
        if opts[0] is None or self.optimizer.iterations < opts[2]:
            return None
        if self._awp_backup is None:
            from . import train_state as TS
            seg = TS.awp_segments(self.entries, self.n_train)
            S = len(seg) - 1
            ws_bytes = int(self._lib.ishara_awp_workspace_bytes(self.n_train, S))
            if ws_bytes < 0:
                _lib.check(-1, "ishara_awp_workspace_bytes")
            f32 = dict(dtype=torch.float32, device=self.device)
            self._awp = dict(seg=torch.from_numpy(seg).to(self.device), S=S, scale=torch.zeros(S, **f32),
                             rec=torch.zeros(4, dtype=torch.int32, device=self.device), ws=torch.empty(ws_bytes, dtype=torch.uint8, device=self.device),
                             clean=torch.zeros(1, **f32), adv=torch.zeros(1, **f32), ran=False)
            self._awp_backup = torch.empty(self.n_train, **f32)
        return opts

    def _loss_and_gradients_step(self, x, y, seed, loss_scale: float, frame_lengths, ends_cycle: bool = True, teacher_logits=None) -> torch.Tensor:
        """The gradient of one (micro)batch of train_on_batch -> its loss tensor.  Without AWP: loss_and_gradients, as ever.  With it:
        pass 1 at loss scale 1 (the perturbation does not depend on the world size; no collective), ishara_awp_perturb on the trainable
        prefix by that gradient, pass 2 at the perturbed weights with the same seed (the dropout and drop-path masks the adversary was
        computed for) and the caller's loss scale, ishara_awp_restore.  `grads` then hold the second gradient; the loss returned is the
        first pass's, in a tensor of the helper's own, comparable with a run without AWP.  The weight shadows are refreshed behind the
        perturbation, and behind the restore by the optimizer step that follows, or here when the microbatch does not end its cycle
        (ends_cycle False).  No host synchronise."""
        self._pg_begin_step()          # a change of the groups in the middle of a cycle is refused before any work
        if self._kd_begin_step() is None:
            return self._loss_and_gradients_passes(x, y, seed, loss_scale, frame_lengths, ends_cycle)
        self._kd_rows = self._teacher_rows(x, frame_lengths, teacher_logits)      # once per (micro)batch: both of AWP's passes read these rows
        try:
            return self._loss_and_gradients_passes(x, y, seed, loss_scale, frame_lengths, ends_cycle)
        finally:
            self._kd_rows = None

    def _loss_and_gradients_passes(self, x, y, seed, loss_scale: float, frame_lengths, ends_cycle: bool) -> torch.Tensor:
        """the one pass, or AWP's two, of _loss_and_gradients_step"""
        awp = self._awp_begin_step()
        if awp is None:
            return self.loss_and_gradients(x, y, seed=seed, loss_scale=loss_scale, **_fl_kw(frame_lengths))[0]
        delta, eps, _, relative = awp
        a = self._awp
        if seed is None:                # both passes draw the masks __call__ would have drawn for this step
            seed = (self._step_seed + 0x9E3779B1 * self._steps) & 0xFFFFFFFF
        self.loss_and_gradients(x, y, seed=seed, loss_scale=1.0, **_fl_kw(frame_lengths))
        a["clean"].copy_(self._loss_buf)
        self._mask_frozen(self.grads[:self.n_train])       # a frozen tensor is not perturbed (a zero gradient: a step of 0) and is not in the norms
        _lib.check(self._lib.ishara_awp_perturb(self._h, _lib.ptr(self.params), _lib.ptr(self._awp_backup), _lib.ptr(self.grads), _lib.ptr(a["seg"]),
                                                a["S"], self.n_train, C.c_float(delta), C.c_float(eps), 1 if relative else 0, _lib.ptr(a["scale"]),
                                                _lib.ptr(a["rec"]), _lib.ptr(a["ws"]), _stream()), "ishara_awp_perturb")
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")
        self.loss_and_gradients(x, y, seed=seed, loss_scale=loss_scale, **_fl_kw(frame_lengths))
        a["adv"].copy_(self._loss_buf)
        _lib.check(self._lib.ishara_awp_restore(self._h, _lib.ptr(self.params), _lib.ptr(self._awp_backup), self.n_train, _stream()), "ishara_awp_restore")
        if not ends_cycle:
            _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")
        a["ran"] = True
        return a["clean"]

    def _awp_required(self, what: str):
        if self._awp is None or not self._awp["ran"]:
            raise _lib.IsharaError(f"{what}: no step has run with adversarial weight perturbation (optimizer.awp_delta set and awp_start_step reached)")

    def awp_stats(self) -> Dict[str, float]:
        """{grad_norm, delta_norm, perturbed, zeroed, clean_loss, adv_loss} of the last perturbed (micro)batch: the norm of its first
        gradient and of the perturbation over the tensors that were perturbed, how many tensors were perturbed and how many were left alone
        (a NaN or Inf in their gradient), the loss at the weights and at the perturbed weights.  This read is the only host synchronise of
        the feature."""
        self._awp_required("awp_stats")
        raw = self._awp["rec"].cpu().numpy()
        return dict(grad_norm=float(raw[:2].view(np.float32)[0]), delta_norm=float(raw[:2].view(np.float32)[1]), perturbed=int(raw[2]), zeroed=int(raw[3]),
                    clean_loss=float(self._awp["clean"].item()), adv_loss=float(self._awp["adv"].item()))

    def awp_scales(self) -> Dict[str, float]:
        """{entry name: the factor its gradient was multiplied by} of the last perturbed (micro)batch, 0.0 for a tensor left alone"""
        self._awp_required("awp_scales")
        names = [n for _, n in sorted((o, n) for n, _, o, t in self.entries if t)]
        return dict(zip(names, (float(v) for v in self._awp["scale"].cpu().numpy())))

    # ------------------------------------------------------------------ moving average of the weights (csrc/weight_avg.hip)
    def _not_while_averaged(self, what: str):
        if self._ema_swapped:
            raise _lib.IsharaError(f"{what}: refused inside averaged_weights(): params hold the moving average, not the training weights")

    def _ema_start(self, updates: int = 0):
        """a fresh average at the present params[:n_train] (Keras: initial_value=var) and the record with `updates`; no host synchronise"""
        self._ema_avg = self.params[:self.n_train].detach().clone()
        self._ema_rec = torch.zeros(2, dtype=torch.int64, device=self.device)
        if updates:
            self._ema_rec[0] = int(updates)

    def _ema_begin_step(self):
        """In front of an optimizer step: the checked EMA options when optimizer.use_ema is on, else None (and then nothing of the
        average is touched, allocated or launched).  The first such step creates the average at the weights the step starts from."""
        opts = self.optimizer.ema_options()
        if not opts[0]:
            return None
        if self._ema_avg is None:
            self._ema_start()
        return opts

    def _ema_update(self, opts, gstats, skip: bool):
        """ishara_weight_average behind the optimizer step on the same stream; with an overwrite frequency the 16-bit weight shadows are
        refreshed behind it (the host cannot know whether this launch overwrote without reading the record)"""
        _, momentum, every, warmup = opts
        _lib.check(self._lib.ishara_weight_average(self._h, _lib.ptr(self._ema_avg), _lib.ptr(self.params), self.n_train, C.c_float(momentum),
                                                   1 if warmup else 0, every, _lib.ptr(self._ema_rec), _lib.ptr(gstats), 1 if skip else 0,
                                                   _stream()), "ishara_weight_average")
        if every:
            _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")

    def _ema_required(self, what: str):
        if self._ema_avg is None:
            raise _lib.IsharaError(f"{what}: there is no moving average: no training step has run with optimizer.use_ema set")

    def ema_weights(self) -> Dict[str, np.ndarray]:
        """get_weights() of the averaged model: the trainable entries from the moving average, the others (the BatchNorm moving
        statistics, which are not averaged) from `params`."""
        self._ema_required("ema_weights")
        flat = self.params.detach().cpu().numpy().copy()
        if not self._ema_swapped:                              # inside averaged_weights() the average is what params hold
            flat[:self.n_train] = self._ema_avg.cpu().numpy()
        return {n: flat[o:o + int(np.prod(s))].reshape(s).copy() for n, s, o, _ in self.entries}

    def ema_state(self) -> dict:
        """{updates, alpha, overwrote} of the device record: the updates applied so far, the smoothing factor of the last one and whether
        it overwrote the weights.  This read is the only host synchronise of the feature."""
        self._ema_required("ema_state")
        raw = self._ema_rec.cpu().numpy()
        return dict(updates=int(raw[0]), alpha=float(raw[1:].view(np.float32)[0]), overwrote=int(raw[1:].view(np.int32)[1]))

    def _ema_swap(self):
        _lib.check(self._lib.ishara_weight_swap(self._h, _lib.ptr(self.params), _lib.ptr(self._ema_avg), self.n_train, _stream()), "ishara_weight_swap")
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")

    @contextlib.contextmanager
    def averaged_weights(self):
        """with model.averaged_weights(): ... runs the body on the moving average: params[:n_train] and the average change places on the
        device (bit for bit, no copy through the host) and the weight shadows are refreshed; on exit, also through an exception, they change
        back.  The BatchNorm moving statistics are not averaged and stay.  Training, nesting, and entering without an average are refused."""
        self._ema_required("averaged_weights")
        if self._ema_swapped:
            raise _lib.IsharaError("averaged_weights: already inside averaged_weights() (nesting would swap the training weights back)")
        self._ema_swap()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swap()
            self._ema_swapped = False

    def finalize_ema(self):
        """Overwrites the trainable weights with their moving average (Keras' optimizer.finalize_variable_values, which `fit` calls after the
        last epoch); the optimizer slots stay, the weight shadows are refreshed."""
        self._ema_required("finalize_ema")
        self._not_while_averaged("finalize_ema")
        self.params[:self.n_train].copy_(self._ema_avg)
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")

    def grad_stats(self) -> Dict[str, float]:
        """{norm, coef, nonfinite, skipped} of the last cycle that ran with clipping, skipping or accumulation: the global L2 norm of the
        (mean) gradient, the factor the step applied to the summed gradient, the count of NaN / Inf elements, and the number of steps
        skipped so far.  This read is the only host synchronise of the feature."""
        if self._gstats is None:
            raise _lib.IsharaError("grad_stats: no training step has run with global_clipnorm, skip_nonfinite or accumulate_steps set")
        raw = self._gstats.cpu().numpy()
        f = raw.view(np.float32)
        return dict(norm=float(f[0]), coef=float(f[1]), nonfinite=int(raw[2]), skipped=int(raw[3]))

    # ------------------------------------------------------------------ resumable state
    def save_state(self, path: str) -> str:
        """Everything a preempted run needs to go on as if it had not stopped (train_state.py): parameters with the BatchNorm moving
        statistics, the optimizer slots m / v / slow, the iteration and dropout-seed counters, learning rate, weight decay and the
        clipping / skipping / accumulation settings -> `path` (.npz).  Refused in the middle of an accumulation cycle: the accumulator
        is not part of the state."""
        from . import train_state as TS
        self._not_while_averaged("save_state")
        if self._micro:
            raise ValueError(f"save_state: in the middle of an accumulation cycle ({self._micro} of {self.optimizer.accumulate_steps} microbatches); "
                             "save after the cycle's last train_on_batch")
        o = self.optimizer
        skipped = int(self._gstats.cpu()[3]) if self._gstats is not None else 0
        st = TS.pack_state(self.entries, *(t.detach().cpu().numpy() for t in (self.params, self.opt_m, self.opt_v, self.opt_slow)),
                           iterations=o.iterations, steps=self._steps, step_seed=self._step_seed, learning_rate=float(o.learning_rate),
                           weight_decay=float(o.weight_decay), apply_weight_decay=o.apply_weight_decay, global_clipnorm=o.global_clipnorm,
                           skip_nonfinite=o.skip_nonfinite, accumulate_steps=o.accumulate_steps, skipped=skipped, **self._ema_state_entries(), **self._awp_state_entries(),
                           param_groups=o.group_options(), **self._mwer_state_entries(), **self._kd_state_entries())
        return TS.save_state_file(path, st)

    def _ema_state_entries(self) -> dict:
        """what save_state adds for the moving average: nothing when there is none"""
        if self._ema_avg is None:
            return {}
        use, momentum, every, warmup = self.optimizer.ema_options()
        return dict(ema_avg=self._ema_avg.cpu().numpy(), ema_updates=self.ema_state()["updates"], use_ema=use, ema_momentum=momentum,
                    ema_warmup=warmup, ema_overwrite_frequency=every or None)

    def _mwer_state_entries(self) -> dict:
        """what save_state adds for minimum-risk training: its seven options as one key when it is configured, nothing otherwise"""
        opts = self.optimizer.mwer_options()
        return dict(mwer=opts) if opts["mwer_nbest"] > 0 else {}

    def _kd_state_entries(self) -> dict:
        """what save_state adds for distillation: its five options as one key when it is configured, nothing otherwise; never the teacher"""
        opts = self.optimizer.kd_options()
        return dict(kd=opts) if opts["kd_weight"] > 0 else {}

    def _awp_state_entries(self) -> dict:
        """what save_state adds for adversarial weight perturbation: its four options when it is configured (it has no device state
        beyond them), nothing otherwise"""
        delta, eps, start, relative = self.optimizer.awp_options()
        if delta is None:
            return {}
        return dict(awp_delta=delta, awp_eps=eps, awp_start_step=start, awp_relative=relative)

    def load_state(self, path: str):
        """Restores what save_state wrote into this model (same architecture: the entry list is checked).  A file with a moving average
        restores it, its update count and the four ema settings; a file without one leaves the settings alone and, with optimizer.use_ema
        on, starts a fresh average at the loaded weights with 0 updates.  A file with the options of adversarial weight perturbation sets
        them; a file without them leaves them alone, and so with the optimizer's parameter groups, the options of minimum-risk
        training and those of distillation (whose teacher is never in the file: attach it again with set_teacher)."""
        from . import train_state as TS
        self._not_while_averaged("load_state")
        st = TS.load_state_file(path, self.entries)
        for t, k in ((self.params, "params"), (self.opt_m, "opt_m"), (self.opt_v, "opt_v"), (self.opt_slow, "opt_slow")):
            t.copy_(torch.from_numpy(st[k]))
        o = self.optimizer
        o.iterations, self._steps, self._step_seed, self._micro = st["iterations"], st["steps"], st["step_seed"], 0
        o.learning_rate, o.weight_decay, o.apply_weight_decay = st["learning_rate"], st["weight_decay"], st["apply_weight_decay"]
        o.global_clipnorm, o.skip_nonfinite, o.accumulate_steps = st["global_clipnorm"], st["skip_nonfinite"], st["accumulate_steps"]
        if self._gstats is None:
            self._gstats = torch.zeros(4, dtype=torch.int32, device=self.device)
            self._gstats_ws = torch.empty(int(self._lib.ishara_grad_stats_workspace_bytes(self.n_train)), dtype=torch.uint8, device=self.device)
        self._gstats[3] = st["skipped"]
        self._skipped_seen = st["skipped"]
        if "param_groups" in st:
            o.param_groups = st["param_groups"]
        if "mwer" in st:
            for k, v in st["mwer"].items():
                setattr(o, k, v)
        if "kd" in st:              # the options only: the teacher is attached again with set_teacher
            for k, v in st["kd"].items():
                setattr(o, k, v)
        if "awp_delta" in st:
            o.awp_delta, o.awp_eps, o.awp_start_step, o.awp_relative = st["awp_delta"], st["awp_eps"], st["awp_start_step"], st["awp_relative"]
        self._ema_avg = self._ema_rec = None
        if "ema_avg" in st:
            o.use_ema, o.ema_momentum, o.ema_warmup, o.ema_overwrite_frequency = st["use_ema"], st["ema_momentum"], st["ema_warmup"], st["ema_overwrite_frequency"]
            self._ema_start(st["ema_updates"])
            self._ema_avg.copy_(torch.from_numpy(st["ema_avg"]))
        elif o.ema_options()[0]:
            self._ema_start()
        _lib.check(self._lib.ishara_optimizer_set_iterations(self._h, st["iterations"]), "ishara_optimizer_set_iterations")
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")

    # ---- gradient buckets (all-reduce overlapped with the backward pass; opt-in, see parallel.overlap_enabled)
    def grad_buckets(self) -> List[Tuple[int, int]]:
        """(offset, count) ranges of the flat gradient in the order the backward pass completes them."""
        out = []
        for i in range(int(self._lib.ishara_grad_buckets(self._h))):
            off, cnt = C.c_int64(), C.c_int64()
            _lib.check(self._lib.ishara_grad_bucket(self._h, i, C.byref(off), C.byref(cnt)), "ishara_grad_bucket")
            out.append((int(off.value), int(cnt.value)))
        return out

    def enable_grad_buckets(self):
        _lib.check(self._lib.ishara_grad_buckets_enable(self._h), "ishara_grad_buckets_enable")

    def wait_grad_bucket(self, i: int, side_stream: "torch.cuda.Stream"):
        """Makes `side_stream` wait until bucket i of the last backward pass is final (no host sync)."""
        _lib.check(self._lib.ishara_grad_bucket_wait(self._h, i, C.c_void_p(side_stream.cuda_stream)), "ishara_grad_bucket_wait")

    def fit(self, train_dataset: Iterable, validation_data: Optional[Iterable] = None, epochs: int = 1,
            callbacks: Sequence[Callback] = (), steps_per_epoch: Optional[int] = None, verbose: int = 1, initial_epoch: int = 0) -> History:
        """model.fit(train_dataset, validation_data=, epochs=, callbacks=[...]) — c12:1-10.
        Datasets are re-iterable objects yielding (x [B,T,F] float32, y [B,64] int64) or (x, y, frame_lengths [B]).  `initial_epoch` (Keras): the epoch to start
        from when a run is resumed (after load_state); epochs initial_epoch .. epochs - 1 run.  With optimizer.global_clipnorm or
        .skip_nonfinite the epoch logs gain `grad_norm` (the last cycle's) and `skipped_steps` (in this epoch): one device read per epoch.
        With optimizer.use_ema they gain `ema_updates` (one more read), and after the last epoch, before on_train_end, finalize_ema()
        overwrites the weights with their moving average, as Keras' fit does.
        With accumulate_steps = k every batch is a microbatch; an epoch whose batch count is no multiple of k leaves its last cycle open."""
        hist = History()
        for cb in callbacks:
            if hasattr(cb, "set_model"): cb.set_model(self)
            elif not getattr(cb, "model", None): cb.model = self
        for cb in callbacks: getattr(cb, "on_train_begin", lambda logs=None: None)()
        self.stop_training = False
        for epoch in range(initial_epoch, epochs):
            logs: Dict[str, float] = {}
            for cb in callbacks: cb.on_epoch_begin(epoch, logs)
            tot = torch.zeros(1, dtype=torch.float32, device=self.device)
            n = 0
            for bi, batch in enumerate(train_dataset):
                if steps_per_epoch is not None and bi >= steps_per_epoch:
                    break
                x, y, fl = split_batch(batch)
                tot += self.train_on_batch(x, y, **_fl_kw(fl))
                n += 1
                for cb in callbacks: getattr(cb, "on_train_batch_end", lambda b, logs=None: None)(bi, logs)
            logs["loss"] = float(tot.item()) / max(n, 1)
            logs["lr"] = float(self.optimizer.learning_rate)
            if (self.optimizer.global_clipnorm is not None or self.optimizer.skip_nonfinite) and self._gstats is not None:
                gs = self.grad_stats()
                logs["grad_norm"] = gs["norm"]
                logs["skipped_steps"] = gs["skipped"] - self._skipped_seen
                self._skipped_seen = gs["skipped"]
            if self.optimizer.use_ema and self._ema_avg is not None:
                logs["ema_updates"] = self.ema_state()["updates"]
            if validation_data is not None:
                logs["val_loss"] = self.evaluate(validation_data)
            for cb in callbacks: cb.on_epoch_end(epoch, logs)
            hist.epoch.append(epoch)
            for k, v in logs.items(): hist.history.setdefault(k, []).append(v)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs} - " + " - ".join(f"{k}: {v:.4g}" for k, v in logs.items()))
            if self.stop_training:
                break
        if self.optimizer.use_ema and self._ema_avg is not None:
            self.finalize_ema()
        for cb in callbacks: getattr(cb, "on_train_end", lambda logs=None: None)()
        return hist

    def profile_step(self, x, y, seed: Optional[int] = None) -> Dict[str, dict]:
        """One training step with every kernel launch bracketed by HIP events on the launch stream.
        Returns {kernel family: {launches, ms, bytes (algorithmic), flops}}."""
        _lib.check(self._lib.ishara_profile_enable(self._h, 1))
        try:
            self.train_on_batch(x, y, seed=seed)
            buf = C.create_string_buffer(1 << 16)
            n = self._lib.ishara_profile_report(self._h, buf, len(buf))
            if n < 0:
                _lib.check(n, "ishara_profile_report")
        finally:
            self._lib.ishara_profile_enable(self._h, 0)
        out = {}
        for line in buf.value.decode().splitlines():
            k, cnt, ms, by, fl = line.split()
            out[k] = dict(launches=int(cnt), ms=float(ms), bytes=float(by), flops=float(fl))
        return out

    # ------------------------------------------------------------------ module probe (debug aid: tests/test_modules_gpu.py)
    def _module_info(self, i: int):
        """(name, in_cols, out_cols, first dropout site, number of sites) of module i."""
        name, a, b, s0, ns = C.c_char_p(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self._lib.ishara_debug_module_info(self._h, i, C.byref(name), C.byref(a), C.byref(b), C.byref(s0), C.byref(ns)),
                   "ishara_debug_module_info")
        return name.value.decode(), a.value, b.value, s0.value, ns.value

    def module_names(self) -> List[str]:
        """The modules of the sequential graph in forward order: stem, Conv1DBlocks, block sub-modules, head."""
        n = int(self._lib.ishara_debug_module_count(self._h))
        if n < 0:
            _lib.check(n, "ishara_debug_module_count")
        return [self._module_info(i)[0] for i in range(n)]

    def module_forward(self, i: int, x, training: bool = False, seed: int = 0, frame_lengths=None) -> torch.Tensor:
        """Module i alone on x [B,T,in_cols] through the model's own orchestration -> f32 [B,T,out_cols] (the head: logits).
        frame_lengths [B]: as in __call__ (modules without a masked operation ignore them)."""
        _, cin, cout, _, _ = self._module_info(i)
        x = torch.as_tensor(x).to(self.device, torch.float32).contiguous()
        if x.dim() != 3 or x.shape[1:] != (self.T, cin):
            raise ValueError(f"module {i}: expected input [B,{self.T},{cin}], got {tuple(x.shape)}")
        fl = self._as_frame_lengths(frame_lengths, x.shape[0])
        y = torch.empty((x.shape[0], self.T, cout), dtype=torch.float32, device=self.device)
        if fl is None:
            _lib.check(self._lib.ishara_debug_module_forward(self._h, i, _lib.ptr(x), x.shape[0], _lib.ptr(y), 1 if training else 0,
                                                             C.c_uint32(seed), _stream()), "ishara_debug_module_forward")
        else:
            _lib.check(self._lib.ishara_debug_module_forward_ex(self._h, i, _lib.ptr(x), x.shape[0], _lib.ptr(y), 1 if training else 0,
                                                                C.c_uint32(seed), _lib.ptr(fl), _stream()), "ishara_debug_module_forward_ex")
        self._last_x = x          # the stem's weight gradient re-reads it
        return y

    def module_backward(self, i: int, dy, labels=None, loss_scale: float = 1.0, frame_lengths=None) -> Optional[torch.Tensor]:
        """Backward of module i after module_forward(i, ..., training=True): dy [B,T,out_cols] -> the gradient with respect to the module's
        input (None for the stem); the parameter gradients are in `grads`.  The head takes its logits as dy and `labels` [B,L]: CTC + head
        backward, the loss in `_loss_buf`.  frame_lengths: the ones module_forward was given (the head takes none)."""
        _, cin, cout, _, _ = self._module_info(i)
        dy = torch.as_tensor(dy).to(self.device, torch.float32).contiguous()
        if dy.dim() != 3 or dy.shape[1:] != (self.T, cout):
            raise ValueError(f"module {i}: expected dy [B,{self.T},{cout}], got {tuple(dy.shape)}")
        B = dy.shape[0]
        if labels is not None:
            yl = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels).to(self.device, torch.int64).contiguous()
            if yl.shape != (B, self._cfg.max_label_len):
                raise ValueError(f"labels must be [B,{self._cfg.max_label_len}] padded with {self.C - 1}")
            dx = torch.empty((B, self.T, cin), dtype=torch.float32, device=self.device)
            _lib.check(self._lib.ishara_debug_head_loss_backward(self._h, _lib.ptr(dy), _lib.ptr(yl), B, _lib.ptr(self._loss_buf), _lib.ptr(self._nll_buf),
                                                                 C.c_float(loss_scale), _lib.ptr(dx), _stream()), "ishara_debug_head_loss_backward")
            return dx
        dx = None if i == 0 else torch.empty((B, self.T, cin), dtype=torch.float32, device=self.device)
        fl = self._as_frame_lengths(frame_lengths, B)
        if fl is None:
            _lib.check(self._lib.ishara_debug_module_backward(self._h, i, _lib.ptr(dy), B, _lib.ptr(dx), _stream()), "ishara_debug_module_backward")
        else:
            _lib.check(self._lib.ishara_debug_module_backward_ex(self._h, i, _lib.ptr(dy), B, _lib.ptr(dx), _lib.ptr(fl), _stream()),
                       "ishara_debug_module_backward_ex")
        return dx

    def ctc_loss(self, y, logits, frame_lengths=None) -> torch.Tensor:
        """CTCLoss(labels, logits) (c6:1-13) on the GPU; returns per-sample nll [B].  frame_lengths [B] (1..T): clip b has that many
        frames (logit_length of tf.nn.ctc_loss); a label that does not fit its clip gives the kernel's sentinel 1e30."""
        logits = logits.to(self.device, torch.float32).contiguous()
        y = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(self.device, torch.int64).contiguous()
        B, T, Cc = logits.shape
        L = y.shape[1]
        ws = torch.empty(int(self._lib.ishara_ctc_workspace_bytes(B, T, L)), dtype=torch.uint8, device=self.device)
        nll = torch.empty(B, dtype=torch.float32, device=self.device)
        if frame_lengths is not None:
            from . import ctc
            fl = ctc._lengths(frame_lengths, B, T, 1, "frame_lengths", self.device)
            _lib.check(self._lib.ishara_ctc_loss_ex(_lib.ptr(logits), _lib.ptr(y), B, T, Cc, L, Cc - 1, _lib.ptr(nll), None, C.c_float(1.0),
                                                    _lib.ptr(ws), _lib.ptr(fl), None, 0, _stream()), "ishara_ctc_loss_ex")
            return nll
        _lib.check(self._lib.ishara_ctc_loss(_lib.ptr(logits), _lib.ptr(y), B, T, Cc, L, Cc - 1, _lib.ptr(nll), None,
                                             C.c_float(1.0), _lib.ptr(ws), _stream()), "ishara_ctc_loss")
        return nll

    def evaluate(self, dataset: Iterable, averaged: bool = False) -> float:
        """Mean CTC loss over a dataset of (x, y) or (x, y, frame_lengths) batches; the lengths mask the model as in __call__, the loss
        keeps logit_length = T like the training loss.  averaged: of the moving average of the weights (inside averaged_weights())."""
        if averaged:
            with self.averaged_weights():
                return self.evaluate(dataset)
        tot, n = 0.0, 0
        for batch in dataset:
            x, y, fl = split_batch(batch)
            logits = self(x, training=False, **_fl_kw(fl))
            tot += float(self.ctc_loss(y, logits).mean().item())
            n += 1
        return tot / max(n, 1)

    # ------------------------------------------------------------------ decode
    def decode_batch(self, logits: torch.Tensor, frame_lengths=None) -> List[np.ndarray]:
        """decode_batch_predictions (c8:15-20) -> list of index arrays (decode_phrase, c8:4-12).  frame_lengths [B] (1..T): clip b is
        decoded as logits[b, :frame_lengths[b]]."""
        idx, ln = self._decode_device(logits, frame_lengths)
        idx, ln = idx.cpu().numpy(), ln.cpu().numpy()
        return [idx[b, :ln[b]].astype(np.int64) for b in range(idx.shape[0])]

    def _decode_device(self, logits: torch.Tensor, frame_lengths=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """decode_batch's decode left on the device: (indices int32 [B, T], lengths int32 [B])."""
        logits = logits.to(self.device, torch.float32).contiguous()
        if frame_lengths is not None:
            from . import ctc
            return ctc.greedy_decode_device(logits, frame_lengths)
        B, T, Cc = logits.shape
        idx = torch.empty((B, T), dtype=torch.int32, device=self.device)
        ln = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self._lib.ishara_greedy_decode(_lib.ptr(logits), B, T, Cc, Cc - 1, _lib.ptr(idx), _lib.ptr(ln), _stream()),
                   "ishara_greedy_decode")
        return idx, ln


    def beam_decode(self, logits, beam_width: int = 16, nbest: int = 1, lm=None, alpha: float = 0.0, beta: float = 0.0,
                    frame_lengths=None) -> List[List[Tuple[np.ndarray, float]]]:
        """CTC prefix beam search (ishara_amd/ctc_beam.py semantics, blank = C - 1) of logits [B, T, C] on the device -> per clip a list
        of (indices int64, score), best first, at most nbest entries.  lm: a [C, C] log-probability table (e.g. CharBigramLM), a CharNGramLM or an
        LMAutomaton (ctc_lm.py: ishara_ctc_beam_decode_lm), or None.
        Unlike decode_batch it uses the last frame too.  The workspace of the latest shape is kept for the next call; the call waits for
        its results, so successive calls never overlap, but calls from several threads at once on one Model would share it (not supported)."""
        from . import ctc_beam
        logits = torch.as_tensor(logits).to(self.device, torch.float32).contiguous()
        if logits.ndim != 3:
            raise ValueError(f"logits must be [B, T, C], got {tuple(logits.shape)}")
        if frame_lengths is not None:                       # clip b is logits[b, :frame_lengths[b]]
            from . import ctc
            return ctc.ctc_beam_decode(logits, frame_lengths, beam_width, nbest, lm, alpha, beta, workspace=getattr(self, "_beam_ws", None))
        B, T, Cc = logits.shape
        ctc_beam.check_device_args(Cc, T, beam_width, nbest)
        lm_dev = ctc_beam.lm_to_device(lm, Cc, self.device)
        nbytes = max(ctc_beam.workspace_bytes(self._lib, B, T, Cc, beam_width), 4)
        ws = getattr(self, "_beam_ws", None)
        if ws is None or ws.numel() < nbytes:
            ws = self._beam_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        idx = torch.empty((B, nbest, T), dtype=torch.int32, device=self.device)
        ln = torch.empty((B, nbest), dtype=torch.int32, device=self.device)
        sc = torch.empty((B, nbest), dtype=torch.float32, device=self.device)
        ctc_beam.launch(self._lib, logits, B, T, Cc, beam_width, nbest, lm_dev, alpha, beta, ws, idx, ln, sc, _stream())
        idx, ln, sc = idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy()
        return [[(idx[b, n, :ln[b, n]].astype(np.int64), float(sc[b, n])) for n in range(nbest) if ln[b, n] >= 0] for b in range(B)]

    def mbr_decode(self, logits, beam_width: int = 16, nbest: int = 8, temperature: float = 1.0, normalise: bool = True, lm=None,
                   alpha: float = 0.0, beta: float = 0.0, frame_lengths=None) -> List[Tuple[np.ndarray, int, float]]:
        """Minimum-Bayes-risk decode (ishara_amd/mbr.py): the beam search's n-best list (beam_decode's arguments), then, on the device,
        the hypothesis with the smallest expected edit distance to the others under the votes exp((score - max) / temperature);
        normalise: the distance to a voter is divided by that voter's length, as the score of c18 divides by the target's.
        -> per clip (indices int64, the selected slot of the n-best, its risk); a clip the selection did not rank (mbr.py: a hypothesis
        longer than 64 symbols) gets the beam's top-1 and a NaN risk."""
        from . import ctc, mbr
        logits = torch.as_tensor(logits).to(self.device, torch.float32).contiguous()
        if logits.ndim != 3:
            raise ValueError(f"logits must be [B, T, C], got {tuple(logits.shape)}")
        it = mbr.inverse_temperature(temperature)
        mbr.check_device_args(nbest, logits.shape[1], logits.shape[2], 1 if normalise else 0)
        hyp = ctc.ctc_beam_nbest_device(logits, frame_lengths, beam_width, nbest, lm, alpha, beta)
        idx, ln, best, det = mbr.mbr_select(*hyp, inv_temp=it, mode=1 if normalise else 0, C=logits.shape[2], return_details=True)
        idx, ln, best, risk = idx.cpu().numpy(), ln.cpu().numpy(), best.cpu().numpy(), det["risk"].cpu().numpy()
        return [(idx[b, :ln[b]].astype(np.int64), int(best[b]), float(risk[b, best[b]]) if best[b] >= 0 else float("nan"))
                for b in range(idx.shape[0])]

    def rescore_decode(self, logits, beam_width: int = 16, nbest: int = 8, lm=None, alpha: float = 0.0, beta: float = 0.0, search_lm=None,
                       frame_lengths=None, mbr: bool = False, temperature: float = 1.0) -> List[Tuple[np.ndarray, float, float]]:
        """Two-pass decode (ishara_amd/rescore.py): the beam search with `search_lm` (or no LM; its alpha / beta are this call's), then, on
        the device, the exact CTC log-likelihood of every hypothesis of the n-best and the rescoring logp + alpha * lm + beta * len with
        `lm` (a CharNGramLM, an LMAutomaton or a [C, C] table).  -> per clip (indices int64, score, posterior): the top hypothesis of the
        rescored list, or with mbr=True the minimum-Bayes-risk choice voted with the posterior.  A clip without a hypothesis gives
        (empty, -inf, 0)."""
        from . import ctc, rescore
        from . import mbr as mbr_mod
        logits = torch.as_tensor(logits).to(self.device, torch.float32).contiguous()
        if logits.ndim != 3:
            raise ValueError(f"logits must be [B, T, C], got {tuple(logits.shape)}")
        mbr_mod.inverse_temperature(temperature)
        lm = rescore.lm_to_device(lm, self.device)
        if lm is not None and int(lm.logp.shape[1]) != logits.shape[2]:
            raise ValueError(f"the lm has {int(lm.logp.shape[1])} classes, the logits {logits.shape[2]}")
        idx, ln, _ = ctc.ctc_beam_nbest_device(logits, frame_lengths, beam_width, nbest, search_lm, alpha if search_lm is not None else 0.0, beta)
        logp = rescore.ctc_score_nbest(logits, idx, ln, frame_lengths)
        idx, ln, sc, det = rescore.rescore_nbest(idx, ln, logp, None, lm, alpha, beta, temperature, return_details=True)
        post = det["posterior"]
        if mbr:
            best = mbr_mod.mbr_select(idx, ln, weights=post, mode=1, C=logits.shape[2])[2]
        else:
            best = torch.zeros(idx.shape[0], dtype=torch.int32, device=idx.device)
        idx, ln, sc, post, best = idx.cpu().numpy(), ln.cpu().numpy(), sc.cpu().numpy(), post.cpu().numpy(), best.cpu().numpy()
        out = []
        for b in range(idx.shape[0]):
            k = int(best[b])
            if k < 0 or ln[b, k] < 0:
                out.append((np.zeros(0, np.int64), float("-inf"), 0.0))
            else:
                out.append((idx[b, k, :ln[b, k]].astype(np.int64), float(sc[b, k]), float(post[b, k])))
        return out

    def align(self, logits, y, frame_lengths=None) -> list:
        """CTC forced alignment (ishara_amd/ctc_align.py semantics, blank = C - 1) of logits [B, T, C] to the labels y [B, L] (padded with
        C - 1) on the device -> per clip an Alignment: the label index every frame emits, the log-probability of the best path and one
        (symbol, start, end, conf) span per symbol.  The workspace is kept for the next call, as beam_decode keeps its own."""
        from . import ctc_align
        logits = torch.as_tensor(logits).to(self.device, torch.float32).contiguous()
        if frame_lengths is not None:                       # clip b is logits[b, :frame_lengths[b]]; frame_pos is -1 past it
            from . import ctc
            return ctc.ctc_align(logits, y, frame_lengths, workspace=getattr(self, "_align_ws", None))
        y = torch.as_tensor(np.asarray(y) if not isinstance(y, torch.Tensor) else y).to(self.device, torch.int64).contiguous()
        if logits.ndim != 3 or y.ndim != 2 or y.shape[0] != logits.shape[0]:
            raise ValueError(f"logits must be [B, T, C] and y [B, L], got {tuple(logits.shape)} and {tuple(y.shape)}")
        B, T, Cc = logits.shape
        L = y.shape[1]
        ctc_align.check_device_args(Cc, T, L, Cc - 1)
        nbytes = max(ctc_align.workspace_bytes(self._lib, B, T, L), 16)
        ws = getattr(self, "_align_ws", None)
        if ws is None or ws.numel() < nbytes:
            ws = self._align_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        fp = torch.empty((B, T), dtype=torch.int32, device=self.device)
        st = torch.empty((B, L), dtype=torch.int32, device=self.device)
        en = torch.empty((B, L), dtype=torch.int32, device=self.device)
        cf = torch.empty((B, L), dtype=torch.float32, device=self.device)
        sc = torch.empty(B, dtype=torch.float32, device=self.device)
        ctc_align.launch(self._lib, logits, y, B, T, Cc, L, Cc - 1, ws, fp, st, en, cf, sc, _stream())
        return ctc_align.to_alignments(y.cpu().numpy(), *(t.cpu().numpy() for t in (fp, st, en, cf, sc)))


def _fl_kw(frame_lengths):
    """the frame_lengths keyword of a call, only when there are lengths: without them train_on_batch calls loss_and_gradients exactly as it
    did before lengths existed (a wrapper or subclass with the older signature keeps working)"""
    return {} if frame_lengths is None else {"frame_lengths": frame_lengths}


def split_batch(batch):
    """(x, y) or (x, y, frame_lengths) of a dataset -> (x, y, frame_lengths or None)"""
    if len(batch) == 3:
        return batch[0], batch[1], batch[2]
    x, y = batch
    return x, y, None


def frame_lengths(x) -> torch.Tensor:
    """Per-clip frame counts of a zero-padded batch x [B,T,F] (float32, on the GPU) -> int32 [B] on the same device: 1 + the index of the
    last frame with any non-zero feature, 0 for an all-zero clip.  The prefix reading of Keras's Masking(0.0): an all-zero frame inside a
    clip stays valid.  No host synchronise."""
    x = torch.as_tensor(x)
    if x.ndim != 3 or x.dtype != torch.float32:
        raise ValueError(f"frame_lengths: x must be float32 [B,T,F], got {tuple(x.shape)} {x.dtype}")
    if not x.is_cuda:
        raise _lib.IsharaError("frame_lengths: x must be on the GPU: the kernel has no CPU path")
    x = x.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().ishara_frame_lengths(_lib.ptr(x), x.shape[0], x.shape[1], x.shape[2], _lib.ptr(out), _stream()), "ishara_frame_lengths")
    return out


def make_config(dim=256, num_conv_squeeze_blocks=2, num_conv_conform_blocks=2, kernel_sizes=(11, 5, 3),
                num_conv_per_block=3, dropout_rate=0.2, num_heads=8, expansion_factor=2, transformer_kernel_size=15,
                input_shape=(176, 276), num_classes=60, top_dim=0, squeeze_expansion=0, conformer_expansion=0,
                head_dropout=0.4, conformer_attn_dropout=0.1, dtype="bf16", max_batch=64, max_label_len=64,
                attn_impl=1) -> _lib.Config:
    c = _lib.Config()
    c.dim, c.num_conv_squeeze_blocks, c.num_conv_conform_blocks = dim, num_conv_squeeze_blocks, num_conv_conform_blocks
    ks = list(kernel_sizes)
    c.num_kernel_sizes = len(ks)
    for i, k in enumerate(ks[:8]):
        c.kernel_sizes[i] = k
    c.num_conv_per_block, c.dropout_rate, c.num_heads = num_conv_per_block, dropout_rate, num_heads
    c.expansion_factor, c.transformer_kernel_size = expansion_factor, transformer_kernel_size
    c.frames, c.features, c.num_classes = input_shape[0], input_shape[1], num_classes
    c.top_dim, c.squeeze_expansion, c.conformer_expansion = top_dim, squeeze_expansion, conformer_expansion
    c.head_dropout, c.conformer_attn_dropout = head_dropout, conformer_attn_dropout
    c.dtype = {"f32": _lib.F32, "fp32": _lib.F32, "float32": _lib.F32, "bf16": _lib.BF16, "bfloat16": _lib.BF16,
               "f16": _lib.F16, "fp16": _lib.F16, "float16": _lib.F16}[dtype]
    c.max_batch, c.max_label_len, c.attn_impl = max_batch, max_label_len, attn_impl
    return c


def get_model(dim=256, num_conv_squeeze_blocks=2, num_conv_conform_blocks=2, kernel_sizes=[11, 5, 3],
              num_conv_per_block=3, dropout_rate=0.2, num_heads=8, expansion_factor=2, transformer_kernel_size=15,
              *, input_shape=(176, 276), num_classes=60, dtype="bf16", max_batch=64, device="cuda:0", seed=0, **variant):
    """get_model(...) of conv-hybrid-model.ipynb c7:1-72.  The positional/keyword arguments are
    the reference's; the keyword-only ones replace the notebook globals (INPUT_SHAPE c3:119,
    len(char_to_num) c1:7) and pick the build's storage dtype / workspace size."""
    cfg = make_config(dim, num_conv_squeeze_blocks, num_conv_conform_blocks, kernel_sizes, num_conv_per_block, dropout_rate,
                      num_heads, expansion_factor, transformer_kernel_size, input_shape, num_classes, dtype=dtype,
                      max_batch=max_batch, **variant)
    model = Model(cfg, device=device, seed=seed)
    model.compile(loss="ctc", optimizer=Optimizer())
    return model
