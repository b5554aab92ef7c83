"""Host-side mirror of the reference's torch Conformer stack — `conformer/conformer.py:76-87` (`ConformerEncoder`) and the
modules it stacks (`:6-73`) — on the HIP library (csrc/conformer_r5.hip, family ISHARA_FAMILY_TORCH_CONFORMER).

`ConformerEncoder(dim, num_layers=7, num_heads=8, expansion_factor=4, kernel_size=31, dropout=0.1)` has the reference's
constructor; `enc(x)` / `enc.train()` / `enc.eval()` / `state_dict()` / `load_state_dict()` behave like the torch module's:
state-dict keys and array layouts are the reference's (`layers.0.ffn1.linear1.weight` `[out,in]`, `in_proj_weight` `[3d,d]`
q|k|v block-major, `depthwise_conv.weight` `[d,1,k]`, `batch_norm.running_mean`, ...).  `enc(x)` is differentiable through
`torch.autograd`: `y = enc(x); loss(y).backward()` fills `x.grad` and `enc.flat.grad` (the flat trainable-parameter vector
any `torch.optim` optimiser can step); `enc.grad_state_dict()` gives the parameter gradients keyed and laid out like
`state_dict()`.

All arithmetic runs in libishara_hip.so; torch tensors are containers.  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from ._handle import Handle
from ._lib import IsharaError, stream as _stream


def head_major_perm(dim: int, heads: int) -> np.ndarray:
    """Column order of the library's packed qkv projection (h*3dh + {q,k,v}*dh + i) in terms of nn.MultiheadAttention's
    in_proj rows ({q,k,v}*d + h*dh + i): `W_lib[:, j] = in_proj_weight[perm[j], :]`."""
    dh = dim // heads
    return np.array([part * dim + h * dh + i for h in range(heads) for part in range(3) for i in range(dh)], dtype=np.int64)


class _LayoutMap:
    """torch state_dict array <-> the array stored in the library's flat buffer, per entry name."""

    def __init__(self, dim: int, heads: int):
        self.perm = head_major_perm(dim, heads)
        self.inv = np.argsort(self.perm)

    def to_lib(self, name: str, a: np.ndarray) -> np.ndarray:
        if name.endswith("in_proj_weight"): return np.ascontiguousarray(a[self.perm].T)            # [3d,d] -> [d,3d] head-major columns
        if name.endswith("in_proj_bias"): return np.ascontiguousarray(a[self.perm])
        if name.endswith("depthwise_conv.weight"): return np.ascontiguousarray(a[:, 0, :].T)        # [d,1,k] -> [k,d]
        if name.endswith("pointwise_conv1.weight") or name.endswith("pointwise_conv2.weight"): return np.ascontiguousarray(a[:, :, 0].T)
        if a.ndim == 2: return np.ascontiguousarray(a.T)                                            # Linear [out,in] -> [in,out]
        return a

    def to_torch(self, name: str, a: np.ndarray) -> np.ndarray:
        if name.endswith("in_proj_weight"): return np.ascontiguousarray(a.T[self.inv])
        if name.endswith("in_proj_bias"): return np.ascontiguousarray(a[self.inv])
        if name.endswith("depthwise_conv.weight"): return np.ascontiguousarray(a.T[:, None, :])
        if name.endswith("pointwise_conv1.weight") or name.endswith("pointwise_conv2.weight"): return np.ascontiguousarray(a.T[:, :, None])
        if a.ndim == 2: return np.ascontiguousarray(a.T)
        return a


def default_state_dict(shapes: "OrderedDict[str, tuple]", seed: int) -> "OrderedDict[str, np.ndarray]":
    """Default initialisers of the torch layers the reference stacks: nn.Linear / nn.Conv1d draw weight and bias from
    U(+-1/sqrt(fan_in)); nn.MultiheadAttention uses xavier_uniform for in_proj_weight and zero in_proj / out_proj biases;
    norms start at (1, 0), running statistics at (0, 1).  Same distributions as torch's, not the same draws."""
    g = torch.Generator().manual_seed(seed)
    sd: "OrderedDict[str, np.ndarray]" = OrderedDict()

    def uniform(shape, lim):
        return ((torch.rand(tuple(shape), generator=g) * 2 - 1) * lim).numpy().astype(np.float32)

    for name, shape in shapes.items():
        leaf = name.rsplit(".", 1)[-1]
        if "layer_norm" in name or "batch_norm" in name:
            sd[name] = (np.ones if leaf in ("weight", "running_var") else np.zeros)(shape, np.float32)
        elif name.endswith("in_proj_weight"):
            sd[name] = uniform(shape, (6.0 / (shape[0] + shape[1])) ** 0.5)
        elif name.endswith("in_proj_bias") or name.endswith("out_proj.bias"):
            sd[name] = np.zeros(shape, np.float32)
        elif leaf == "weight":
            sd[name] = uniform(shape, float(np.prod(shape[1:])) ** -0.5)
        else:                                       # bias of a Linear / Conv1d: the fan_in of its weight
            sd[name] = uniform(shape, float(np.prod(sd[name[:-4] + "weight"].shape[1:])) ** -0.5)
    return sd


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flat, enc, attn_bias=None, key_len=None, input_len=None):
        ctx.enc = enc
        ctx.attn_bias, ctx.key_len = attn_bias, key_len      # the caller's mask arrays: the library keeps no pointer, backward() passes them again
        ctx.mask_versions = tuple(None if t is None else t._version for t in (attn_bias, key_len))      # (they never require grad: not save_for_backward's business)
        ctx.input_len, ctx.input_len_version = input_len, None if input_len is None else input_len._version      # the Squeezeformer family's padding mask
        y = enc._forward(x, training=enc.training, attn_bias=attn_bias, key_len=key_len, input_len=input_len)
        ctx.gen = enc._gen                # the library keeps the saved activations of its LAST training forward only
        return y

    @staticmethod
    def backward(ctx, dy):
        enc = ctx.enc
        if ctx.gen != enc._gen:
            raise IsharaError("backward() of an encoder output whose saved activations were overwritten by a later forward pass of the same "
                              "encoder: one live autograd graph per encoder (call backward() before the next forward, or use a second encoder "
                              "object for a second branch)")
        if ctx.mask_versions != tuple(None if t is None else t._version for t in (ctx.attn_bias, ctx.key_len)):
            raise IsharaError("attn_mask / key_lengths were modified in place between the forward pass and backward(): the gradient would belong to "
                              "another mask than the output")
        if ctx.input_len is not None and ctx.input_len_version != ctx.input_len._version:
            raise IsharaError("input_lengths were modified in place between the forward pass and backward(): the gradient would belong to "
                              "another mask than the output")
        dx = enc._backward(dy, attn_bias=ctx.attn_bias, key_len=ctx.key_len, input_len=ctx.input_len)
        return dx, enc.grads[:enc.n_train].clone(), None, None, None, None


class _TorchFamilyEncoder(Handle):
    """Shared host side of the two torch encoder families: one library handle, flat parameter / gradient buffers, state_dict in
    the reference's keys and layouts, torch.autograd integration.  Subclasses fill an `_lib.Config` and a layout map."""

    def _create(self, cfg, layout_map, in_features, seq_len, max_batch, device, seed):
        self._create_handle(cfg)
        self.T, self.F_in = seq_len, in_features
        self._map = layout_map
        self.T_out = int(self._lib.ishara_encoder_output_frames(self._h))
        self.training = True
        self._seed, self._steps = seed * 7919 + 17, 0
        self._gen = 0                     # forward passes so far (autograd graphs check it: the library saves ONE pass)
        self._synced_version = -1         # `flat._version` at the last ishara_sync_weights
        if device is not None:
            self._to_device(device, seed)

    # ------------------------------------------------------------------ device state
    def _to_device(self, device, seed):
        self._bind_device(device)
        # the flat trainable vector as a leaf torch optimisers can step; it aliases the library's parameter buffer
        self.flat = torch.nn.Parameter(self.params[:self.n_train], requires_grad=True)
        self.load_state_dict(self._default_state(seed))

    # ------------------------------------------------------------------ nn.Module surface
    def train(self, mode: bool = True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def parameters(self):
        return [self.flat]

    def zero_grad(self):
        self.flat.grad = None

    def torch_shapes(self) -> "OrderedDict[str, tuple]":
        """state_dict key -> shape in the reference's layout, in state_dict order."""
        out = OrderedDict()
        for n, s, _, _ in self.entries:
            out[n] = tuple(self._map.to_torch(n, np.empty(s, np.float32)).shape)
        return out

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        flat = self.params.detach().cpu().numpy()
        return OrderedDict((n, torch.from_numpy(self._map.to_torch(n, flat[o:o + int(np.prod(s))].reshape(s).copy()))) for n, s, o, _ in self.entries)

    def grad_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Parameter gradients of the last backward pass, keyed and laid out like state_dict()."""
        flat = self.grads.detach().cpu().numpy()
        return OrderedDict((n, torch.from_numpy(self._map.to_torch(n, flat[o:o + int(np.prod(s))].reshape(s).copy())))
                           for n, s, o, t in self.entries if t)

    def load_state_dict(self, sd: Dict[str, "torch.Tensor"], strict: bool = True):
        names = {n for n, _, _, _ in self.entries}
        extra = [k for k in sd if k not in names and not k.endswith("num_batches_tracked")]
        missing = [n for n in names if n not in sd]
        if strict and (extra or missing):
            raise KeyError(f"load_state_dict: missing {sorted(missing)[:4]}, unexpected {sorted(extra)[:4]}")
        flat = self.params.detach().cpu().numpy().copy()
        for n, s, o, _ in self.entries:
            if n not in sd:
                continue
            a = np.asarray(sd[n].detach().cpu().numpy() if isinstance(sd[n], torch.Tensor) else sd[n], np.float32)
            a = self._map.to_lib(n, a)
            if tuple(a.shape) != tuple(s):
                raise ValueError(f"{n}: expected {self.torch_shapes()[n]}, got an array that maps to {a.shape} (library shape {s})")
            flat[o:o + a.size] = a.reshape(-1)
        with torch.no_grad():
            self.params.copy_(torch.from_numpy(flat))
        self.sync_weights()

    def sync_weights(self):
        """Re-derive the MFMA-typed weight copies after the flat parameters changed (an optimiser step on `enc.flat`).  `_forward`
        calls it by itself whenever torch's version counter of the flat buffer moved since the last call (in-place optimiser steps,
        `load_state_dict` bump it); writes that bypass the counter (`enc.flat.data...`, a raw pointer) need the explicit call."""
        _lib.check(self._lib.ishara_sync_weights(self._h, _stream()), "ishara_sync_weights")
        self._synced_version = self.flat._version

    # ------------------------------------------------------------------ forward / backward
    def _forward(self, x: torch.Tensor, training: bool, seed: Optional[int] = None, attn_bias=None, key_len=None, input_len=None) -> torch.Tensor:
        if x.dim() == 2:
            x = x[None]
        if x.shape[1:] != (self.T, self.F_in):
            raise ValueError(f"expected input [B,{self.T},{self.F_in}], got {tuple(x.shape)}")
        x = x.detach().to(self.device, torch.float32).contiguous()
        B = x.shape[0]
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch {self.max_batch}")
        y = torch.empty((B, self.T_out, self.dim), dtype=torch.float32, device=self.device)
        if self.flat._version != self._synced_version:      # the parameters moved (optimiser step): refresh the MFMA-typed copies first
            self.sync_weights()
        self._gen += 1
        if seed is None:
            seed = (self._seed + 0x9E3779B1 * self._steps) & 0xFFFFFFFF
            self._steps += 1
        if input_len is not None:      # SqueezeformerEncoder(mask_padding=True): input frames per clip
            if tuple(input_len.shape) != (B,):
                raise ValueError(f"input_lengths: expected [{B}] (one per clip of the batch), got {tuple(input_len.shape)}")
            _lib.check(self._lib.ishara_encoder_forward_lengths(self._h, _lib.ptr(x), B, _lib.ptr(y), 1 if training else 0, C.c_uint32(seed), _lib.ptr(input_len),
                                                                _stream()), "ishara_encoder_forward_lengths")
        elif attn_bias is None and key_len is None:
            _lib.check(self._lib.ishara_encoder_forward(self._h, _lib.ptr(x), B, _lib.ptr(y), 1 if training else 0, C.c_uint32(seed), _stream()),
                       "ishara_encoder_forward")
        else:
            if key_len is not None and tuple(key_len.shape) != (B,):
                raise ValueError(f"key_lengths: expected [{B}] (one per clip of the batch), got {tuple(key_len.shape)}")
            _lib.check(self._lib.ishara_encoder_forward_ex(self._h, _lib.ptr(x), B, _lib.ptr(y), 1 if training else 0, C.c_uint32(seed), _lib.ptr(attn_bias),
                                                           _lib.ptr(key_len), _stream()), "ishara_encoder_forward_ex")
        self._last_x = x
        return y

    def _backward(self, dy: torch.Tensor, attn_bias=None, key_len=None, input_len=None) -> torch.Tensor:
        dy = dy.detach().to(self.device, torch.float32).contiguous()
        dx = torch.empty((dy.shape[0], self.T, self.F_in), dtype=torch.float32, device=self.device)
        if input_len is not None:
            _lib.check(self._lib.ishara_encoder_backward_lengths(self._h, _lib.ptr(dy), dy.shape[0], _lib.ptr(dx), _lib.ptr(input_len), _stream()),
                       "ishara_encoder_backward_lengths")
        elif attn_bias is None and key_len is None:
            _lib.check(self._lib.ishara_encoder_backward(self._h, _lib.ptr(dy), dy.shape[0], _lib.ptr(dx), _stream()), "ishara_encoder_backward")
        else:
            _lib.check(self._lib.ishara_encoder_backward_ex(self._h, _lib.ptr(dy), dy.shape[0], _lib.ptr(dx), _lib.ptr(attn_bias), _lib.ptr(key_len), _stream()),
                       "ishara_encoder_backward_ex")
        return dx

    def _default_state(self, seed):
        return default_state_dict(self.torch_shapes(), seed)

    def _apply(self, x, attn_bias=None, key_len=None, input_len=None):
        """Training mode with grad enabled: differentiable through `_EncoderFn` — ONE live graph per encoder (the library keeps the
        saved activations and the dropout seed of its last training forward; a stale graph's backward raises).  Eval mode returns a
        constant (inference path, nothing saved): asking for a gradient w.r.t. the input there is an error, not a silent zero."""
        x = torch.as_tensor(x)
        if torch.is_grad_enabled() and self.training:
            return _EncoderFn.apply(x.to(self.device), self.flat, self, attn_bias, key_len, input_len)
        if torch.is_grad_enabled() and x.requires_grad:
            raise IsharaError("eval-mode forward is not differentiable (no activations are saved): call enc.train() for gradients, or "
                              "pass x.detach() / use torch.no_grad() for inference")
        return self._forward(x, training=self.training, attn_bias=attn_bias, key_len=key_len, input_len=input_len)


class ConformerEncoder(_TorchFamilyEncoder):
    """conformer/conformer.py:76-87 on MI355X.  Extra keyword arguments size the device buffers: `seq_len` (frames per clip,
    a multiple of 8, <= 512), `max_batch`, `dtype` ("bf16" storage + bf16 MFMA with fp32 accumulation, or "f32")."""

    def __init__(self, dim, num_layers=7, num_heads=8, expansion_factor=4, kernel_size=31, dropout=0.1, *,
                 seq_len=384, max_batch=64, dtype="bf16", device: Optional[str] = "cuda:0", seed=0):
        if kernel_size % 2 == 0:
            raise ValueError("kernel_size must be odd (padding=kernel_size//2 keeps the sequence length only then)")
        cfg = _lib.Config()
        cfg.family = _lib.FAMILY_TORCH_CONFORMER
        cfg.dim, cfg.num_conv_conform_blocks, cfg.num_heads = dim, num_layers, num_heads
        cfg.expansion_factor, cfg.transformer_kernel_size, cfg.dropout_rate = expansion_factor, kernel_size, dropout
        cfg.frames, cfg.features, cfg.num_classes = seq_len, dim, 60
        cfg.dtype = {"f32": _lib.F32, "bf16": _lib.BF16}[dtype]
        cfg.max_batch, cfg.max_label_len, cfg.attn_impl = max_batch, 64, 1
        self.dim, self.num_layers, self.num_heads = dim, num_layers, num_heads
        self._create(cfg, _LayoutMap(dim, num_heads), dim, seq_len, max_batch, device, seed)

    def __call__(self, x, attn_mask=None, *, key_lengths=None):
        """ConformerEncoder.forward(x, attn_mask=None) — conformer.py:84-87, which hands `attn_mask` to nn.MultiheadAttention (:30-33)
        and to nothing else.  So only the attention is masked here too: the convolution module and BatchNorm1d keep seeing the padded
        frames of a clip as they do without a mask.

        `attn_mask`: `(T, T)`, row = query, column = key, torch tensor or array, shared by every clip and head.  `bool`: True = not
        allowed.  Floating: added to the scaled score, softmax(scale * q.k^T + attn_mask), not scaled itself; entries finite or -inf.
        It is turned into the fp32 additive table on the device (no host synchronise) and has no gradient: a mask that
        `requires_grad` is an error.  A 3-D mask raises NotImplementedError: per-clip padding is what `key_lengths` is for.
        `key_lengths`: `[B]` integers; the keys j >= key_lengths[b] of clip b are masked for every query and head (the 3-D mask a
        torch user builds for padding).  A device tensor is used where it is; values are clamped to [0, T] on the device.
        Both work together, in eval and in training mode (dropout acts on the masked probabilities).

        A query row whose keys are all masked gives an all-zero attention output and takes no part in the backward pass.  This differs
        from the reference, whose own call (`need_weights=True`) returns NaN for such a row; zeros are this library's convention.
        `attn_mask=None, key_lengths=None` is the unmasked path, unchanged."""
        return self._apply(x, self._attn_bias(attn_mask), self._key_len(key_lengths))

    def _attn_bias(self, attn_mask):
        """the fp32 additive table [T, T] on the device (None for None); every check is made on the argument as given, before any device work"""
        if attn_mask is None:
            return None
        m = torch.as_tensor(attn_mask)
        if m.requires_grad:
            raise ValueError("attn_mask has no gradient here: pass attn_mask.detach() (a mask that requires_grad is refused, not silently detached)")
        if m.dim() == 3:
            raise NotImplementedError("a 3-D attn_mask is not supported: a per-clip padding mask is passed as key_lengths=[B] (keys >= key_lengths[b] are "
                                      "masked for clip b); a (T, T) attn_mask is shared by every clip and head")
        if tuple(m.shape) != (self.T, self.T):
            raise ValueError(f"attn_mask: expected ({self.T}, {self.T}) (query, key), got {tuple(m.shape)}")
        if m.dtype == torch.bool:
            m = m.to(self.device)
            return torch.zeros((self.T, self.T), dtype=torch.float32, device=self.device).masked_fill_(m, float("-inf"))
        if not m.is_floating_point():
            raise TypeError(f"attn_mask: bool (True = not allowed) or floating (added to the score), got {m.dtype}")
        m = m.to(self.device, torch.float32).contiguous()
        return m if m.data_ptr() % 16 == 0 else m.clone()

    def _key_len(self, key_lengths):
        """int32 [B] on the device (None for None); a device int32 tensor is used where it is"""
        if key_lengths is None:
            return None
        k = torch.as_tensor(key_lengths)
        if k.dim() != 1 or k.dtype == torch.bool or k.is_floating_point() or k.is_complex():
            raise ValueError(f"key_lengths: expected [B] integers, got shape {tuple(k.shape)} of {k.dtype}")
        return k.to(self.device, torch.int32).contiguous()

    forward = __call__
