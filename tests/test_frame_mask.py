"""Per-clip frame lengths of the Keras hybrid family, on the CPU: the fp64 restatement (tests/frame_mask_parity.py) against a direct
transcription of Keras's masked formulas, against the oracle's unmasked modules at lengths all T, and the refusals that need no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import frame_mask_parity as FM
import module_parity as MP
from ishara_amd import Model, _lib, make_config
from oracle import ishara_oracle as O

FAKE = C.c_void_p(0x1000)
KW = dict(dim=32, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, num_heads=4, kernel_sizes=(5, 3), num_conv_per_block=2, input_shape=(24, 12))
LENS = (24, 13, 1, 7)


def _cfg(dropout=0.2):
    return O.Config(dropout_rate=dropout, head_dropout=0.4 if dropout else 0.0, conformer_attn_dropout=0.1 if dropout else 0.0, **KW)


def _params(cfg, seed=0):
    g = np.random.default_rng(5)
    W = O.init_params(cfg, seed)
    for n in W:          # non-trivial gains, biases and ECA taps
        if n.rsplit("/", 1)[-1] in ("gamma", "beta", "bias"):
            W[n] = (W[n] + 0.2 * g.standard_normal(W[n].shape)).astype(np.float32)
    return O.to_torch(W, torch.float64, requires_grad=False)


# ------------------------------------------------------------------ Keras's formulas, transcribed
def keras_gap(x, m):
    """GlobalAveragePooling1D.call(inputs, mask): mask cast and expanded, inputs *= mask, sum over steps / sum of the mask"""
    m = m[:, :, None]
    return (x * m).sum(dim=1) / m.sum(dim=1)


def keras_softmax(scores, m):
    """Softmax.call(inputs, mask): adder = (1 - mask) * -1e9, inputs += adder, softmax over the last axis"""
    return torch.softmax(scores + (1.0 - m) * -1e9, dim=-1)


def test_masked_mean_is_keras_gap():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 24, 40, dtype=torch.float64, generator=g)
    m = FM.frame_mask(LENS, 24)
    assert float((FM.masked_mean(x, LENS) - keras_gap(x, m)).abs().max()) <= 1e-12
    assert float((FM.eca_masked(x, torch.tensor([0.3, -0.2, 0.5, 0.1, -0.4], dtype=torch.float64), LENS)
                  - x * torch.sigmoid(torch.nn.functional.conv1d(keras_gap(x, m).unsqueeze(1), torch.tensor([[[0.3, -0.2, 0.5, 0.1, -0.4]]], dtype=torch.float64),
                                                                   padding=2).squeeze(1))[:, None, :]).abs().max()) <= 1e-12


def test_excluded_keys_are_keras_masked_softmax():
    cfg = _cfg(0.0)
    P = _params(cfg)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(4, 24, 32, dtype=torch.float64, generator=g)
    name = "squeezeformer_0/mha"
    got = FM.mhsa(x, P, name, cfg, 0.0, O._Sites(1, False), LENS)
    B, T, d = x.shape
    H, dh = cfg.num_heads, d // cfg.num_heads
    qkv = O.dense(x, P, f"{name}/qkv", bias=False).view(B, T, H, 3 * dh).permute(0, 2, 1, 3)          # c5:101-104
    q, k, v = qkv[..., :dh], qkv[..., dh:2 * dh], qkv[..., 2 * dh:]
    attn = keras_softmax((q @ k.transpose(-1, -2)) * (d ** -0.5), FM.frame_mask(LENS, T)[:, None, None, :])   # c5:106-112: mask = mask[:, None, None, :]
    ref = O.dense((attn @ v).permute(0, 2, 1, 3).reshape(B, T, d), P, f"{name}/proj", bias=False)
    assert float((got - ref).abs().max()) <= 1e-12


def test_a_clip_without_frames_gives_zeros_not_nan():
    cfg = _cfg(0.0)
    P = _params(cfg)
    x = torch.randn(2, 24, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_(True)
    y = FM.mhsa(x, P, "squeezeformer_0/mha", cfg, 0.0, O._Sites(1, False), (0, 24))
    assert float(y[0].detach().abs().max()) == 0.0 and bool(torch.isfinite(y).all())
    y.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad[0].abs().max()) == 0.0
    assert float(FM.masked_mean(x.detach(), (0, 5))[0].abs().max()) == 0.0


@pytest.mark.parametrize("name", ["convsqueeze_0_1", "convsqueeze_0_2", "squeezeformer_0/mha", "squeezeformer_0/conv", "conformer_0/mha"])
def test_lengths_all_T_restate_the_oracle(name):
    """with every length equal to T the restatement is the oracle's unmasked module (training, dropout on), y and dx"""
    cfg = _cfg(0.2)
    P = _params(cfg)
    first = {n: f for n, f, _ in MP.walk_sites(cfg)}[name]
    x0 = torch.randn(3, 24, 32, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    out = []
    for masked in (True, False):
        x = x0.clone().requires_grad_(True)
        sites, ns = O._Sites(9, True, first=first), {}
        if masked:
            y = FM.module_forward(name, x, P, cfg, sites, ns, (24, 24, 24))
        elif MP.module_kind(name) == "conv":
            y = O.conv1d_block(x, P, name, cfg, True, sites, ns)
        else:
            blk, sub = name.split("/")
            y = {"squeezeformer_0/mha": O.sqz_mha, "squeezeformer_0/conv": O.sqz_conv, "conformer_0/mha": O.conf_mha}[name](x, P, blk, cfg, sites)
        y.square().sum().backward()
        out.append((y.detach(), x.grad, ns))
    assert float((out[0][0] - out[1][0]).abs().max()) <= 1e-12 and float((out[0][1] - out[1][1]).abs().max()) <= 1e-12 * float(out[1][1].abs().max() + 1)
    for k in out[1][2]:
        assert float((out[0][2][k] - out[1][2][k]).abs().max()) <= 1e-12


def test_whole_model_restatement_at_all_T_is_the_oracle():
    cfg = _cfg(0.2)
    W = O.init_params(cfg, 0)
    x, y = O.synthetic_batch(cfg, 3, seed=1)
    a = FM.loss_and_grads(W, x, y, cfg, (24, 24, 24), seed=7)
    b = O.loss_and_grads(W, x, y, cfg, training=True, seed=7, dtype=torch.float64)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(b[0]) and np.abs(a[1] - b[1]).max() <= 1e-11
    c = FM.loss_and_grads(W, x, y, cfg, (24, 11, 5), seed=7)
    assert np.abs(c[1] - b[1]).max() > 1e-3          # and real lengths change the logits


def test_frame_lengths_restatement():
    x = np.zeros((4, 8, 3), np.float32)
    x[1, 7, 2] = 1.0; x[2, 0, 0] = -1.0; x[2, 4, 1] = 2.0; x[3, 2, 0] = np.nan
    assert FM.frame_lengths_np(x).tolist() == [0, 8, 5, 3]


# ------------------------------------------------------------------ refusals that need no GPU
@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _refused(lib, rc, *words):
    assert rc != 0
    msg = lib.ishara_last_error().decode()
    for w in words:
        assert w in msg, f"{msg!r} does not say {w!r}"


def test_frame_lengths_of_the_wrong_shape_or_type_are_refused():
    m = Model(make_config(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 36), max_batch=2), device=None)
    x = torch.zeros(2, 48, 36)
    for bad in ([48, 20, 3], [[48, 20]], torch.tensor([48.0, 20.0]), torch.tensor([True, False]), 5):
        with pytest.raises(ValueError, match="frame_lengths"):
            m(x, frame_lengths=bad)
        with pytest.raises(ValueError, match="frame_lengths"):
            m.loss_and_gradients(x, np.full((2, 64), 59), frame_lengths=bad)
    for good in ([48, 20], np.array([48, 0]), torch.tensor([100, -3], dtype=torch.int64)):      # well-formed: converted, values untouched (the kernels clamp)
        t = m._as_frame_lengths(good, 2)
        assert t.dtype == torch.int32 and t.is_contiguous() and t.tolist() == [int(v) for v in good]
    assert m._as_frame_lengths(None, 2) is None


def test_other_families_f16_and_misaligned_lengths_are_refused(lib):
    from ishara_amd.squeezeformer import SqueezeformerEncoder
    from ishara_amd import ConformerEncoder
    sq = SqueezeformerEncoder(16, 32, 2, 0, 1, 2, seq_len=64, max_batch=2, device=None)
    enc = ConformerEncoder(32, 1, 4, seq_len=48, max_batch=2, dtype="f32", device=None)
    for h in (sq, enc):
        _refused(lib, lib.ishara_forward_ex(h._h, None, 1, None, 0, 0, FAKE, None), "ishara_forward_ex", "ISHARA_FAMILY_KERAS_HYBRID")
        _refused(lib, lib.ishara_loss_backward_ex(h._h, None, None, 1, None, None, C.c_float(1.0), FAKE, None), "ishara_loss_backward_ex", "ISHARA_FAMILY_KERAS_HYBRID")
        _refused(lib, lib.ishara_debug_module_forward_ex(h._h, 0, None, 1, None, 0, 0, FAKE, None), "ishara_debug_module_forward_ex", "ISHARA_FAMILY_KERAS_HYBRID")
    kw = dict(dim=64, num_conv_squeeze_blocks=1, num_conv_conform_blocks=1, input_shape=(48, 36), max_batch=2)
    f16 = Model(make_config(dtype="f16", **kw), device=None)
    _refused(lib, lib.ishara_forward_ex(f16._h, None, 1, None, 0, 0, FAKE, None), "ishara_forward_ex", "ISHARA_F16", "frame lengths")
    _refused(lib, lib.ishara_debug_module_forward_ex(f16._h, 1, None, 1, None, 0, 0, FAKE, None), "ishara_debug_module_forward_ex", "ISHARA_F16")
    with pytest.raises(_lib.IsharaError, match="f16"):
        f16(torch.zeros(2, 48, 36), frame_lengths=[48, 20])
    m = Model(make_config(**kw), device=None)
    off = C.c_void_p(FAKE.value + 2)
    _refused(lib, lib.ishara_forward_ex(m._h, None, 1, None, 0, 0, off, None), "ishara_forward_ex", "4-byte")
    _refused(lib, lib.ishara_loss_backward_ex(m._h, None, None, 1, None, None, C.c_float(1.0), off, None), "ishara_loss_backward_ex", "4-byte")
    _refused(lib, lib.ishara_forward_ex(m._h, None, 1, None, 0, 0, FAKE, None), "ishara_forward_ex", "not bound")      # the lengths themselves pass
    _refused(lib, lib.ishara_frame_lengths(None, 1, 8, 4, FAKE, None), "ishara_frame_lengths", "null")
    _refused(lib, lib.ishara_frame_lengths(FAKE, 1, 0, 4, FAKE, None), "ishara_frame_lengths", "positive")


def test_the_tflite_wrappers_refuse_frame_lengths():
    from ishara_amd.tflite_batch import BatchedTFLiteModel
    from ishara_amd.tflite_model import TFLiteModel
    for cls in (TFLiteModel, BatchedTFLiteModel):
        w = cls.__new__(cls)          # the refusal comes before anything of the wrapper is touched
        with pytest.raises(ValueError, match="frame_lengths are refused"):
            w(np.zeros((4, 276), np.float32), frame_lengths=[4])
        with pytest.raises(ValueError, match="frame_lengths are refused"):
            w.predict_indices(np.zeros((4, 276), np.float32), frame_lengths=[4])


def test_shard_batch_cuts_the_lengths_with_the_batch():
    from ishara_amd import parallel
    x, y, fl = np.arange(6), np.arange(6) * 10, np.arange(6) + 100
    xs, ys, fs = parallel.shard_batch(x, y, 1, 2, frame_lengths=fl)
    assert xs.tolist() == [1, 3, 5] and ys.tolist() == [10, 30, 50] and fs.tolist() == [101, 103, 105]
    assert len(parallel.shard_batch(x, y, 0, 2)) == 2
    with pytest.raises(ValueError, match="frame_lengths"):
        parallel.shard_batch(x, y, 0, 2, frame_lengths=fl[:5])
